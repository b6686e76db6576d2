"""Time the EMA of the weights on one MI355X: python tools/ema_time.py [--rounds 7] [--launches 50] [--steps 3] [--no-step]

(a) lstc_ema_multi against lstc_adam_multi over the parameter list of the LTN-SHT model (bench.py's ltn_sht config: about 45
    tensors, 101.8 M elements) in ONE process, in alternating rounds (Adam, EMA, Adam, ...), each round the mean of --launches
    calls between two device events; the table gives the median and the spread of the rounds and the achieved bytes per second -
    the EMA moves 12 bytes per element (reads avg, w; writes avg), Adam 28 (reads w, g, m, v; writes w, m, v) - and the EMA's
    bytes per second over Adam's (the yardstick: not below 0.8).  The EMA words are past 1 after the warm-up calls, so the timed
    launches are blends, not copies.
(b) the headline training step (bench.py's default batch and its model construction, static feed) with and without
    ema_decay=0.999 in fp32 and bf16 mode: two TrainSteps alive side by side, alternating rounds of --steps steps each, median ms
    per step of each and their difference against (a)'s launch time."""
import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch

from bench import CONFIGS
from lstc_vad_amd import _lib
from lstc_vad_amd import functional as Fn
from lstc_vad_amd.models import Classifier, Encoder

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=50)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--no-step", action="store_true")
a = ap.parse_args()
if a.rounds < 5:
    raise SystemExit("--rounds: a median of fewer than 5 rounds is not reported")
dev = torch.device("cuda", 0)
mode, ekw, skw, drops, _ = CONFIGS["ltn_sht"]


def models():
    torch.manual_seed(0)
    enc = Encoder(n_layers=3, n_head=8, d_k=256, d_v=256, MHA_attn_dropout=drops[0], MHA_fc_dropout=drops[1], FFN_dropout=drops[2],
                  weight_init=False, **ekw).to(dev).train()
    return enc, Classifier(ekw["d_model"], drops[3]).to(dev).train()


def line(name, t, extra=""):
    med = statistics.median(t)
    print(f"{name:24s} median {med:9.2f}   min {min(t):9.2f}  max {max(t):9.2f}  spread {(max(t) - min(t)) / med * 100:4.1f} %{extra}", flush=True)
    return med


def kernels():
    lib = _lib.load()
    enc, head = models()
    ws = [p.detach() for p in list(enc.parameters()) + list(head.parameters())]
    n = sum(w.numel() for w in ws)
    gs = [1e-3 * torch.randn_like(w) for w in ws]
    m, v, avg = ([torch.zeros_like(w) for w in ws] for _ in range(3))
    words = torch.zeros(2 * len(ws), dtype=torch.int32, device=dev)
    adam = (_lib.AdamItem * len(ws))(*[(w.data_ptr(), g.data_ptr(), x.data_ptr(), y.data_ptr(), w.numel(), words.data_ptr() + 4 * i, None,
                                        1e-4, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1) for i, (w, g, x, y) in enumerate(zip(ws, gs, m, v))])
    ema = (_lib.EmaItem * len(ws))(*[(x.data_ptr(), w.data_ptr(), w.numel(), words.data_ptr() + 4 * (len(ws) + i), 0.999, 0)
                                     for i, (w, x) in enumerate(zip(ws, avg))])
    st = torch.cuda.current_stream().cuda_stream
    calls = {"lstc_adam_multi": (lambda: lib.lstc_adam_multi(adam, len(ws), st), 28),
             "lstc_ema_multi": (lambda: lib.lstc_ema_multi(ema, len(ws), st), 12)}
    times = {k: [] for k in calls}
    for fn, _ in calls.values():
        for _ in range(3):
            _lib.check(fn())
    for _ in range(a.rounds):
        for name, (fn, _) in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.launches):
                rc = fn()
            e1.record()
            torch.cuda.synchronize()
            _lib.check(rc)
            times[name].append(e0.elapsed_time(e1) / a.launches * 1e3)
    print(f"(a) {len(ws)} tensors, {n / 1e6:.1f} M elements; {a.rounds} alternating rounds of {a.launches} launches; us per call "
          "(the count-word launch in front of each update included)")
    med, rate = {}, {}
    for name, (_, bpe) in calls.items():
        rate[name] = bpe * n / statistics.median(times[name]) / 1e6
        med[name] = line(name, times[name], f"   {bpe} B/element  {rate[name]:6.2f} TB/s")
    print(f"    EMA bytes per second / Adam bytes per second {rate['lstc_ema_multi'] / rate['lstc_adam_multi']:.3f}   (yardstick: >= 0.8);"
          f"   time ratio {med['lstc_ema_multi'] / med['lstc_adam_multi']:.3f}   (bytes moved: {12 / 28:.3f})")
    return med["lstc_ema_multi"]


def steps(ema_us):
    from argparse import Namespace
    from lstc_vad_amd.engine import TrainStep
    bs, pn, L, P, d = 32, 32, skw["part_len"], skw["n_patch"], ekw["d_model"]
    args = Namespace(batch_size=bs, part_num=pn, part_len=L, n_patch=P, lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8, lambda_BCE=1.0,
                     lambda_normal=0.2, lambda_abnormal=2.0, temporal_only=False, clip_grad=False)
    gen = torch.Generator(device=dev).manual_seed(1000)
    nf = 0.5 * torch.relu(torch.randn(bs, pn * L, P, d, device=dev, generator=gen))
    af = 0.5 * torch.relu(torch.randn(bs, pn * L, P, d, device=dev, generator=gen))
    u = torch.rand(bs, pn * L, 1, device=dev, generator=gen)
    al = torch.where(u > 0.9, u, torch.zeros_like(u))
    print(f"(b) headline step ({bs} pairs x {pn} parts, static feed); {a.rounds} alternating rounds of {a.steps} steps; ms per step")
    for dtype in ("fp32", "bf16"):
        Fn.set_compute_dtype(dtype)
        tss = {}
        for name, decay in (("without EMA", None), ("ema_decay=0.999", 0.999)):
            enc, head = models()
            tss[name] = TrainStep(args, mode, enc, head, lr_encoder=1e-4, lr_head=1e-2, weight_decay=1e-3, cls_only=True, fuse_qkv="auto",
                                  ema_decay=decay)
            for _ in range(3):
                tss[name].step(nf, af, al)
        times = {k: [] for k in tss}
        for _ in range(a.rounds):
            for name, ts in tss.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.steps):
                    ts.step(nf, af, al)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.steps)
        med = {name: line(f"{dtype} {name}", t) for name, t in times.items()}
        gap = (med["ema_decay=0.999"] - med["without EMA"]) * 1e3
        print(f"    {dtype}: the step with the EMA is {gap:+.0f} us; the launch alone is {ema_us:.0f} us (a)", flush=True)
        del tss
        Fn.bump_weight_epoch()
    Fn.set_compute_dtype("fp32")


ema_us = kernels()
if not a.no_step:
    steps(ema_us)
