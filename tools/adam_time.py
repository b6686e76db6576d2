"""Time lstc_adam_multi against lstc_adagrad_multi on one MI355X: python tools/adam_time.py [--rounds 5] [--launches 20] [--step]

Both kernels run over the parameter list of the LTN-SHT model (bench.py's ltn_sht config: about 45 tensors, 101.8 M elements) in
ONE process, in alternating rounds (Adagrad, Adam, Adagrad, ...), each round the mean of --launches calls between two events; the
table gives the median and the spread of the rounds, the achieved bytes per second - Adagrad moves 20 bytes per element (reads
w, g, s; writes w, s), Adam 28 (reads w, g, m, v; writes w, m, v) - and the ratio of the medians (the traffic says 1.4).

--step adds the headline training step (bench.py's default batch, static feed) with optimizer="adagrad" and optimizer="adamw" in
fp32 and bf16 mode: median ms per step of each, for the record."""
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
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--step", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
mode, ekw, skw, drops, _ = CONFIGS["ltn_sht"]


def models():
    torch.manual_seed(0)
    enc = Encoder(n_layers=3, n_head=8, d_k=256, d_v=256, MHA_attn_dropout=drops[0], MHA_fc_dropout=drops[1], FFN_dropout=drops[2],
                  weight_init=False, **ekw).to(dev).train()
    return enc, Classifier(ekw["d_model"], drops[3]).to(dev).train()


def kernels():
    lib = _lib.load()
    enc, head = models()
    ws = [p.detach() for p in list(enc.parameters()) + list(head.parameters())]
    n = sum(w.numel() for w in ws)
    gs = [1e-3 * torch.randn_like(w) for w in ws]
    s1, s2 = [torch.zeros_like(w) for w in ws], [torch.zeros_like(w) for w in ws]
    words = torch.zeros(len(ws), dtype=torch.int32, device=dev)
    ada = (_lib.AdagradItem * len(ws))(*[(w.data_ptr(), g.data_ptr(), s.data_ptr(), w.numel(), 1e-4, 1e-3, 1e-10, 1.0)
                                         for w, g, s in zip(ws, gs, s1)])
    adam = (_lib.AdamItem * len(ws))(*[(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), w.numel(), words.data_ptr() + 4 * i, None,
                                        1e-4, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1) for i, (w, g, m, v) in enumerate(zip(ws, gs, s1, s2))])
    st = torch.cuda.current_stream().cuda_stream
    calls = {"lstc_adagrad_multi": (lambda: lib.lstc_adagrad_multi(ada, len(ws), st), 20),
             "lstc_adam_multi": (lambda: lib.lstc_adam_multi(adam, len(ws), st), 28)}
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
    print(f"{len(ws)} tensors, {n / 1e6:.1f} M elements; {a.rounds} alternating rounds of {a.launches} launches")
    med = {}
    for name, (_, bpe) in calls.items():
        t = times[name]
        med[name] = statistics.median(t)
        print(f"{name:20s} median {med[name]:8.1f} us   min {min(t):8.1f}  max {max(t):8.1f}  spread {(max(t) - min(t)) / med[name] * 100:4.1f} %   "
              f"{bpe} B/element  {bpe * n / med[name] / 1e6:6.2f} TB/s")
    print(f"ratio adam / adagrad {med['lstc_adam_multi'] / med['lstc_adagrad_multi']:.3f}   (bytes moved: 1.400)")


def steps():
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
    for dtype in ("fp32", "bf16"):
        Fn.set_compute_dtype(dtype)
        for opt in ("adagrad", "adamw", "adagrad", "adamw"):
            enc, head = models()
            ts = TrainStep(args, mode, enc, head, 1e-4, 1e-2, 1e-3, optimizer=opt)
            ms = []
            for i in range(3 + 7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ts.step(nf, af, al)
                e1.record()
                torch.cuda.synchronize()
                if i >= 3:
                    ms.append(e0.elapsed_time(e1))
            print(f"step {dtype:5s} {opt:8s} median {statistics.median(ms):8.2f} ms   min {min(ms):8.2f}  max {max(ms):8.2f}", flush=True)
            del ts, enc, head
            Fn.bump_weight_epoch()
    Fn.set_compute_dtype("fp32")


kernels()
if a.step:
    steps()
