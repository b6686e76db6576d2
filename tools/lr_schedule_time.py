"""Time what a learning-rate schedule adds to the optimizer launch on one MI355X: python tools/lr_schedule_time.py [--rounds 7] [--launches 50]

Three launches over the parameter list of the LTN-SHT model (bench.py's ltn_sht config: about 45 tensors, 101.8 M elements) in ONE
process, in alternating rounds (plain, scaled, schedule, plain, ...), each round the mean of --launches calls between two device
events: lstc_adagrad_multi, lstc_adagrad_multi_scaled (the same update with lr_t = lr * *lr_scale read on the device) and
lstc_lr_schedule alone (one thread, two words).  The table gives the median and the spread of the rounds; Adagrad moves 20 bytes
per element (reads w, g, s; writes w, s) whichever entry runs it.  The scale word holds 0.5 and the step word is far from its
end, so the scaled launches do the full update and the schedule launches take the cosine arm."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch

from bench import CONFIGS
from lstc_vad_amd import _lib
from lstc_vad_amd.models import Classifier, Encoder

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--launches", type=int, default=50)
a = ap.parse_args()
if a.rounds < 5:
    raise SystemExit("--rounds: a median of fewer than 5 rounds is not reported")
dev = torch.device("cuda", 0)
mode, ekw, skw, drops, _ = CONFIGS["ltn_sht"]
torch.manual_seed(0)
enc = Encoder(n_layers=3, n_head=8, d_k=256, d_v=256, MHA_attn_dropout=drops[0], MHA_fc_dropout=drops[1], FFN_dropout=drops[2],
              weight_init=False, **ekw).to(dev).train()
head = Classifier(ekw["d_model"], drops[3]).to(dev).train()
lib = _lib.load()
ws = [p.detach() for p in list(enc.parameters()) + list(head.parameters())]
n = sum(w.numel() for w in ws)
gs = [1e-3 * torch.randn_like(w) for w in ws]
ss = [torch.zeros_like(w) for w in ws]
items = (_lib.AdagradItem * len(ws))(*[(w.data_ptr(), g.data_ptr(), s.data_ptr(), w.numel(), 1e-4, 1e-3, 1e-10, 1.0) for w, g, s in zip(ws, gs, ss)])
scale = torch.full((1,), 0.5, device=dev)
step = torch.zeros(1, dtype=torch.int32, device=dev)
idle = torch.ones(1, device=dev)          # the schedule launches write here, not into the word the scaled launches read
sched = _lib.LrSchedule(_lib.LR_COSINE, 100, 1 << 30, 0, 0.0, 0.1, 0.1)
st = torch.cuda.current_stream().cuda_stream
calls = {"lstc_adagrad_multi": lambda: lib.lstc_adagrad_multi(items, len(ws), st),
         "lstc_adagrad_multi_scaled": lambda: lib.lstc_adagrad_multi_scaled(items, len(ws), scale.data_ptr(), st),
         "lstc_lr_schedule": lambda: lib.lstc_lr_schedule(ctypes.byref(sched), step.data_ptr(), idle.data_ptr(), st)}
times = {k: [] for k in calls}
for fn in calls.values():
    for _ in range(3):
        _lib.check(fn())
for _ in range(a.rounds):
    for name, fn in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.launches):
            rc = fn()
        e1.record()
        torch.cuda.synchronize()
        _lib.check(rc)
        times[name].append(e0.elapsed_time(e1) / a.launches * 1e3)
print(f"{len(ws)} tensors, {n / 1e6:.1f} M elements; {a.rounds} alternating rounds of {a.launches} launches; us per call")
med = {}
for name, t in times.items():
    med[name] = statistics.median(t)
    rate = "" if name == "lstc_lr_schedule" else f"   20 B/element  {20 * n / med[name] / 1e6:6.2f} TB/s"
    print(f"{name:28s} median {med[name]:9.2f}   min {min(t):9.2f}  max {max(t):9.2f}  spread {(max(t) - min(t)) / med[name] * 100:4.1f} %{rate}", flush=True)
print(f"    scaled / plain {med['lstc_adagrad_multi_scaled'] / med['lstc_adagrad_multi']:.4f};   "
      f"schedule launch / plain optimizer launch {med['lstc_lr_schedule'] / med['lstc_adagrad_multi']:.4f};   "
      f"step word after the run {int(step)} (3 + {a.rounds} x {a.launches})")
