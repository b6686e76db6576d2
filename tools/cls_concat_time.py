"""The CLS-concat entry points at the headline shape (N = 2048 sequences, S = 49, d = 2048): lstc_cls_concat_fwd[_pack] on the 16-B
path and on the 4-B path (input 4 bytes off a 16-B boundary), the gather entry, lstc_cls_concat_bwd, and the len and var forms
forward and backward with every length 48, so that the three layouts move the same bytes.  One line per case; LSTC_LIBRARY names
another build's liblstc_hip.so to time instead."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstc_vad_amd import _lib
from lstc_vad_amd._lib import dev_ptr, stream_ptr, check
lib = _lib.load()
DEV = "cuda"
N, S, d, P = 2048, 49, 2048, 16
L = S - 1
lo = torch.randn(N // 2, L, d, device=DEV); hi = torch.randn(N // 2, L, d, device=DEV)
off = torch.empty(lo.numel() + 1, device=DEV)[1:].view_as(lo); off.copy_(lo)
y = torch.empty(N, S, d, device=DEV)
buf = torch.empty(int(lib.lstc_pack1_bytes(N * S, d)), device=DEV, dtype=torch.uint8)
def t(fn, n=10):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
gb = (N * L * d * 4 + N * S * d * 4) / 1e9          # x read, y written (or dy read, dx written, one row less)
def show(name, us, gbytes=gb):
    print(f"cls_concat {name}: {us:.1f} us ({gbytes / us * 1e3:.2f} TB/s)", flush=True)
for name, x in (("vector", lo), ("scalar", off)):
    show(f"fwd {name}", t(lambda: check(lib.lstc_cls_concat_fwd(dev_ptr(x), dev_ptr(hi), N // 2, None, None, dev_ptr(y), N, S, d, stream_ptr()), "f")))
    show(f"fwd_pack {name}", t(lambda: check(lib.lstc_cls_concat_fwd_pack(dev_ptr(x), dev_ptr(hi), N // 2, None, None, dev_ptr(y), N, S, d, dev_ptr(buf), stream_ptr()), "p")),
         gb + N * S * d * 2 / 1e9)
del lo, hi, off
x = torch.randn(N, L, d, device=DEV)          # also the gather's bank: N * L / P clips of P patches, each read once
idx = torch.randperm(N * L // P, device=DEV)
show("gather_fwd", t(lambda: check(lib.lstc_cls_concat_gather_fwd(dev_ptr(x), N * L // P, dev_ptr(idx), P, None, None, dev_ptr(y), N, S, d, None, stream_ptr()), "g")))
lens = torch.full((N,), L, dtype=torch.int32, device=DEV)
row0 = torch.arange(N + 1, dtype=torch.int32, device=DEV) * S
dtok = torch.empty(S, d, device=DEV)
show("len_fwd", t(lambda: check(lib.lstc_cls_concat_len_fwd(dev_ptr(x), dev_ptr(lens), None, None, dev_ptr(y), N, S, d, stream_ptr()), "lf")))
show("var_fwd", t(lambda: check(lib.lstc_cls_concat_var_fwd(dev_ptr(x), dev_ptr(row0), None, None, dev_ptr(y), N, d, stream_ptr()), "vf")))
# backward: y is dy, x is dx; the len and var calls also sum the token rows (dy read a second time)
show("bwd", t(lambda: check(lib.lstc_cls_concat_bwd(dev_ptr(y), dev_ptr(x), N, S, d, 1, stream_ptr()), "b")))
show("len_bwd", t(lambda: check(lib.lstc_cls_concat_len_bwd(dev_ptr(y), dev_ptr(lens), dev_ptr(x), dev_ptr(dtok), N, S, d, 1, stream_ptr()), "lb")),
     gb + N * S * d * 4 / 1e9)
show("var_bwd", t(lambda: check(lib.lstc_cls_concat_var_bwd(dev_ptr(y), dev_ptr(row0), dev_ptr(x), dev_ptr(dtok), N, S, d, 1, stream_ptr()), "vb")),
     gb + N * S * d * 4 / 1e9)
