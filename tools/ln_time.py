"""Time the LayerNorm kernels (plain and pack-emitting) on one MI355X: python tools/ln_time.py [rows d] [--rounds n] [--lib path.so ...].

Extra --lib arguments name other builds of the library (another commit's liblstc_hip.so, say).  The three f32-row backward entry
points - lstc_layernorm_bwd, lstc_layernorm_bwd_drop_pack, lstc_layernorm_bwd_drop, at the n_partial functional.py gives them - are
then timed on the in-tree library and on each of those builds in turn, --rounds times over (default 5), and dx, df or the pack
and the partial planes of every build are compared bit for bit with the in-tree library's.  Exit status 1 if a build refuses an
entry point at this shape or gives other bits."""
import ctypes as C
import sys

import os
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from lstc_vad_amd import _lib
from lstc_vad_amd.functional import dev_ptr, stream_ptr

args = [a for a in sys.argv[1:]]
libs = []
while "--lib" in args:
    i = args.index("--lib")
    libs.append(args[i + 1])
    del args[i:i + 2]
rounds = 5
if "--rounds" in args:
    i = args.index("--rounds")
    rounds = int(args[i + 1])
    del args[i:i + 2]
rows, d = (int(args[0]), int(args[1])) if len(args) >= 2 else (100352, 2048)
lib = _lib.load()
dev = "cuda"
x = torch.randn(rows, d, device=dev)
dz = torch.randn(rows, d, device=dev)
gamma, beta = torch.randn(d, device=dev), torch.randn(d, device=dev)
y, dx, df = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
pk = torch.empty(int(lib.lstc_pack1_bytes(rows, d)), device=dev, dtype=torch.uint8)
seed = 0x1234567890ABCDEF


def timed(name, fn, gb, n=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        rc = fn()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / n * 1e3
    print(f"{name:42s} {us:8.1f} us  {gb / us * 1e3:7.2f} TB/s (rc {rc})", flush=True)
    return us, rc


B = rows * d * 4 / 1e9
s = stream_ptr()
P = dev_ptr


def bwd_calls(L):
    """(entry point, n_partial, GB moved, outputs, call(partial)) of the three f32-row backward entry points of library ``L``."""
    return (
        ("lstc_layernorm_bwd", 1024, 3 * B, (dx,),
         lambda part, n: L.lstc_layernorm_bwd(P(dz), P(x), P(gamma), P(mean), P(rstd), P(dx), P(part), n, rows, d, s)),
        ("lstc_layernorm_bwd_drop_pack", 768, 3.5 * B, (dx, pk[:rows * d * 2]),
         lambda part, n: L.lstc_layernorm_bwd_drop_pack(P(dz), P(x), P(gamma), P(mean), P(rstd), P(dx), P(part), n, rows, d, 0.2, seed, P(pk), s)),
        ("lstc_layernorm_bwd_drop", 768, 4 * B, (dx, df),
         lambda part, n: L.lstc_layernorm_bwd_drop(P(dz), P(x), P(gamma), P(mean), P(rstd), P(dx), P(df), P(part), n, rows, d, 0.2, seed, s)),
    )


timed("layernorm_fwd", lambda: lib.lstc_layernorm_fwd(P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), rows, d, 1e-6, s), 2 * B)
timed("layernorm_fwd_pack", lambda: lib.lstc_layernorm_fwd_pack(P(x), P(gamma), P(beta), P(y), P(mean), P(rstd), rows, d, 1e-6, P(pk), s), 2.5 * B)
timed("pack1", lambda: lib.lstc_pack1(P(y), rows, d, d, 0, P(pk), s), 1.5 * B)
timed("dropout_apply", lambda: lib.lstc_dropout_apply(P(dz), P(df), rows * d, 0.2, seed, s), 2 * B)
for npart in (512, 768, 1024):
    part = torch.empty(3, npart, d, device=dev)
    for name, _, gb, _, call in bwd_calls(lib)[:2]:
        timed(f"{name[5:]} n_partial={npart}", lambda: call(part, npart), gb)

vp, i32, i64, f32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_uint64
SIGS = {"lstc_layernorm_bwd": [vp] * 7 + [i32, i64, i32, vp],
        "lstc_layernorm_bwd_drop_pack": [vp] * 7 + [i32, i64, i32, f32, u64, vp, vp],
        "lstc_layernorm_bwd_drop": [vp] * 8 + [i32, i64, i32, f32, u64, vp]}


def bind(path):
    alt = C.CDLL(path)
    for name, sig in SIGS.items():
        fn = getattr(alt, name)
        fn.argtypes, fn.restype = sig, C.c_int
    return alt


if libs:
    builds = [("in-tree", lib)] + [(path, bind(path)) for path in libs]
    bad = 0      # entry points a build refused, and builds whose bits differ from the in-tree library's
    for k, (name, npart, gb, outs, _) in enumerate(bwd_calls(lib)):
        print(f"== {name}  rows {rows}  d {d}  n_partial {npart}")
        part = torch.empty(3, npart, d, device=dev)
        times, ref, rc = [[] for _ in builds], None, 0      # one list of times per build, in the order given
        for rnd in range(rounds):
            for b, (bname, L) in enumerate(builds):
                call = bwd_calls(L)[k][4]
                if rnd == 0:
                    for t in outs + (part,):
                        t.zero_()
                us, rc = timed(f"  round {rnd} {bname}", lambda: call(part, npart), gb)
                if rc != 0:
                    break
                times[b].append(us)
                if rnd == 0:
                    got = [t.clone() for t in outs + (part,)]
                    if ref is None:
                        ref = got
                    else:
                        same = [torch.equal(x1, x0) for x1, x0 in zip(got, ref)]
                        bad += not all(same)
                        print(f"   {bname}: outputs identical to in-tree: {same[:-1]}  partial planes identical: {same[-1]}")
            if rc != 0:
                print(f"   refused (rc {rc}): neither timed nor compared")
                bad += 1
                break
        for (bname, _), ts in zip(builds, times):
            if ts:
                ts = sorted(ts)
                print(f"   {bname:40s} min {ts[0]:8.1f}  median {ts[len(ts) // 2]:8.1f}  max {ts[-1]:8.1f} us over {len(ts)} rounds")
    sys.exit(1 if bad else 0)
