"""Times the attention core at N = 2048, H = 8, d_k = d_v = 256 for S = 128 (the short path, for continuity) and the key-tiled long
path (S = 145, 257: csrc/attention_long.hip), exact-f32 and bf16 products, with torch events.  Prints one line per (S, dtype):
ms, TFLOP/s on 4 N H S^2 d_k (forward; backward 8 N H S^2 d_k) and GB/s on the bytes the kernels must move (Q K V O + P forward;
Q K V dO P + dQ dK dV backward).  Usage: python tools/attn_long_time.py [--out FILE]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstc_vad_amd import functional as Fn  # noqa: E402
from lstc_vad_amd.models.MultiHeadAttention import relative_position_index_3d  # noqa: E402


def timed(fn, n=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda"
    N, H, dk = 2048, 8, 256
    lines = []
    for S, L in ((128, 8), (145, 9), (257, 16)):       # S = L * 16 (+ 1 CLS token for 145 / 257; 128 = a window of 8 without it)
        M = N * S
        q, k, v, do = (torch.randn(M, H * dk, device=dev) for _ in range(4))
        idx = relative_position_index_3d(L, 4).to(dev)
        tab = torch.randn((2 * L - 1) * 49, H, device=dev) * 0.1
        flop_f = 4.0 * N * H * S * S * dk
        by_f = (4 * M * H * dk + N * H * S * S) * 4.0
        by_b = (8 * M * H * dk + N * H * S * S) * 4.0
        for dtype in ("fp32", "bf16"):
            Fn.set_compute_dtype(dtype)
            try:
                best_f = best_b = 1e9
                for _ in range(2):
                    tf, (o, p) = timed(lambda: Fn.attn_fwd(q, k, v, N, S, H, dk, dk, tab, idx, 0.2, 7))
                    tb, _ = timed(lambda: Fn.attn_bwd(do, q, k, v, p, N, S, H, dk, dk, tab, idx, 0.2, 7))
                    best_f, best_b = min(best_f, tf), min(best_b, tb)
                    del o, p
            finally:
                Fn.set_compute_dtype("fp32")
            rec = dict(S=S, dtype=dtype, path="long" if S > 128 else "short", N=N, H=H, dk=dk,
                       fwd_ms=round(best_f, 4), fwd_tflops=round(flop_f / best_f / 1e9, 2), fwd_gbs=round(by_f / best_f / 1e6, 1),
                       bwd_ms=round(best_b, 4), bwd_tflops=round(2 * flop_f / best_b / 1e9, 2), bwd_gbs=round(by_b / best_b / 1e6, 1))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del q, k, v, do
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
