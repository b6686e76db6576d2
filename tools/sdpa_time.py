"""Times the rectangular attention core (lstc_sdpa_fwd / lstc_sdpa_bwd, csrc/attention_x.hip) at N = 2048, H = 8, d_k = d_v = 256,
dropout 0.2, no mask, for (Sq, Sk) = (49, 49), (128, 128), (257, 257), (49, 257), (257, 49), (1, 257), with torch events, and in
the same run, interleaved round by round, the square kernels as the yardstick: lstc_attn_fwd / lstc_attn_bwd without bias at
S = 49, 128, 257 and lstc_attn_cls_* at S = 257.  One line per case: ms (best of the rounds, and the spread over them), TFLOP/s on
the nominal 4 N H Sq Sk d (forward; the backward counts twice that) and that rate as a fraction of the 105 TFLOP/s exact-f32
ceiling of DESIGN 3.3b.  Usage: python tools/sdpa_time.py [--out FILE] [--rounds R]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstc_vad_amd import functional as Fn  # noqa: E402

CEILING = 105.0        # TFLOP/s on the nominal count, exact-f32 MFMA
N, H, D, P_DROP, SEED = 2048, 8, 256, 0.2, 7


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


def sdpa_case(Sq, Sk, dev):
    """Head-major operands; returns (forward, backward) closures."""
    q, do = (torch.randn(N, H, Sq, D, device=dev) for _ in range(2))
    k, v = (torch.randn(N, H, Sk, D, device=dev) for _ in range(2))
    state = {}

    def fwd():
        state["p"] = Fn.sdpa_fwd(q, k, v, 1.0 / D ** 0.5, P_DROP, SEED)[1]
    return fwd, lambda: Fn.sdpa_bwd(do, q, k, v, state["p"], 1.0 / D ** 0.5, P_DROP, SEED)


def square_case(S, dev):
    q, k, v, do = (torch.randn(N * S, H * D, device=dev) for _ in range(4))
    state = {}

    def fwd():
        state["p"] = Fn.attn_fwd(q, k, v, N, S, H, D, D, None, None, P_DROP, SEED)[1]
    return fwd, lambda: Fn.attn_bwd(do, q, k, v, state["p"], N, S, H, D, D, None, None, P_DROP, SEED)


def cls_case(S, dev):
    qc, doc = (torch.randn(N, H * D, device=dev) for _ in range(2))
    k, v = (torch.randn(N * S, H * D, device=dev) for _ in range(2))
    state = {}

    def fwd():
        state["p"] = Fn.attn_cls_fwd(qc, k, v, N, S, H, D, D, P_DROP, SEED)[1]
    return fwd, lambda: Fn.attn_cls_bwd(doc, qc, k, v, state["p"], N, S, H, D, D, P_DROP, SEED)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdpa_time.py needs a GPU: a time measured anywhere else says nothing")
    dev = "cuda"
    # groups of cases that are timed in alternation: each rectangular shape next to its square yardstick
    groups = [
        [("sdpa", 49, 49), ("attn", 49, 49)],
        [("sdpa", 128, 128), ("attn", 128, 128)],
        [("sdpa", 257, 257), ("attn", 257, 257)],
        [("sdpa", 49, 257), ("sdpa", 257, 49)],
        [("sdpa", 1, 257), ("attn_cls", 1, 257)],
    ]
    lines = [f"# N = {N}, H = {H}, d_k = d_v = {D}, dropout {P_DROP}, no mask, exact-f32; best of {a.rounds} interleaved rounds of 5 launches "
             f"(spread = (max - min) / min over the rounds); TFLOP/s on 4 N H Sq Sk d (backward: 8 ...); frac = of {CEILING:.0f} TFLOP/s"]
    print(lines[0], flush=True)
    for group in groups:
        made = []
        for kind, Sq, Sk in group:
            made.append(sdpa_case(Sq, Sk, dev) if kind == "sdpa" else square_case(Sq, dev) if kind == "attn" else cls_case(Sk, dev))
        times = [([], []) for _ in group]
        for _ in range(a.rounds):
            for (fwd, bwd), (tf, tb) in zip(made, times):
                tf.append(timed(fwd)[0])
                tb.append(timed(bwd)[0])
        for (kind, Sq, Sk), (tf, tb) in zip(group, times):
            flop = 4.0 * N * H * Sq * Sk * D
            name = {"sdpa": "lstc_sdpa", "attn": "lstc_attn", "attn_cls": "lstc_attn_cls"}[kind]
            for what, ts, mult in (("fwd", tf, 1.0), ("bwd", tb, 2.0)):
                best = min(ts)
                tfl = mult * flop / best / 1e9
                line = (f"{name}_{what:3s} Sq {Sq:3d} Sk {Sk:3d}  {best:9.4f} ms  spread {100 * (max(ts) - best) / best:5.1f} %  "
                        f"{tfl:7.2f} TFLOP/s  frac {tfl / CEILING:.3f}")
                print(line, flush=True)
                lines.append(line)
        del made
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
