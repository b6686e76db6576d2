"""Times the rectangular attention core (lstc_sdpa_fwd / lstc_sdpa_bwd, csrc/attention_x.hip) at N = 2048, H = 8, d_k = d_v = 256,
dropout 0.2, no mask, for (Sq, Sk) = (49, 49), (128, 128), (257, 257), (49, 257), (257, 49), (1, 257), with torch events, and in
the same run, interleaved round by round, the square kernels as the yardstick: lstc_attn_fwd / lstc_attn_bwd without bias at
S = 49, 128, 257 and lstc_attn_cls_* at S = 257.  One line per case: ms (best of the rounds, and the spread over them), TFLOP/s on
the nominal 4 N H Sq Sk d (forward; the backward counts twice that) and that rate as a fraction of the 105 TFLOP/s exact-f32
ceiling of DESIGN 3.3b.  Usage: python tools/sdpa_time.py [--out FILE] [--rounds R]

--fewq-lib PATH runs the few-query section instead: the same core at (Sq, Sk) in {1, 2, 4, 8, 16} x {49, 257} plus SDPA_FEWQ_MAX and
SDPA_FEWQ_MAX + 1 at Sk = 257, on the product library and on PATH, a -DSDPA_FEWQ_MAX=0 build of the same commit
(tools/build_variant.sh fewq0 attention_x -DSDPA_FEWQ_MAX=0 -> build/fewq0/liblstc_hip.so), both loaded into this process and
timed in alternation round by round; lstc_attn_cls_* rides along at 1 x 257.  One line per case and library: ms, the
algorithmic bytes (forward K + V + P + Q + O, backward K + V + dK + dV + P + Q + dO + dQ, each once) and those bytes over the
time as a fraction of the 8 TB/s HBM peak - the bound of this shape is HBM, not arithmetic.  Then one
MultiHeadAttention.forward_cross call with backward at (N, Sq, Sk, d_model) = (2048, 1, 257, 2048) and (2048, 49, 257, 2048),
H = 8, fp32, split into projections, core and the rest.  --fewq-out FILE keeps the lines."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstc_vad_amd import functional as Fn  # noqa: E402

CEILING = 105.0        # TFLOP/s on the nominal count, exact-f32 MFMA
HBM_PEAK = 8.0e12      # bytes / s
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


class use_lib:
    """Route every library call of lstc_vad_amd through ``lib`` inside the block."""

    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        from lstc_vad_amd import _lib
        self.prev, _lib._lib = _lib._lib, self.lib

    def __exit__(self, *exc):
        from lstc_vad_amd import _lib
        _lib._lib = self.prev


def load_variant(path):
    """(product library, the library at ``path``), both bound in this process."""
    from lstc_vad_amd import _lib
    prod = _lib.load()
    saved = (_lib.LIB_PATH, _lib._lib)
    _lib.LIB_PATH, _lib._lib = path, None
    try:
        var = _lib.load()
    finally:
        _lib.LIB_PATH, _lib._lib = saved
    return prod, var


def fewq_section(prod, var, rounds, emit):
    m_prod, m_var = int(prod.lstc_sdpa_few_query_max()), int(var.lstc_sdpa_few_query_max())
    if m_var != 0 or m_prod < 1:
        raise SystemExit(f"--fewq-lib: expected a -DSDPA_FEWQ_MAX=0 build next to a product build, got {m_var} and {m_prod}")
    emit(f"# few-query section: N = {N}, H = {H}, d_k = d_v = {D}, dropout {P_DROP}, no mask; SDPA_FEWQ_MAX = {m_prod} (fewq) against a "
         f"-DSDPA_FEWQ_MAX=0 build of the same commit (tile), alternating round by round; best of {rounds} rounds of 5 launches, "
         f"spread = (max - min) / min; GB = algorithmic bytes, frac = GB / ms over the {HBM_PEAK / 1e12:.0f} TB/s HBM peak (the bound)")
    shapes = [(sq, sk) for sk in (49, 257) for sq in (1, 2, 4, 8, 16)]      # every row-count instantiation of the few-query kernels
    shapes += [s for s in ((m_prod, 257), (m_prod + 1, 257)) if s not in shapes]
    dev = "cuda"
    for Sq, Sk in shapes:
        fwd, bwd = sdpa_case(Sq, Sk, dev)
        runs = [("fewq" if Sq <= m_prod else "tile", prod), ("tile0", var)]
        if (Sq, Sk) == (1, 257):
            runs.append(("cls", None))
            cfwd, cbwd = cls_case(Sk, dev)
        times = {name: ([], []) for name, _ in runs}
        for _ in range(rounds):
            for name, lib in runs:
                if lib is None:
                    times[name][0].append(timed(cfwd)[0])
                    times[name][1].append(timed(cbwd)[0])
                    continue
                with use_lib(lib):
                    times[name][0].append(timed(fwd)[0])
                    times[name][1].append(timed(bwd)[0])
        kv, qo, pp = 4.0 * N * H * Sk * D, 4.0 * N * H * Sq * D, 4.0 * N * H * Sq * Sk
        nbytes = {"fwd": 2 * kv + pp + 2 * qo, "bwd": 4 * kv + pp + 3 * qo}
        for name, _ in runs:
            for what, ts in zip(("fwd", "bwd"), times[name]):
                best = min(ts)
                emit(f"{name:5s} {what} Sq {Sq:3d} Sk {Sk:3d}  {best:9.4f} ms  spread {100 * (max(ts) - best) / best:5.1f} %  "
                     f"{nbytes[what] / 1e9:7.3f} GB  frac {nbytes[what] / (best * 1e-3) / HBM_PEAK:.3f}")
        del fwd, bwd
        torch.cuda.empty_cache()


def module_section(rounds, emit):
    """One forward_cross call with backward, and its parts timed on their own: the nine projection products (three forward, three
    weight gradients, three input gradients) and the attention core; the rest is what remains (fc, LayerNorm, residual, autograd)."""
    from lstc_vad_amd.models import MultiHeadAttention
    dm, dev = 2048, "cuda"
    emit(f"# module level: MultiHeadAttention.forward_cross + backward, N = {N}, H = {H}, d_model = {dm}, d_k = d_v = {D}, fp32, dropout "
         f"0.2 / 0.1, k and v different tensors; best of {rounds} rounds of 3 calls; parts timed on their own, rest = total - parts")
    for Sq, Sk in ((1, 257), (49, 257)):
        mod = MultiHeadAttention(H, dm, D, D, layerNorm=True, attn_dropout=0.2, fc_dropout=0.1).to(dev).train()
        xq = torch.randn(N, Sq, dm, device=dev, requires_grad=True)
        xk, xv = (torch.randn(N, Sk, dm, device=dev, requires_grad=True) for _ in range(2))
        g = torch.randn(N, Sq, dm, device=dev)

        def whole():
            for t in (xq, xk, xv):
                t.grad = None
            mod.zero_grad(set_to_none=True)
            mod.forward_cross(xq, xk, xv)[0].backward(g)

        xs = [t.detach().view(-1, dm) for t in (xq, xk, xv)]
        ws = [mod.w_qs.weight.detach(), mod.w_ks.weight.detach(), mod.w_vs.weight.detach()]
        ys = [Fn.gemm(x, w, trans_b=True) for x, w in zip(xs, ws)]

        def projections():
            for x, w, y in zip(xs, ws, ys):
                Fn.gemm(x, w, trans_b=True)
                Fn.wgrad(y, x)
                Fn.gemm(y, w)

        heads = lambda t, l: t.view(N, l, H, D).transpose(1, 2)
        q4, k4, v4 = heads(ys[0], Sq), heads(ys[1], Sk), heads(ys[2], Sk)
        do4 = heads(torch.randn(N * Sq, H * D, device=dev), Sq)

        def core():
            _, p = Fn.sdpa_fwd(q4, k4, v4, 1.0 / D ** 0.5, P_DROP, SEED)
            Fn.sdpa_bwd(do4, q4, k4, v4, p, 1.0 / D ** 0.5, P_DROP, SEED)

        ts = {"total": [], "projections": [], "core": []}
        for _ in range(rounds):
            for name, fn in (("total", whole), ("projections", projections), ("core", core)):
                ts[name].append(timed(fn, 3)[0])
        best = {k: min(v) for k, v in ts.items()}
        rest = best["total"] - best["projections"] - best["core"]
        emit(f"forward_cross Sq {Sq:3d} Sk {Sk:3d}  total {best['total']:8.3f} ms (spread {100 * (max(ts['total']) - best['total']) / best['total']:4.1f} %)  "
             f"projections {best['projections']:8.3f} ms  core {best['core']:7.3f} ms  rest {rest:7.3f} ms")
        del mod, xq, xk, xv, xs, ys, q4, k4, v4, do4
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fewq-lib", default=None, help="a -DSDPA_FEWQ_MAX=0 build of liblstc_hip.so: run the few-query section")
    ap.add_argument("--fewq-out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sdpa_time.py needs a GPU: a time measured anywhere else says nothing")
    if a.fewq_lib:
        if a.rounds < 3:
            raise SystemExit("the few-query section wants at least three rounds")
        kept = []

        def emit(line):
            print(line, flush=True)
            kept.append(line)
        prod, var = load_variant(os.path.abspath(a.fewq_lib))
        fewq_section(prod, var, a.rounds, emit)
        module_section(a.rounds, emit)
        if a.fewq_out:
            with open(a.fewq_out, "w") as f:
                f.write("\n".join(kept) + "\n")
        return
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
