"""Helpers of tests/test_attention_short_gpu.py: inputs as the long sweep builds them, functional.attn_fwd / attn_bwd under a
chosen LstcAttnDesc.variant and compute mode, the same calls through a raw descriptor (any operand layout, any output base, the
atomic table gradient), the float64 bars, and the dispatch table of csrc/attention.hip attn_fwd as sets of variants that must
give the same bits."""
import atexit
import ctypes as C
import os

import torch

DEV = "cuda"
NAMES = ("P", "O", "dQ", "dK", "dV", "dtable")
P_DROP = 0.2


def Fn():
    from lstc_vad_amd import functional
    return functional


def L():
    from lstc_vad_amd import _lib
    return _lib


def model_index(S):
    """The models' index for S tokens at 16 patches (wider than S - 1 whenever S - 1 < 16 L) and its table row count."""
    from lstc_vad_amd.models.MultiHeadAttention import relative_position_index_3d
    n = max(1, -(-(S - 1) // 16))
    return relative_position_index_3d(n, 4).to(DEV), (2 * n - 1) * 49


def inputs(N, S, H, dk, dv, seed):
    """Q, K [N S, H d_k], V, dO [N S, H d_v], the table (scaled by 0.4) and the models' index."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q, k = (torch.randn(N * S, H * dk, device=DEV, generator=g) for _ in range(2))
    v, do = (torch.randn(N * S, H * dv, device=DEV, generator=g) for _ in range(2))
    index, rows = model_index(S)
    table = 0.4 * torch.randn(rows, H, device=DEV, generator=g)
    return q, k, v, do, table, index


class _Hooks:
    """functional's measurement hooks and compute mode set for one call, put back afterwards."""

    def __init__(self, variant, mode, npw=0):
        self.new = (variant, npw, mode)

    def __enter__(self):
        F = Fn()
        self.old = (F._ATTN_VARIANT, F._BWD_NPW, F.get_compute_dtype())
        F._ATTN_VARIANT, F._BWD_NPW = self.new[:2]
        F.set_compute_dtype(self.new[2])

    def __exit__(self, *exc):
        F = Fn()
        F._ATTN_VARIANT, F._BWD_NPW = self.old[:2]
        F.set_compute_dtype(self.old[2])


def fwd(q, k, v, N, S, H, dk, dv, table, index, seed, variant=0, mode="fp32", p_drop=P_DROP):
    """(P, O) of functional.attn_fwd with functional._ATTN_VARIANT = ``variant`` in compute mode ``mode``."""
    with _Hooks(variant, mode):
        o, p = Fn().attn_fwd(q, k, v, N, S, H, dk, dv, table, index, p_drop, seed)
        torch.cuda.synchronize()
    return p, o


def bwd(do, q, k, v, probs, N, S, H, dk, dv, table, index, seed, variant=0, mode="fp32", npw=0, out=None, p_drop=P_DROP):
    """(dQ, dK, dV, dtable) of functional.attn_bwd (partial tables, summed by functional.colsum); ``npw``: sequences per
    workgroup asked for through functional._BWD_NPW (0: functional's choice); ``out``: views with the strides of Q / K / V."""
    with _Hooks(variant, mode, npw):
        if out is None:
            out = tuple(torch.empty_strided(t.shape, t.stride(), device=DEV) for t in (q, k, v))
        r = Fn().attn_bwd(do, q, k, v, probs, N, S, H, dk, dv, table, index, p_drop, seed, out=out)
        torch.cuda.synchronize()
    return r


def _desc(q, k, v, N, S, H, dk, dv, table, index, seed, variant, mode, p_drop):
    lib = L()
    d = lib.AttnDesc()
    d.N, d.S, d.H, d.dk, d.dv = N, S, H, dk, dv
    d.ldq, d.ldk, d.ldv = q.stride(0), k.stride(0), v.stride(0)
    d.dtype = lib.BF16 if mode == "bf16" else lib.F32
    if table is not None:
        d.index_ld, d.table_rows = index.shape[1], table.shape[0]
        d.table, d.index = table.data_ptr(), index.data_ptr()
    d.scale = 1.0 / (dk ** 0.5)
    d.dropout_p, d.dropout_seed = float(p_drop), int(seed)
    d.Q, d.K, d.V = q.data_ptr(), k.data_ptr(), v.data_ptr()
    d.variant = variant
    return d


def raw_fwd(q, k, v, o, N, S, H, dk, dv, table, index, seed, variant=0, mode="fp32", p_drop=P_DROP):
    """lstc_attn_fwd through a descriptor built here: O lands in the view ``o`` (any base, any row stride).  Returns (P, o)."""
    lib = L()
    for t in (q, k, v, o):
        assert t.is_cuda and t.dtype == torch.float32 and t.stride(1) == 1
    probs = torch.empty(N, H, S, S, device=DEV)
    d = _desc(q, k, v, N, S, H, dk, dv, table, index, seed, variant, mode, p_drop)
    d.O, d.ldo, d.probs = o.data_ptr(), o.stride(0), probs.data_ptr()
    lib.check(lib.load().lstc_attn_fwd(C.byref(d), lib.stream_ptr()), "lstc_attn_fwd")
    torch.cuda.synchronize()
    return probs, o


def raw_bwd(do, q, k, v, probs, out, N, S, H, dk, dv, table, index, seed, variant=0, mode="fp32", chunks=0, table_rows=None,
            p_drop=P_DROP):
    """lstc_attn_bwd through a descriptor built here.  ``chunks`` = 0: the table gradient by float atomics into a zeroed
    [rows, H] table; > 0: that many partial tables, summed here in float64.  Returns (dQ, dK, dV, dtable)."""
    lib = L()
    dq, dk_, dv_ = out
    for t, s in ((dq, q), (dk_, k), (dv_, v)):
        assert t.stride() == s.stride()
    d = _desc(q, k, v, N, S, H, dk, dv, table, index, seed, variant, mode, p_drop)
    d.dO, d.ldo, d.probs = do.data_ptr(), do.stride(0), probs.data_ptr()
    d.dQ, d.dK, d.dV = dq.data_ptr(), dk_.data_ptr(), dv_.data_ptr()
    dtab = None
    if table is not None:
        if table_rows is not None:
            d.table_rows = table_rows
        dtab = torch.zeros(max(chunks, 1), d.table_rows, H, device=DEV)
        d.dtable, d.dtable_chunks = dtab.data_ptr(), chunks
    lib.check(lib.load().lstc_attn_bwd(C.byref(d), lib.stream_ptr()), "lstc_attn_bwd")
    torch.cuda.synchronize()
    if dtab is not None:
        dtab = dtab[0] if chunks == 0 else dtab.double().sum(0)
    return dq, dk_, dv_, dtab


def keep_mask(N, H, S, seed, p_drop=P_DROP):
    return Fn().dropout_mask((N, H, S, S), p_drop, seed, DEV) if p_drop > 0 else None


# ---------------------------------------------------------------------------------------------------- bars

def bar(name, ref):
    return 2e-6 if name == "P" else 2e-5 * float(ref.abs().max()) + 1e-6


WORST = {}      # (section, name) -> (err / bar, err, bar, case)


def _dump():
    path = os.environ.get("LSTC_ATTN_SHORT_ERRORS")
    if path and WORST:
        with open(path, "w") as f:
            f.write(f"{'section':<42} {'what':<8} {'max|err|':<13} {'bar':<12} {'err/bar':<8} at\n")
            for (sec, name), (r, e, b, case) in sorted(WORST.items()):
                f.write(f"{sec:<42} {name:<8} {e:<13.3e} {b:<12.3e} {r:<8.3f} {case}\n")


atexit.register(_dump)


def record(section, name, err, b, case):
    r = err / b
    if (section, name) not in WORST or r > WORST[(section, name)][0]:
        WORST[(section, name)] = (r, err, b, case)


def check_exact(section, got, ref, case, names=NAMES):
    """Every result finite and within its bar of the float64 reference; a ``None`` reference skips that result."""
    bad = {}
    for name, a, b in zip(names, got, ref):
        if b is None:
            continue
        a = a.double()
        assert a.shape == b.shape, (case, name, a.shape, b.shape)
        assert torch.isfinite(a).all(), (case, name)
        err, br = float((a - b).abs().max()), bar(name.split()[0], b)
        record(section, name, err, br, case)
        if err > br:
            bad[name] = (err, br)
    assert not bad, (section, case, "max |err| > bar", bad)


def check_sensitive(q, k, v, N, S, H, dk, dv, table, index, keep, ref_o, p_drop=P_DROP):
    """The O bar sees a lost key: the float64 O without key S - 1 is more than 4 bars away from the true O."""
    from util import attn_reference
    o_cut = attn_reference(q, k, v, None, N, S, H, dk, dv, table, index, keep, p_drop, cut_key=S - 1)[1]
    gap = float((o_cut - ref_o).abs().max())
    assert gap > 4 * bar("O", ref_o), (gap, bar("O", ref_o))


def rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def check_band(section, got, exact, ref, case, names=NAMES[1:]):
    """bf16 products: relative Frobenius error above 10x the exact run's (the bf16 MFMA ran) and below 8e-3 (bf16 operand
    rounding), the exact run's below 1e-5.  A reference that is zero everywhere (dQ, dK, dtable at S = 1: dA = P (dP - dP P) with
    P = 1 is 0 in every arithmetic) has no relative error: both runs must give exact zeros."""
    for name, a, e, r in zip(names, got, exact, ref):
        if r is None:
            continue
        if float(r.norm()) == 0.0:
            assert float(a.abs().max()) == 0.0 and float(e.abs().max()) == 0.0, (case, name)
            continue
        err, err_exact = rel(a, r), rel(e, r)
        record(section + " bf16 rel", name, err, 8e-3, case)
        assert err_exact < 1e-5 and 10 * err_exact < err < 8e-3, (case, name, err, err_exact)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- dispatch

def forward_groups(mode, S, dk, dv, vectorisable=True):
    """csrc/attention.hip attn_fwd as sets of LstcAttnDesc.variant values that launch the same kernel (S <= 96, no mask, row
    operands), each with the kernel's name.  ``vectorisable``: every base 16-B aligned, every row stride a multiple of 4."""
    T = -(-S // 32)
    if not vectorisable or dk % 32 or dv % 32:
        return [((0, 1, 2, 3), "first")]
    if mode == "bf16":
        return [((0, 2), "fwd2 bf16"), ((1, 3), "first")]
    if dv % 64 == 0:
        return [((0, 3), "fwd3f"), ((2,), "fwd2"), ((1,), "first")] if T != 2 else [((0, 1, 2), "first"), ((3,), "fwd3f")]
    return [((0, 2), "fwd2"), ((1, 3), "first")] if T != 2 else [((0, 1, 2, 3), "first")]


def forward_all_variants(q, k, v, N, S, H, dk, dv, table, index, seed, mode="fp32", vectorisable=True, run=None):
    """The forward under variants 0 .. 3 with the identities of ``forward_groups`` asserted on P and O, bit for bit.  Returns
    {variant: (P, O)}.  ``run(variant)``: the call, by default ``fwd`` on the given operands."""
    if run is None:
        run = lambda var: fwd(q, k, v, N, S, H, dk, dv, table, index, seed, variant=var, mode=mode)
    res = {var: run(var) for var in (0, 1, 2, 3)}
    for group, kernel in forward_groups(mode, S, dk, dv, vectorisable):
        for var in group[1:]:
            for name, a, b in zip(("P", "O"), res[group[0]], res[var]):
                assert same_bits(a, b), (mode, S, dk, dv, kernel, f"variant {group[0]} != variant {var}", name,
                                         float((a - b).abs().max()))
    return res
