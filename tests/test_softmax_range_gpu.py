"""Every attention softmax of the library at exact logits up to 6.5e4 (tests/util_softmax_range.py), arm by arm, against the float64
reference of each family (util.attn_reference, util_mask.attn_reference_masked, util_unpadded.attn_var_reference,
util_sdpa.sdpa_reference, util_ragged.cls_dot_len, util_attn_packed.model_fwd / model_bwd).

The other attention tests keep every logit within about +-6, where a lost wave maximum, a lost exchange between the lane halves, a
stale online rescale or a mask applied after the maximum all stay a hundred times under the bars.  Here the logits are exact in
f32 and in bf16 (only expf, the sum and the division round), so the standing bars hold unchanged: every output finite, P within
2e-6, O and dV within 2e-5 max|ref| + 1e-6 - in bf16 mode too for P; O of a bf16 arm (V ~ randn IS rounded there) under the
bf16 band's upper bound of 8e-3 relative.  dQ, dK and the table gradient take util_rowops.tol, 8 max(e32, 4 2^-24 B): K holds
entries up to 2.6e5 here and a plain float32 torch evaluation already uses nearly the whole sweep bar.  e32 comes from the
float32 evaluation of util_softmax_range.formulas on the CPU, never from a kernel.

scale = 1 / 8 throughout: d_k = 64 where the entry point derives 1 / sqrt(d_k), set in the descriptor otherwise (the float64
references then get d_k = 64 for their scale; they read the operand width off the tensors).  Masked rows lose their peak and its
+-30 neighbours (a superset of +-3): the nearest kept key lies 120 under the masked maximum.

LSTC_SOFTMAX_RANGE_ERRORS=<file> writes the worst error / bar per arm (profiles/softmax_range_errors.txt)."""
import ctypes as C
import functools
import types

import pytest
import torch

import util_attn_packed as AP
import util_attn_short as A
import util_ragged
import util_softmax_range as R
import util_unpadded as U
from util import attn_reference
from util_mask import attn_reference_masked, make_mask
from util_rowops import tol
from util_sdpa import make_mask_x, sdpa_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
H = 2
P = R.P_DROP
HALFWIDTH = 30
REF_DK = 64          # what the float64 references get as d_k: their scale 1 / sqrt(64) is the recipe's 1 / 8


def _Fn():
    return A.Fn()


def _dev(*ts):
    return tuple(t.to(DEV) for t in ts)


def _keep(shape, seed):
    return _Fn().dropout_mask(shape, P, seed, DEV)


# ---------------------------------------------------------------------------------------------------- square cases

@functools.lru_cache(maxsize=None)
def _square(S, dk=64, dv=64, N=3, sharp=False, round_v=False):
    """Operands of one square case, built once and never written: q4 .. do4 [N, H, S, d] on the host, q .. do [N S, H d], the table
    and the models' index on the device."""
    c = R.build(N, H, S, S, dk, seed=11 * S + dk, sharp=sharp)
    c.S, c.dv, c.seed = S, dv, 900 + S
    c.v4, c.do4 = R.values(N, H, S, S, dv, seed=S + dv)
    if round_v:
        c.v4, c.do4 = c.v4.bfloat16().float(), c.do4.bfloat16().float()
    c.q4, c.k4 = c.q, c.k
    c.q, c.k, c.v, c.do = _dev(*(R.rows(t) for t in (c.q4, c.k4, c.v4, c.do4)))
    c.index, c.trows = A.model_index(S)
    c.table = R.bias_table(S, H, S, c.trows).to(DEV)
    c.shape = (N, S, H, dk, dv)
    return c


def _tols(q4, k4, v4, do4, bias=None, kept=None, keep=None, index=None, trows=None):
    """util_rowops.tol of dQ, dK (and dtable): the float32 and float64 evaluations of the contract on the host."""
    args = (q4.cpu(), k4.cpu(), v4.cpu(), do4.cpu(), R.SCALE)
    kw = dict(bias=None if bias is None else bias.cpu(), kept=None if kept is None else kept.cpu(),
              keep=None if keep is None else keep.cpu(), p_drop=P)
    f64, f32 = R.formulas(*args, R.F64, **kw), R.formulas(*args, R.F32, **kw)
    out = {n: tol(f64[n], f32[n], f64["terms"][n]) for n in ("dQ", "dK")}
    if bias is not None:
        ix = index.cpu()
        out["dtable"] = tol(*(R.table_grad(f[n], ix, trows) for f, n in ((f64, "dbias"), (f32, "dbias"), (f64["terms"], "dbias"))))
    return out


def _square_tols(c, keep, kept=None):
    bias = R.gather_bias(c.table.cpu(), c.index.cpu(), c.S)
    return _tols(c.q4, c.k4, c.v4, c.do4, bias, kept, keep.view(c.N, H, c.S, c.S), c.index, c.trows)


def _check_fwd(arm, got, ref, case, bf16=False):
    R.check(arm, "P", got[0], ref[0], case)
    if bf16:
        assert bool(torch.isfinite(got[1]).all()), (arm, case, "O")
        rel = A.rel(got[1], ref[1])
        R.record(arm, "O rel", rel, 8e-3, case)
        assert rel < 8e-3, (arm, case, "O", rel)
    else:
        R.check(arm, "O", got[1], ref[1], case)


def _check_bwd(arm, got, ref, tols, case):
    """got, ref: (dQ, dK, dV, dtable or None)."""
    R.check(arm, "dV", got[2], ref[2], case)
    for name, a, b in zip(("dQ", "dK", "dtable"), (got[0], got[1], got[3]), (ref[0], ref[1], ref[3])):
        if b is not None:
            R.check(arm, name, a, b, case, b=tols[name])


def _raw_fwd(c, var, mode):
    """lstc_attn_fwd through util_attn_short's descriptor with scale = 1 / 8 whatever d_k is -> (P, O)."""
    lib = A.L()
    N, S, _, dk, dv = c.shape
    d = A._desc(c.q, c.k, c.v, *c.shape, c.table, c.index, c.seed, var, mode, P)
    d.scale = R.SCALE
    o, probs = torch.empty(N * S, H * dv, device=DEV), torch.empty(N, H, S, S, device=DEV)
    d.O, d.ldo, d.probs = o.data_ptr(), o.stride(0), probs.data_ptr()
    lib.check(lib.load().lstc_attn_fwd(C.byref(d), lib.stream_ptr()), "lstc_attn_fwd")
    torch.cuda.synchronize()
    return probs, o


def _raw_bwd(c, probs, var, mode="fp32"):
    """lstc_attn_bwd the same way, one partial table per sequence summed in float64 -> (dQ, dK, dV, dtable)."""
    lib = A.L()
    N = c.shape[0]
    d = A._desc(c.q, c.k, c.v, *c.shape, c.table, c.index, c.seed, var, mode, P)
    d.scale = R.SCALE
    g = tuple(torch.empty_like(t) for t in (c.q, c.k, c.v))
    parts = torch.zeros(N, c.trows, H, device=DEV)
    d.dO, d.ldo, d.probs = c.do.data_ptr(), c.do.stride(0), probs.data_ptr()
    d.dQ, d.dK, d.dV = (t.data_ptr() for t in g)
    d.dtable, d.dtable_chunks = parts.data_ptr(), N
    lib.check(lib.load().lstc_attn_bwd(C.byref(d), lib.stream_ptr()), "lstc_attn_bwd")
    torch.cuda.synchronize()
    return g + (parts.double().sum(0),)


def _reference(c, keep, mask=None):
    N, S, _, _, dv = c.shape
    if mask is None:
        return attn_reference(c.q, c.k, c.v, c.do, N, S, H, REF_DK, dv, c.table, c.index, keep, P)
    return attn_reference_masked(c.q, c.k, c.v, c.do, N, S, H, REF_DK, dv, c.table, c.index, keep, P, mask)


# ---------------------------------------------------------------------------------------------------- 1. short row-operand kernels

SHORT = [(S, 64, 64, False) for S in (2, 17, 33, 49, 65, 96)] + [(33, 32, 96, False), (81, 32, 96, False), (33, 64, 64, True), (96, 64, 64, True)]


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("S,dk,dv,sharp", SHORT)
def test_short_kernels(S, dk, dv, sharp, mode):
    """Variants 0 .. 3 (first generation, attn_fwd2, attn_fwd3f; LSTC_BF16 on the staged kernels) with the bitwise identities of
    util_attn_short.forward_groups; fp32: the backward of variants 0 and 1 on their own P."""
    c = _square(S, dk, dv, sharp=sharp)
    keep = _keep((c.N, H, S, S), c.seed)
    ref = _reference(c, keep)
    res = A.forward_all_variants(c.q, c.k, c.v, *c.shape, c.table, c.index, c.seed, mode=mode, run=lambda var: _raw_fwd(c, var, mode))
    groups = {var: name for group, name in A.forward_groups(mode, S, dk, dv) for var in group}
    for var, got in res.items():
        _check_fwd(f"1 short {mode} {groups[var]}", got, ref, (S, dk, dv, sharp, var), bf16=mode == "bf16" and "bf16" in groups[var])
    if mode == "fp32":
        tols = _square_tols(c, keep)
        for var in (0, 1):
            _check_bwd(f"1 short bwd variant {var}", _raw_bwd(c, res[var][0], var), ref[2:], tols, (S, dk, dv, sharp))


# ---------------------------------------------------------------------------------------------------- 2. packed-operand bf16 kernels

@pytest.mark.parametrize("S", [17, 49, 96])
def test_packed_operand_kernels(S):
    """attn_fwd3 / attn_bwd3 on the fused bf16 pack (N S a multiple of 256: N = 256, 256, 8): the pack holds the recipe's integers
    exactly, so P keeps the 2e-6 bar; O and dV under the packed arm's own bars against its float64 model (their bf16 output
    rounding is part of that contract); the table gradient under util_rowops.tol against the model in float32; dQ and dK below."""
    N = 8 if S == 96 else 256
    c = _square(S, N=N, round_v=True)
    keep = _keep((N, H, S, S), c.seed)
    bias = (c.table, c.index)
    p64, o64, bo = AP.model_fwd(c.q, c.k, c.v, *c.shape, *bias, keep, P)
    qkv, dop = AP.pack(torch.cat([c.q, c.k, c.v], 1)), AP.pack(c.do)
    probs, o = AP.raw_fwd3(qkv, *c.shape, *bias, c.seed, p_drop=P)
    arm = "2 packed bf16"
    R.check(arm, "P", probs[..., :S], p64, (S,))
    AP.check_out(arm, "O", AP.unpack(o, N * S, H * 64), o64, bo, S, (S,))
    pview = probs[..., :S]
    m64 = AP.model_bwd(c.do, c.q, c.k, c.v, pview, *c.shape, *bias, keep, P)
    m32 = AP.model_bwd(c.do, c.q, c.k, c.v, pview, *c.shape, *bias, keep, P, dt=torch.float32)
    outs, dtab = AP.raw_bwd3(dop, qkv, probs, *c.shape, *bias, c.seed, p_drop=P)
    g = AP.unpack(outs[0], N * S, H * 192)
    AP.check_out(arm, "dV", g[:, 256:], *m64[2], S, (S,))
    f = R.formulas(*(R.heads(t, N, S, H) for t in (c.q, c.k, c.v, c.do)), R.SCALE, R.F64, R.gather_bias(c.table, c.index, S), None, keep, P)
    terms = R.table_grad(f["terms"]["dbias"], c.index, c.trows)
    R.check(arm, "dtable", dtab, m64[3], (S,), b=tol(m64[3].cpu(), m32[3].cpu(), terms.cpu()))
    # dQ, dK: util_rowops.tol (e32 from the model WITHOUT its bf16 roundings in float32 against the same in float64) on top of
    # what the packed contract itself rounds - dA to bf16 (2^-7 bound) and the output to bf16 (2^-8 |ref|).  The rule alone is a
    # float32 bar and cannot hold a bf16 kernel; the packed bars alone fail here, because the +-32 table makes many rows one-hot,
    # where dA = P dPk - P rs cancels to float32 rounding noise and ``bound`` = sum |bf16(dA)| |K| collapses with it while K
    # holds 2.6e5 (measured on the kernel: excess up to 2.0 bound).
    plain = [AP.model_bwd(c.do, c.q, c.k, c.v, pview, *c.shape, *bias, keep, P, dt=dt, rounding=False) for dt in (torch.float64, torch.float32)]
    for i, (name, got) in enumerate((("dQ", g[:, :128]), ("dK", g[:, 128:256]))):
        r, bound = m64[i]
        assert bool(torch.isfinite(got).all()), (arm, S, name)
        t = tol(plain[0][i][0].cpu(), plain[1][i][0].cpu(), R.rows(f["terms"][name]).cpu())
        over = float(((got.double() - r).abs() - AP.BAR_STAT * r.abs() - AP.BAR_EXCESS * bound).max())
        R.record(arm, name, max(over, 0.0), t, (S,))
        print(arm, S, name, f"{over:.3e} / {t:.3e}")
        assert over <= t, (arm, S, name, over, t)


# ---------------------------------------------------------------------------------------------------- 3. key-tiled long kernels

@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("S", [97, 129, 160, 257, 449, 512])
def test_long_kernels(S, mode):
    """functional.attn_fwd / attn_bwd as the sweep reaches them: the first-generation T = 4 kernels at S = 97, the key-tiled online
    max / sum above 128 with exact-f32 and with bf16 products.  fp32 backward at S = 97, 129 and 449."""
    c = _square(S)
    keep = _keep((c.N, H, S, S), c.seed)
    ref = _reference(c, keep)
    probs, o = A.fwd(c.q, c.k, c.v, *c.shape, c.table, c.index, c.seed, mode=mode, p_drop=P)
    _check_fwd(f"3 long {mode}", (probs, o), ref, (S,), bf16=mode == "bf16" and S > 128)
    if mode == "fp32" and S in (97, 129, 449):
        got = A.bwd(c.do, c.q, c.k, c.v, probs, *c.shape, c.table, c.index, c.seed, p_drop=P)
        _check_bwd("3 long bwd", got, ref[2:], _square_tols(c, keep), (S,))


# ---------------------------------------------------------------------------------------------------- 4. masked kernels

def _head_free(kept):
    """[N, H, Sq, Sk] -> [N, 1, Sq, Sk]: kept where every head keeps."""
    return kept.all(1, keepdim=True)


def _check_mask_properties(arm, probs, dq4, kept, case):
    """Exact zeros at the masked keys of a row that keeps a key; a fully masked row uniform within 2e-6, its dQ zero."""
    kept = kept.to(DEV).expand(probs.shape)
    alive = kept.any(-1, keepdim=True).expand(probs.shape)
    assert bool((probs[~kept & alive] == 0).all()), (arm, case, "masked key with non-zero probability")
    dead = ~alive
    if bool(dead.any()):
        assert float((probs[dead] - 1.0 / probs.shape[-1]).abs().max()) <= 2e-6, (arm, case, "fully masked row is not uniform")
        if dq4 is not None:
            assert bool((dq4[dead[..., 0]] == 0).all()), (arm, case, "dQ of a fully masked row")


@pytest.mark.parametrize("kind", ["lengths", "rows", "full", "causal"])
@pytest.mark.parametrize("S", [49, 96, 145, 449])
def test_masked_kernels(S, kind):
    """lstc_attn_fwd_masked / _bwd_masked, short and key-tiled: "rows" and "full" masks also lose every second row's peak band (the
    raw logits under the mask exceed the kept maximum by 120 or more), "rows" has a fully masked row and the band makes more;
    "lengths" and "causal" cut whatever peaks lie behind them.  Backward at S = 49 and 96."""
    Fn = _Fn()
    c = _square(S)
    N = c.N
    mask, _ = make_mask(kind, N, H, S, seed=S)
    band = R.peak_mask(c.peaks, S, HALFWIDTH)
    if kind == "rows":
        mask = mask & _head_free(band)
    elif kind == "full":
        mask = mask & band
    marg = Fn.attn_mask_arg(mask, N, H, S, device=DEV)
    keep = _keep((N, H, S, S), c.seed)
    ref = _reference(c, keep, mask)
    o, probs = Fn.attn_fwd(c.q, c.k, c.v, *c.shape, c.table, c.index, P, c.seed, mask=marg)
    torch.cuda.synchronize()
    arm = "4 masked short" if S <= 96 else "4 masked long"
    _check_fwd(arm, (probs, o), ref, (S, kind))
    dq4 = None
    if S <= 96:
        got = Fn.attn_bwd(c.do, c.q, c.k, c.v, probs, *c.shape, c.table, c.index, P, c.seed, mask=marg)
        torch.cuda.synchronize()
        _check_bwd(arm + " bwd", got, ref[2:], _square_tols(c, keep, mask), (S, kind))
        dq4 = R.heads(got[0], N, S, H)
    _check_mask_properties(arm, probs, dq4, mask, (S, kind))


# ---------------------------------------------------------------------------------------------------- 5. offsets (VAR)

@functools.lru_cache(maxsize=None)
def _var_case(tokens):
    """Sequences of ``tokens`` tokens back to back: each one a one-sequence recipe case of its own S."""
    seqs = [R.build(1, H, S, S, 64, seed=5 * S + n) for n, S in enumerate(tokens)]
    vals = [R.values(1, H, S, S, 64, seed=S) for S in tokens]
    c = types.SimpleNamespace(tokens=tokens, seqs=seqs, vals=vals, seed=77 + tokens[-1])
    cat = lambda ts: torch.cat([R.rows(t) for t in ts], 0)
    c.q, c.k = cat([s.q for s in seqs]), cat([s.k for s in seqs])
    c.v, c.do = cat([v for v, _ in vals]), cat([d for _, d in vals])
    c.index, c.trows = A.model_index(max(tokens))
    c.table = R.bias_table(max(tokens), H, tokens[-1], c.trows)
    return c


@pytest.mark.parametrize("tokens,max_tokens", [((2, 33, 96, 128), None), ((2, 129, 257, 512), 512)])
def test_offset_kernels(tokens, max_tokens):
    """One launch group over sequences whose maxima differ by four orders of magnitude (token counts with the CLS token; the
    layout takes no one-token sequence, 2 is its smallest): P, O against float64 on every sequence alone, and a sequence's P
    bitwise the P it gets when launched alone.  Backward of the 128-token launch."""
    Fn = _Fn()
    c = _var_case(tokens)
    lens = [S - 1 for S in tokens]
    layout = lambda ls: Fn.unpadded_layout(ls, max_tokens=max_tokens) if max_tokens else Fn.unpadded_layout(ls)
    lay = layout(lens)
    q, k, v, do, table = _dev(c.q, c.k, c.v, c.do, c.table)
    o, probs = Fn.attn_var_fwd(q, k, v, lay, H, 64, 64, table, c.index, P, c.seed)
    torch.cuda.synchronize()
    keep = Fn.dropout_mask((lay.n_probs(H),), P, c.seed, DEV).cpu()
    ref = U.attn_var_reference(c.q, c.k, c.v, c.do, lens, H, REF_DK, 64, c.table, c.index.cpu(), keep, P)
    arm = "5 offsets" if max_tokens is None else "5 offsets long"
    _check_fwd(arm, (probs, o), ref, tokens)
    prob0 = lay.prob0(H)
    for n, L in enumerate(lens):
        r = slice(lay.row0[n], lay.row0[n + 1])
        _, alone = Fn.attn_var_fwd(q[r], k[r], v[r], layout([L]), H, 64, 64, table, c.index, 0.0, 0)
        torch.cuda.synchronize()
        assert torch.equal(alone, probs[prob0[n]:prob0[n + 1]]), (tokens, n, "P depends on the neighbours")
    if max_tokens is None:
        got = Fn.attn_var_bwd(do, q, k, v, probs, lay, H, 64, 64, table, c.index, P, c.seed)
        torch.cuda.synchronize()
        f = {R.F64: [], R.F32: []}
        for n, (s, (v4, do4)) in enumerate(zip(c.seqs, c.vals)):
            S = tokens[n]
            kp = keep[prob0[n]:prob0[n + 1]].view(1, H, S, S)
            for dt in f:
                f[dt].append(R.formulas(s.q, s.k, v4, do4, R.SCALE, dt, R.gather_bias(c.table, c.index.cpu(), S), None, kp, P))
        cat = lambda fs, name, terms=False: torch.cat([R.rows((x["terms"] if terms else x)[name]) for x in fs], 0)
        tols = {n: tol(cat(f[R.F64], n), cat(f[R.F32], n), cat(f[R.F64], n, True)) for n in ("dQ", "dK")}
        tab = lambda fs, terms=False: sum(R.table_grad((x["terms"] if terms else x)["dbias"], c.index.cpu(), c.trows) for x in fs)
        tols["dtable"] = tol(tab(f[R.F64]), tab(f[R.F32]), tab(f[R.F64], True))
        _check_bwd(arm + " bwd", got, ref[2:], tols, tokens)


# ---------------------------------------------------------------------------------------------------- 6. rectangular attention

@functools.lru_cache(maxsize=None)
def _rect(Sq, Sk, dv, few):
    if few:
        c = R.few_build(Sq, Sk, H)
    else:
        c = R.build(max(2, -(-Sk // (H * Sq)), 3 if Sq * Sk < 40000 else 2), H, Sq, Sk, 64, seed=Sq + 3 * Sk)
    N = c.N
    c.v, c.do = R.values(N, H, Sq, Sk, dv, seed=Sq * Sk + dv)
    c.seed = 300 + Sq + Sk
    return c


def _run_rect(arm, Sq, Sk, dv, few, masked, backward):
    Fn = _Fn()
    c = _rect(Sq, Sk, dv, few)
    N = c.N
    mask = marg = None
    if masked:
        mask, _ = make_mask_x("rows", N, H, Sq, Sk, seed=Sq + Sk)
        mask = mask & _head_free(R.peak_mask(c.peaks, Sk, HALFWIDTH))
        marg = Fn.attn_mask_arg(mask, N, H, Sq, device=DEV, Sk=Sk)
    q, k, v, do = _dev(c.q, c.k, c.v, c.do)
    keep = _keep((N, H, Sq, Sk), c.seed)
    ref = sdpa_reference(q, k, v, do, R.SCALE, keep, P, mask)
    o, probs = Fn.sdpa_fwd(q, k, v, R.SCALE, P, c.seed, marg)
    torch.cuda.synchronize()
    case = (Sq, Sk, dv, "masked" if masked else "plain")
    _check_fwd(arm, (probs, o), ref, case)
    dq = None
    if backward:
        dq, dk_, dv_ = Fn.sdpa_bwd(do, q, k, v, probs, R.SCALE, P, c.seed, marg)
        torch.cuda.synchronize()
        _check_bwd(arm + " bwd", (dq, dk_, dv_, None), ref[2:] + (None,), _tols(c.q, c.k, c.v, c.do, None, mask, keep), case)
    if masked:
        _check_mask_properties(arm, probs, dq, mask, case)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Sq,Sk,dv", [(33, 145, 64), (145, 33, 64), (64, 512, 64), (512, 65, 64), (33, 145, 272)])
def test_rectangular_kernels(Sq, Sk, dv, masked):
    """sdpa_fwd_kernel's two sweeps over the key tiles (the maximum, then the sum) with Sq != Sk both ways; backward at (33, 145)."""
    _run_rect("6 rectangular", Sq, Sk, dv, False, masked, backward=(Sq, Sk, dv) == (33, 145, 64))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Sk", [49, 512])
@pytest.mark.parametrize("Sq", [1, 2, 4, 8, 16])
def test_few_query_kernels(Sq, Sk, masked):
    """sdpa_fewq_fwd_kernel at every row-count instantiation; the rows' peaks are key 0, key Sk - 1 and both sides of every 32-key
    edge.  Backward at Sk = 49."""
    _run_rect("6 few-query", Sq, Sk, 64, True, masked, backward=Sk == 49)


# ---------------------------------------------------------------------------------------------------- 7. CLS-query kernels

CLS_S = [2, 49, 128, 129, 512]


@functools.lru_cache(maxsize=None)
def _cls(S, dm=64, N=None):
    c = R.cls_build(S, H, dm, N)
    c.v, c.do = R.values(c.N, H, 1, S, 64, seed=S)
    c.seed = 40 + S
    return c


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", CLS_S)
def test_cls_query_kernels(S, masked):
    """lstc_attn_cls_fwd(_masked) / _bwd: one query row per (n, h), the peaks over (n, h) at key 0, key S - 1 and both sides of
    every 32- and 64-key edge; masked: every second sequence loses its heads' peak bands (key-padding shape)."""
    Fn = _Fn()
    c = _cls(S)
    N = c.N
    mask = marg = None
    if masked:
        mask = _head_free(R.peak_mask(c.peaks, S, HALFWIDTH))                    # [N, 1, 1, S]: the odd sequences lose their bands
        marg = Fn.attn_mask_arg(mask, N, H, S, device=DEV)
    qc = c.q[:, :, 0].reshape(N, H * 64).to(DEV)
    k, v = _dev(R.rows(c.k), R.rows(c.v))
    doc = c.do[:, :, 0].reshape(N, H * 64).to(DEV)
    keep = _keep((N, H, S, S), c.seed)[:, :, :1]
    ref = sdpa_reference(*_dev(c.q, c.k, c.v, c.do), R.SCALE, keep, P, mask)
    oc, pc = Fn.attn_cls_fwd(qc, k, v, N, S, H, 64, 64, P, c.seed, mask=marg)
    dqc, dk_, dv_ = Fn.attn_cls_bwd(doc, qc, k, v, pc, N, S, H, 64, 64, P, c.seed, mask=marg)
    torch.cuda.synchronize()
    arm, case = "7 cls query", (S, "masked" if masked else "plain")
    _check_fwd(arm, (pc.view(N, H, 1, S), oc.view(N, H, 1, 64)), ref, case)
    got = (dqc.view(N, H, 1, 64), R.heads(dk_, N, S, H), R.heads(dv_, N, S, H), None)
    _check_bwd(arm + " bwd", got, ref[2:] + (None,), _tols(c.q, c.k, c.v, c.do, None, mask, keep), case)
    if masked:
        _check_mask_properties(arm, pc.view(N, H, 1, S), got[0], mask, case)


def _check_dot(arm, got, ref_p, keep0, case):
    """mode 1 of a cls_dot entry point: the probabilities at the P bar; ``out`` is the dropped P under the replayed decisions of
    query row 0 (``keep0`` [N, H, S]): exact zeros where dropped, P / (1 - p) within 2e-6 / (1 - p) of float64 elsewhere."""
    out, probs = got
    keep0 = keep0 != 0          # dropout_mask hands out bytes
    R.check(arm, "P", probs, ref_p, case)
    assert bool(torch.isfinite(out).all()), (arm, case)
    assert bool((out[~keep0] == 0).all()), (arm, case, "a dropped key is not zero")
    want = ref_p.to(DEV) * keep0.double() / (1.0 - P)
    R.check(arm, "Pd", out, want, case, b=2e-6 / (1.0 - P))
    assert bool(((out != 0) == (keep0 & (probs != 0))).all()), (arm, case, "the drop pattern is not the replayed one")


@pytest.mark.parametrize("S", [2, 49, 128])
def test_cls_dot_kernels(S):
    """lstc_cls_dot (fixed), _len and _var in mode 1 (the re-associated CLS passes take S <= 128): u = q / 8 per head against the
    one token matrix the heads share.  _len: every second sequence ends right behind its last peak; _var: the same batch through
    the offset layout, bitwise the fixed call."""
    Fn = _Fn()
    c = _cls(S)
    N = c.N
    u = (c.q[:, :, 0] * R.SCALE).contiguous()                                    # [N, H, d]
    x = c.k[:, 0].contiguous()                                                   # [N, S, d]
    ud, xd = _dev(u, x)
    full = [S] * N
    _, ref_p = util_ragged.cls_dot_len(u, x, full, 1)
    fixed = Fn.cls_dot(ud, xd, 1, None, P, c.seed)
    torch.cuda.synchronize()
    keep0 = _keep((N, H, S, S), c.seed)[:, :, 0]
    _check_dot("7 cls_dot fixed", fixed, ref_p, keep0, (S,))
    klen = [S if n % 2 == 0 else int(c.peaks[n].max()) + 1 for n in range(N)]
    _, ref_len = util_ragged.cls_dot_len(u, x, klen, 1)
    got = Fn.cls_dot_len(ud, xd, torch.tensor(klen, dtype=torch.int32, device=DEV), 1, None, P, c.seed)
    torch.cuda.synchronize()
    _check_dot("7 cls_dot len", got, ref_len, keep0, (S,))
    for n, kl in enumerate(klen):
        assert bool((got[1][n, :, kl:] == 0).all() and (got[0][n, :, kl:] == 0).all()), (S, n)
    lay = Fn.unpadded_layout([S - 1] * N, max_tokens=512)
    var = Fn.cls_dot_var(ud, xd.view(N * S, -1), lay, 1, None, P, c.seed)
    torch.cuda.synchronize()
    _check_dot("7 cls_dot var", var, ref_p, keep0, (S,))
    assert torch.equal(var[1], fixed[1]), (S, "the offset layout at equal lengths is the fixed call")


@pytest.mark.parametrize("S", [2, 49, 128])
def test_cls_dot_pack_kernel(S):
    """lstc_cls_dot_pack in mode 1 on the bf16 pack of the token matrix (d = 1024, N S a multiple of 256): the pack holds the
    recipe's integers exactly, so the P bar stands."""
    Fn = _Fn()
    N = {2: 128, 49: 256, 128: 16}[S]
    c = _cls(S, dm=1024, N=N)
    u = (c.q[:, :, 0] * R.SCALE).contiguous()
    x = c.k[:, 0].contiguous()
    _, ref_p = util_ragged.cls_dot_len(u, x, [S] * N, 1)
    ud, xd = _dev(u, x)
    with A._Hooks(0, "bf16"):
        xp = Fn.pack3(xd.view(N * S, 1024), False)
        assert torch.equal(Fn.unpack1_rows(xp).view(N, S, 1024), xd)
        got = Fn.cls_dot_pack(ud, xp, N, S, 1, None, P, c.seed)
        torch.cuda.synchronize()
    _check_dot("7 cls_dot pack", got, ref_p, _keep((N, H, S, S), c.seed)[:, :, 0], (S,))
