"""The wide-range exact-logit recipe of tests/util_softmax_range.py on the host: its exactness assertions, the seeded softmax
mistakes it must see (and the old randn recipe cannot), and the float32 margin that lets tests/test_softmax_range_gpu.py keep the
project's bars.  No project kernel runs here."""
import functools
import types

import pytest
import torch

import util_softmax_range as R
from util import attn_reference
from util_mask import attn_reference_masked
from util_sdpa import sdpa_reference

SIZES = [1, 2, 33, 96, 129, 512]
N, H = 3, 2
HALFWIDTH = 30          # the masked band around a peak: the nearest kept key then lies 31^2 / 8 = 120 under the masked maximum


@functools.lru_cache(maxsize=None)
def _case(S, dk):
    return R.build(N, H, S, S, dk, seed=S + dk)


def _index(S):
    from lstc_vad_amd.models.MultiHeadAttention import relative_position_index_3d
    n = max(1, -(-(S - 1) // 16))
    return relative_position_index_3d(n, 4), (2 * n - 1) * 49


@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("S", SIZES)
def test_recipe_is_exact(S, dk):
    """``build`` runs ``verify``: bf16 round trip, three float32 summation orders bit-equal to float64, both the intended
    integers; every key is a peak.  Also: the sharp variant (S <= 129), the CLS form (one row per (n, h), every edge key a peak,
    K shared by the heads), a rectangular form, and the range the recipe promises."""
    c = _case(S, dk)
    lo, hi = float(c.logits8.min()) * R.SCALE, float(c.logits8.max()) * R.SCALE
    assert lo >= -((S - 1) ** 2) / 8 and hi <= 2 * (S - 1) ** 2 / 8
    if S == 512:
        assert lo == -(511 ** 2) / 8 and hi == 2 * 511 ** 2 / 8, (lo, hi)          # [-32640.125, +65280.25]
    if S > 2:       # neighbouring rows: maxima far apart
        top = c.logits8.max(-1).values.double() * R.SCALE
        assert float((top[..., 1:] - top[..., :-1]).abs().max()) > (S - 1) ** 2 / 16
    if S <= 129:
        sharp = R.build(N, H, S, S, dk, seed=S, sharp=True)
        assert torch.equal(sharp.logits8, 16 * R.build(N, H, S, S, dk, seed=S).logits8)
    cls = R.cls_build(S, H, dk)
    assert torch.equal(cls.k[:, 0], cls.k[:, 1])
    assert sorted(set(cls.s.reshape(-1).tolist())) == [-1, 0, 1][: cls.N * H]          # the one-row case cycles s over (n, h)
    R.build(N, H, 5, S, dk, seed=S, peaks=R.peaks_edges(N, H, 5, S), coverage=None)
    if len(R.edge_keys(S)) > N * H:
        with pytest.raises(AssertionError):
            R.build(N, H, 1, S, dk, seed=S, peaks=R.peaks_edges(N, H, 1, S), coverage="edges")       # 6 rows cannot hold the edges


def test_an_inexact_operand_is_refused():
    c = _case(33, 16)
    bad = types.SimpleNamespace(**vars(c))
    bad.q = c.q.clone()
    bad.q[0, 0, 5] += 2.0 ** -9 * bad.q[0, 0, 5].abs().max()
    with pytest.raises(AssertionError):
        R.verify(bad)


@pytest.mark.parametrize("S", [2, 33, 96])
def test_formulas_restate_the_references(S):
    """``formulas`` in float64 is the suite's float64 references (util.attn_reference, util_mask.attn_reference_masked,
    util_sdpa.sdpa_reference) on the new inputs, to float64 rounding: its float32 evaluation is then the float32 restatement of
    the reference formulas that util_rowops.tol asks for."""
    dk, dv = 64, 24
    c = _case(S, dk)
    v, do = R.values(N, H, S, S, dv, seed=S)
    index, trows = _index(S)
    table = R.bias_table(S, H, S, trows)
    keep = torch.rand(N, H, S, S, generator=torch.Generator().manual_seed(S)) >= R.P_DROP
    kept = R.peak_mask(c.peaks, S, HALFWIDTH)
    q2, k2, v2, do2 = (R.rows(t) for t in (c.q, c.k, v, do))
    near = lambda a, b: float((a - b).abs().max()) <= 1e-12 * (1.0 + float(b.abs().max()))
    for mask in (None, kept):
        f = R.formulas(c.q, c.k, v, do, R.SCALE, R.F64, R.gather_bias(table, index, S), mask, keep, R.P_DROP)
        if mask is None:
            ref = attn_reference(q2, k2, v2, do2, N, S, H, dk, dv, table, index, keep, R.P_DROP)
        else:
            ref = attn_reference_masked(q2, k2, v2, do2, N, S, H, dk, dv, table, index, keep, R.P_DROP, mask)
        got = (f["P"], R.rows(f["O"]), R.rows(f["dQ"]), R.rows(f["dK"]), R.rows(f["dV"]), R.table_grad(f["dbias"], index, trows))
        for name, a, b in zip(("P", "O", "dQ", "dK", "dV", "dtable"), got, ref):
            assert near(a, b), (S, mask is not None, name)
        x = R.formulas(c.q, c.k, v, do, R.SCALE, R.F64, None, mask, keep, R.P_DROP)
        refx = sdpa_reference(c.q, c.k, v, do, R.SCALE, keep, R.P_DROP, mask)
        for name, b in zip(("P", "O", "dQ", "dK", "dV"), refx):
            assert near(x[name], b), (S, "sdpa", mask is not None, name)


# ---------------------------------------------------------------------------------------------------- seeded mistakes

@pytest.mark.parametrize("S", [96, 512])
def test_the_old_recipe_cannot_see_a_lost_or_partial_maximum(S):
    """Why this file exists: on the sweep's recipe (randn operands, scale 1 / 8, table * 0.4) the float32 softmax without any
    maximum, and with the maximum of the first 32 keys only, stay inside the 2e-6 bar on every row."""
    g = torch.Generator().manual_seed(S)
    q, k = torch.randn(6, S, 64, generator=g), torch.randn(6, S, 64, generator=g)
    a = torch.matmul(q * 0.125, k.transpose(-1, -2)) + 0.4 * torch.randn(6, S, S, generator=g)
    ref = torch.softmax(a.double(), -1)
    for name in ("a no maximum", "b maximum of the first 32 keys"):
        assert not bool(R.failed_rows(R.MISTAKES[name](a), ref).any()), name


@pytest.mark.parametrize("dk", [16, 64])
@pytest.mark.parametrize("S", [33, 96, 129, 512])
def test_the_new_recipe_sees_every_seeded_mistake(S, dk):
    """Each float32 row softmax with one mistake leaves the 2e-6 bar or goes non-finite in at least one row; the correct float32
    softmax fails no row.  (b) is asserted from S = 96: softmax is shift-invariant, so a maximum taken over the first 32 keys is
    wrong only where the true one lies more than ~88 above it, i.e. a peak at key 32 + 27 or beyond.  At S = 33 the shortfall is
    1 / 8 and (b) is exact to rounding - asserted too, so that the reason stays on record."""
    c = _case(S, dk)
    a = (c.logits8.double() * R.SCALE).float()
    assert torch.equal(a.double(), c.logits8.double() * R.SCALE)
    kept = R.peak_mask(c.peaks, S, HALFWIDTH)
    ref = torch.softmax(a.double(), -1)
    ref_masked = torch.softmax(torch.where(kept, a.double(), torch.full_like(a, -1e9, dtype=R.F64)), -1)
    assert not bool(R.failed_rows(R.softmax_ok(a), ref).any())
    assert not bool(R.failed_rows(R.softmax_ok(a, kept), ref_masked).any())
    failed = {}
    for name, fn in R.MISTAKES.items():
        masked = name.startswith("e")
        failed[name] = int(R.failed_rows(fn(a, kept), ref_masked if masked else ref).sum())
    print(S, dk, failed)
    for name, count in failed.items():
        if name.startswith("b") and S < 96:
            assert count == 0, (S, name, count)
        else:
            assert count >= 1, (S, name, failed)
    if S == 512:        # most rows, not one lucky row
        assert failed["a no maximum"] > N * H * S // 2 and failed["b maximum of the first 32 keys"] > N * H * S // 2, failed


def _one_row_cases():
    """The one-row and few-row cases exactly as tests/test_softmax_range_gpu.py builds them."""
    for S in (49, 128, 129, 512):
        yield ("cls", S), R.cls_build(S, H)
    for S, n in ((49, 256), (128, 16)):
        yield ("cls pack", S), R.cls_build(S, H, dm=1024, N=n)
    for Sq in (1, 2, 4, 8, 16):
        for Sk in (49, 512):
            yield ("few", Sq, Sk), R.few_build(Sq, Sk, H)


def test_the_one_row_cases_see_a_lost_maximum():
    """The CLS-query, cls_dot and few-query cases of the GPU file (one to sixteen rows per (n, h)): their row maxima reach above
    88, the softmax without a maximum fails at least one row of each, and the correct float32 softmax fails none.  (S = 2 holds
    no logit above 1 / 4: nothing to see there.)"""
    for name, c in _one_row_cases():
        a = (c.logits8.double() * R.SCALE).float()
        top = a.max(-1).values
        assert float(top.max()) > 88.0 and float(top.min()) == 0.0, (name, float(top.min()), float(top.max()))
        ref = torch.softmax(a.double(), -1)
        assert not bool(R.failed_rows(R.softmax_ok(a), ref).any()), name
        lost = int(R.failed_rows(R.MISTAKES["a no maximum"](a), ref).sum())
        assert lost >= 1, (name, lost)
        kept = R.peak_mask(c.peaks, c.Sk, HALFWIDTH)
        ref_masked = torch.softmax(torch.where(kept, a.double(), torch.full_like(a, -1e9, dtype=R.F64)), -1)
        late = int(R.failed_rows(R.MISTAKES["e mask fill after the maximum"](a, kept), ref_masked).sum())
        assert late >= 1, (name, late)
        print(name, "rows", top.numel(), "no maximum", lost, "fill after maximum", late, "top", float(top.max()))


# ---------------------------------------------------------------------------------------------------- the float32 margin

@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S", [33, 96, 129, 512])
def test_correct_float32_formulas_stay_within_a_quarter_of_the_bars(S, masked):
    """The condition under which the GPU file may hold the kernels to the project's bars on these inputs: the correct formulas in
    plain torch float32 (table, dropout 0.2, with and without the peak mask) lose at most a quarter of the P bar and of the O bar."""
    dk = dv = 64
    c = _case(S, dk)
    v, do = R.values(N, H, S, S, dv, seed=S)
    index, trows = _index(S)
    bias = R.gather_bias(R.bias_table(S, H, S, trows), index, S)
    keep = torch.rand(N, H, S, S, generator=torch.Generator().manual_seed(S)) >= R.P_DROP
    kept = R.peak_mask(c.peaks, S, HALFWIDTH) if masked else None
    f64 = R.formulas(c.q, c.k, v, None, R.SCALE, R.F64, bias, kept, keep, R.P_DROP)
    f32 = R.formulas(c.q, c.k, v, None, R.SCALE, R.F32, bias, kept, keep, R.P_DROP)
    for name in ("P", "O"):
        assert f32[name].dtype == R.F32 and bool(torch.isfinite(f32[name]).all())
        err, b = float((f32[name].double() - f64[name]).abs().max()), R.bar(name, f64[name])
        print(S, masked, name, f"{err:.3e} / {b:.3e}")
        assert err <= 0.25 * b, (S, name, err, b)
    zeros = float((f32["P"] == 0).double().mean())
    assert S < 96 or zeros > 0.2, zeros           # exact float32 zeros in P beyond the peak's reach
