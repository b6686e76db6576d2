"""The GEMM references of tests/util_gemm.py, checked on the CPU before any kernel is checked against them: fma32 against libm's
fmaf (with triples built to sit within a float64 ulp of a float32 tie), the chain and the number formats against restatements,
and - for every (shape, family, dtype) the GPU file's case tables list - the tolerance rule against a float32 evaluation in
another summation order: the check that the inputs were chosen so that only a wrong kernel can fail.  CPU only."""
import ctypes
import ctypes.util

import numpy as np
import pytest
import torch

import util_gemm as G
from util import host_dropout_keep

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------- fma32
def _libm_fmaf(a, b, c):
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    f = libm.fmaf
    return np.array([f(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=np.float32)


def _tie_triples(n, rng):
    """a b + c within a float64 ulp of the midpoint of two neighbouring float32: c = X, any float32 with a large or small exponent;
    a = 1 + m 2**-23, b = +-(ulp(X) / 2) (1 - m 2**-23), so a b = +-(ulp(X) / 2) (1 - m**2 2**-46) exactly (it has < 48 bits): the sum
    misses the tie X +- ulp(X) / 2 by m**2 2**-70 |X|, far below float64's resolution at X.  float64(a b + c) lands ON the tie and
    then rounds to even; fmaf sees which side the exact sum is on."""
    X = (rng.standard_normal(n) * np.exp2(rng.integers(-60, 100, n))).astype(np.float32)      # ulp(X) / 2 stays a normal float32
    ulp = np.spacing(np.abs(X)).astype(np.float64)                    # float32 spacing at |X| (exact powers of two)
    m = rng.integers(1, 31, n).astype(np.float64)
    sign = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
    a = (1.0 + m * 2.0 ** -23).astype(np.float32)
    b = (sign * (ulp / 2) * (1.0 - m * 2.0 ** -23)).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), 1.0 + m * 2.0 ** -23) and np.array_equal(b.astype(np.float64), sign * (ulp / 2) * (1.0 - m * 2.0 ** -23))
    return a, b, X


def test_fma32_equals_libm_fmaf_where_float64_rounds_twice():
    rng = np.random.default_rng(20250)
    n = 60000
    parts = [_tie_triples(n, rng)]
    # plain triples over a wide exponent range
    e = lambda: np.exp2(rng.integers(-40, 40, n))
    parts.append(tuple((rng.standard_normal(n) * e()).astype(np.float32) for _ in range(3)))
    # cancellation: c = -float32(a b), the fused result is the product's own rounding error
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    parts.append((a, b, -(a * b)))
    # the GEMM's own regime: a running sum of magnitude ~ sqrt(K) taking one more product
    parts.append((rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32),
                  (rng.standard_normal(n) * 16).astype(np.float32)))
    a, b, c = (np.concatenate([p[i] for p in parts]) for i in range(3))
    assert a.size >= 200000
    want = _libm_fmaf(a, b, c)
    got = G.fma32(a, b, c)
    assert got.dtype == np.float32
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad[:5], a[bad[:5]], b[bad[:5]], c[bad[:5]], got[bad[:5]], want[bad[:5]])
    # the adversarial set is not tame: the float64 route rounds twice and misses fmaf on many of the tie triples
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    n_naive = int((naive.view(np.uint32) != want.view(np.uint32))[:n].sum())
    print("float64 route differs from fmaf on %d of %d tie triples" % (n_naive, n))
    assert n_naive >= n // 8


def test_fma32_scalar_and_broadcast_shapes():
    assert G.fma32(np.float32(3), np.float32(5), np.float32(7)) == np.float32(22)
    r = G.fma32(np.ones((4, 1), np.float32), np.full((1, 3), 2, np.float32), np.zeros((4, 3), np.float32))
    assert r.shape == (4, 3) and (r == 2).all()


# ------------------------------------------------------------------------------------------- chain, formats
@pytest.mark.parametrize("family", G.FAMILIES)
def test_fmaf_chain_against_float64_product(family):
    M, N, K = 37, 29, 131
    A, B = G.operands(family, M, N, K)
    ref = G.ref64(A, B)
    t = G.tolerance(ref, G.eval32(A, B), G.terms_abs(A, B))
    for order in (None, G.mfma_issue_order(K), list(range(K - 1, -1, -1))):
        c = torch.from_numpy(G.fmaf_chain(A.numpy(), B.numpy(), order=order)).to(F64)
        err = float((c - ref).abs().max())
        assert err <= t, (family, err, t)
        if family == "int":
            assert torch.equal(c, ref)
    # a sub-block is the same numbers as the whole product's sub-block
    rows, cols = np.array([0, 5, 36]), np.array([28, 3])
    whole = G.fmaf_chain(A.numpy(), B.numpy())
    assert np.array_equal(G.fmaf_chain(A.numpy(), B.numpy(), rows, cols), whole[np.ix_(rows, cols)])
    # and the chain is an ORDER: on randn another order gives other bits somewhere
    if family == "randn":
        assert not np.array_equal(whole, G.fmaf_chain(A.numpy(), B.numpy(), order=G.mfma_issue_order(K)))


def test_mfma_issue_order_is_a_permutation_with_the_documented_head():
    for K in (1, 2, 31, 32, 33, 67, 100):
        o = G.mfma_issue_order(K)
        assert sorted(o) == list(range(K))
    assert G.mfma_issue_order(32)[:6] == [0, 16, 1, 17, 2, 18] and G.mfma_issue_order(32)[16:20] == [8, 24, 9, 25]
    assert G.mfma_issue_order(36)[32:] == [32, 33, 34, 35]


def test_bf16_round_against_bit_restatement():
    g = G.gen(5)
    x = torch.cat([torch.randn(50000, generator=g) * torch.exp2(torch.randint(-60, 60, (50000,), generator=g).to(F32)),
                   torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, 3.0e38, 1e-40, -1e-40])])   # ties both ways, a denormal
    # exact ties: 1 + 2**-8 (kept part even -> down), 1 + 3 * 2**-8 (kept part odd -> up)
    assert float(G.bf16_round(torch.tensor(1.00390625))) == 1.0 and float(G.bf16_round(torch.tensor(1.01171875))) == 1.015625
    got = G.bf16_round(x).numpy().view(np.uint32)
    assert np.array_equal(got, G.bf16_round_bits(x.numpy()).view(np.uint32))
    assert ((got & 0xFFFF) == 0).all()


@pytest.mark.parametrize("family", ("randn", "range", "spike"))
def test_pack3_planes_reproduce_the_scaled_tensor(family):
    """h + l = x s to the format's bound: l = f16(x s - h) carries 11 more bits of a residual |x s - h| <= ulp16(h) / 2, so
    |x s - h - l| <= 2**-11 * 2**-11 |x s| where l is a normal f16, and half of f16's smallest subnormal (2**-25) where it is not."""
    A, _ = G.operands(family, 64, 8, 96)
    h, l, s = G.pack3_planes(A)
    assert 2 ** 14 <= float(A.abs().max()) * s < 2 ** 15
    xs = A.to(F64) * s
    bound = torch.maximum(2.0 ** -22 * xs.abs(), torch.tensor(2.0 ** -25, dtype=F64))
    assert bool(((xs - h - l).abs() <= bound).all())
    assert bool((h.abs() <= 65504).all())


def test_pack3_emulation_is_close_to_the_product_and_exact_on_integers():
    A, B = G.operands("randn", 40, 24, 100)
    ref = G.ref64(A, B)
    emu = G.pack3_emulation(A, B)
    # three of four plane products: what is left out is a_l b_l, |a_l| <= 2**-11 |a| - the sum of |terms| times 2**-22, plus the planes' own 2**-22
    assert float((emu - ref).abs().max()) <= 4 * 2.0 ** -22 * float(G.terms_abs(A, B).max())
    A, B = G.operands("int", 40, 24, 100)
    assert torch.equal(G.pack3_emulation(A, B), G.ref64(A, B))


def test_epilogue_order_on_a_hand_made_element():
    """One element through every stage, by hand: acc 3, alpha -2 -> -6; + bias 10 -> 4; relu 4; kept at p = 0.5 -> 8; + residual -1 -> 7;
    mask source > 0 keeps it; + old C 0.5 -> 7.5.  And the same with the element dropped / masked."""
    one = lambda v: torch.tensor([[v]], dtype=F64)
    kw = dict(flags=G.ALL, alpha=-2.0, bias=torch.tensor([10.0]), p=0.5, residual=one(-1.0), c_old=one(0.5))
    T, Fa = torch.tensor([[True]]), torch.tensor([[False]])
    assert float(G.epilogue(one(3.0), keep=T, relu_src=one(1.0), **kw)) == 7.5
    assert float(G.epilogue(one(3.0), keep=Fa, relu_src=one(1.0), **kw)) == -0.5        # dropped: residual + old C
    assert float(G.epilogue(one(3.0), keep=T, relu_src=one(0.0), **kw)) == 0.5          # masked at exactly 0: old C alone
    assert float(G.epilogue(one(-30.0) * -1, keep=T, relu_src=one(1.0), **kw)) == -0.5  # relu(-60 + 10) = 0
    assert float(G.terms_abs(one(3.0), one(1.0), **kw)) == (6.0 + 10.0) / 0.5 + 1.0 + 0.5


# ------------------------------------------------------------------------------------------- the rule on the reference alone
def _sweep_keys(dtype):
    seen, out = set(), []
    # the table, and the cases whose shapes follow the compute-unit count at a nominal 256 CUs
    for case in G.CASES[dtype] + [c for c in G.cu_cases(256).values() if c["dtype"] == dtype]:
        for family in G.case_families(case):
            rounded = dtype in (G.LSTC_BF16, G.LSTC_BF16P)
            key = (rounded, dtype == G.LSTC_F32X3, case["M"], case["N"], case["K"], family, case["flags"] & G.ALL, case["alpha"])
            if key not in seen:
                seen.add(key)
                out.append((case, family))
    # entries that share their operands are neighbours: the shared products and the chain are computed once per operand set
    out.sort(key=lambda cf: (cf[0]["dtype"] in (G.LSTC_BF16, G.LSTC_BF16P), cf[0]["M"], cf[0]["N"], cf[0]["K"], cf[1], cf[0]["dtype"]))
    return out


def _subset(n, rng):
    return np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 14)]))


@pytest.mark.parametrize("dtype", sorted(G.CASES), ids=[G.DTYPE_NAMES[d] for d in sorted(G.CASES)])
def test_tolerance_rule_holds_for_the_reference_alone_on_every_listed_case(dtype):
    """For every (shape, family, dtype, epilogue) of the GPU file's tables: a float32 evaluation in ANOTHER summation order - the
    k-ordered fmaf chain with the epilogue in float32, on up to 16 x 16 chosen rows and columns - stays within the case's own
    tolerance, and is exact for the ``int`` family; for the bf16 dtypes the float32 matmul of the rounded operands likewise."""
    rng = np.random.default_rng(1)
    worst = (0.0, "")
    keys = _sweep_keys(dtype)
    chains = {}
    for case, family in keys:
        M, N, K = case["M"], case["N"], case["K"]
        P = G.products(case, family)
        keep = torch.from_numpy(host_dropout_keep(np.arange(M * N, dtype=np.uint64), G.drop_p(family), 11).reshape(M, N))
        ref, f32, terms, fmt = G.case_reference(case, family, keep)
        t = G.tolerance(ref, f32, terms, fmt)
        assert t > 0 and np.isfinite(t), (case["id"], family)
        ck = (case["dtype"] in (G.LSTC_BF16, G.LSTC_BF16P), M, N, K, family)
        if ck not in chains:
            rows, cols = _subset(M, rng), _subset(N, rng)
            chains = {ck: (rows, cols, torch.from_numpy(G.fmaf_chain(P["A"].numpy(), P["B"].numpy(), rows, cols)))}
        rows, cols, chain = chains[ck]
        ix = (torch.from_numpy(rows)[:, None], torch.from_numpy(cols)[None, :])
        kw = G.epi_kwargs(case, family, P["bias"][torch.from_numpy(cols)], P["res"][ix], P["src"][ix], P["old"][ix], keep[ix])
        cand = G.epilogue(chain, **kw).to(F64)
        err = float((cand - ref[ix]).abs().max())
        if err / t > worst[0]:
            worst = (err / t, "%s %s" % (case["id"], family))
        assert err <= t, (case["id"], family, err, t)
        if family == "int":
            assert K <= 4096 and torch.equal(cand, ref[ix]) and torch.equal(f32.to(F64), ref), (case["id"], family)
            if fmt is not None:
                assert torch.equal(fmt, ref), case["id"]
        if case["dtype"] in (G.LSTC_BF16, G.LSTC_BF16P):
            assert float((f32.to(F64) - ref).abs().max()) <= t
    print("gemm reference sweep %s: %d (shape, family, dtype, epilogue) entries, worst chain err / tol %.3f (%s)" % ((G.DTYPE_NAMES[dtype], len(keys)) + worst))


# ------------------------------------------------------------------------------------------- lstc_gemm_splits
def test_gemm_splits_against_the_header_formula():
    from lstc_vad_amd import _lib
    f = _lib.load().lstc_gemm_splits
    for dtype, bk in ((G.LSTC_F32, 32), (G.LSTC_BF16, 64), (G.LSTC_F32X3, 32), (G.LSTC_BF16P, 64)):
        for K in range(1, 601):
            kt = (K + bk - 1) // bk
            for s in range(0, 21):
                want = G.gemm_splits(dtype, K, s)
                assert f(dtype, K, s) == want, (dtype, K, s)
                assert 1 <= want <= max(s, 1) and want <= kt
                per = -(-kt // max(s, 1))
                assert (want - 1) * per < kt <= want * per           # every slice owns a K tile, together they cover all of them
    assert f(G.LSTC_F32, 4224, 16) == 15 and f(G.LSTC_F32, 160, 4) == 3 and f(G.LSTC_F32, 0, 4) == 0
