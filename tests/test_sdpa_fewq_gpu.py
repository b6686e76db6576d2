"""The few-query kernels behind ``lstc_sdpa_fwd`` / ``lstc_sdpa_bwd`` (csrc/attention_x.hip, Sq <= lstc_sdpa_few_query_max()) on
the GPU against the float64 restatement of tests/util_sdpa.py, at the project's bars (``util_sdpa.bar``): P within 2e-6, O, dQ,
dK, dV within 2e-5 * max|ref| + 1e-6.  N = 2, H = 2, d = 64 unless a case says otherwise."""
import pytest
import torch

from util_sdpa import MASK_KINDS, NAMES, bar, make_mask_x, sdpa_inputs, sdpa_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, H = 2, 2


def _Fn():
    from lstc_vad_amd import functional as Fn
    return Fn


def _M():
    from lstc_vad_amd import _lib
    return int(_lib.load().lstc_sdpa_few_query_max())


def _run(q, k, v, do, scale, p_drop=0.0, seed=0, mask=None):
    Fn = _Fn()
    marg = Fn.attn_mask_arg(mask, q.shape[0], q.shape[1], q.shape[2], device=DEV, Sk=k.shape[2]) if mask is not None else None
    o, probs = Fn.sdpa_fwd(q, k, v, scale, p_drop, seed, marg)
    dq, dk_, dv_ = Fn.sdpa_bwd(do, q, k, v, probs, scale, p_drop, seed, marg)
    torch.cuda.synchronize()
    return probs, o, dq, dk_, dv_


def _keep(shape, p_drop, seed):
    return _Fn().dropout_mask(shape, p_drop, seed, DEV) if p_drop > 0 else None


def _check_exact(got, ref, what):
    errs = {}
    for name, a, b in zip(NAMES, got, ref):
        a = a.double()
        assert a.shape == b.shape and torch.isfinite(a).all(), (what, name)
        errs[name] = (float((a - b).abs().max()), bar(name, b))
        print(what, name, "max|err| %.3e bar %.3e" % errs[name])
    bad = {n: e for n, e in errs.items() if e[0] > e[1]}
    assert not bad, (what, "max |err| > bar", bad)


def _case(Sq, Sk, dk, dv, seed, p_drop=0.0, kind=None, n=N, h=H):
    q, k, v, do = sdpa_inputs(n, h, Sq, Sk, dk, dv, seed, DEV)
    mask, dead = make_mask_x(kind, n, h, Sq, Sk, seed + 1) if kind else (None, None)
    keep = _keep((n, h, Sq, Sk), p_drop, seed)
    scale = 1.0 / dk ** 0.5
    ref = sdpa_reference(q, k, v, do, scale, keep, p_drop, mask)
    got = _run(q, k, v, do, scale, p_drop, seed, mask)
    return (q, k, v, do), scale, mask, dead, keep, ref, got


def test_few_query_max_is_exported_and_in_range():
    assert 1 <= _M() <= 16


SQ_OFFSETS = ("1", "2", "3", "M-1", "M", "M+1")
SK_EDGES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512)
# (Sq as an offset name, Sk): every Sq of SQ_OFFSETS and every Sk of SK_EDGES at least once; M and M + 1 meet at Sk = 257 and 512
EDGE_PAIRS = [("1", 1), ("1", 257), ("1", 512), ("2", 2), ("2", 255), ("3", 63), ("3", 256), ("M-1", 64), ("M-1", 511),
              ("M", 65), ("M", 257), ("M", 512), ("M+1", 257), ("M+1", 512)]


def _sq(name):
    M = _M()
    return {"1": 1, "2": 2, "3": 3, "M-1": max(1, M - 1), "M": M, "M+1": M + 1}[name]


def test_edge_pairs_cover_both_axes():
    assert {a for a, _ in EDGE_PAIRS} == set(SQ_OFFSETS) and {b for _, b in EDGE_PAIRS} == set(SK_EDGES)
    for sk in (257, 512):       # the switch between the two kernel families at one key length
        assert ("M", sk) in EDGE_PAIRS and ("M+1", sk) in EDGE_PAIRS


@pytest.mark.parametrize("sq_name,Sk", EDGE_PAIRS)
def test_block_and_extent_edges(sq_name, Sk):
    Sq = _sq(sq_name)
    *_, ref, got = _case(Sq, Sk, 64, 64, 1000 * Sq + Sk)
    _check_exact(got, ref, (Sq, Sk))


@pytest.mark.parametrize("n,h", [(3, 1), (1, 5)])
def test_odd_sequence_and_head_counts(n, h):
    *_, ref, got = _case(3, 145, 64, 64, 10 * n + h, p_drop=0.2, n=n, h=h)
    _check_exact(got, ref, (n, h))


@pytest.mark.parametrize("dk,dv", [(16, 16), (48, 16), (16, 272), (256, 256), (512, 512)])
def test_head_widths(dk, dv):
    *_, ref, got = _case(5, 145, dk, dv, 7 * dk + dv)
    _check_exact(got, ref, (dk, dv))


@pytest.mark.parametrize("kind", [None, "rows"])
def test_widest_heads_at_the_last_few_query_length(kind):
    """(M, 257) at d_k = d_v = 512: the largest instantiation (all of the static LDS a workgroup may have), without and with a mask."""
    Sq = _M()
    _, _, mask, dead, _, ref, got = _case(Sq, 257, 512, 512, 31 + Sq, p_drop=0.2, kind=kind)
    _check_exact(got, ref, (Sq, 257, 512, kind))
    if kind:
        _check_mask_properties(got, mask, dead, Sq, 257, (Sq, 257, 512, kind))


@pytest.mark.parametrize("sq_name,Sk", [("3", 145), ("M", 49)])
def test_dropout_replayed_from_the_counter_hash(sq_name, Sk):
    Sq = _sq(sq_name)
    _, _, _, _, keep, ref, got = _case(Sq, Sk, 64, 64, 11 * Sq + Sk, p_drop=0.2)
    frac = float(keep.float().mean())
    assert 0.7 < frac < 0.9, frac
    _check_exact(got, ref, (Sq, Sk, "p=0.2"))


def _check_mask_properties(got, mask, dead, Sq, Sk, what):
    probs, dq = got[0], got[2]
    kept = mask.to(DEV).expand(N, H, Sq, Sk)
    alive = kept.any(-1, keepdim=True).expand(N, H, Sq, Sk)
    assert bool((~kept & alive).any()) and bool((probs[~kept & alive] == 0.0).all()), (what, "masked key with non-zero probability")
    if dead is not None:
        n, i = dead
        assert not bool(kept[n, :, i].any())
        assert float((probs[n, :, i] - 1.0 / Sk).abs().max()) <= 2e-6, (what, "fully masked row is not uniform")
        assert bool((dq[n, :, i] == 0.0).all()), (what, "dQ of a fully masked row is not zero")


@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("sq_name,Sk", [("1", 49), ("7", 145), ("M", 333)])
def test_masks(sq_name, Sk, kind):
    Sq = min(7, _M()) if sq_name == "7" else _sq(sq_name)
    p_drop = 0.2
    ops, scale, mask, dead, keep, ref, got = _case(Sq, Sk, 64, 64, 13 * Sq + Sk, p_drop=p_drop, kind=kind)
    what = (Sq, Sk, kind)
    _check_exact(got, ref, what)
    _check_mask_properties(got, mask, dead, Sq, Sk, what)
    # the f64 O without the mask is more than 4 bars away wherever a key is masked: a kernel that ignores the mask cannot pass
    o_plain = sdpa_reference(*ops[:3], None, scale, keep, p_drop, None)[1]
    gap = (o_plain - ref[1]).abs().amax((1, 2, 3))
    has_masked = (~mask.expand(N, H, Sq, Sk)).reshape(N, -1).any(-1)
    assert bool(has_masked.any())
    for n in range(N):
        if bool(has_masked[n]):
            assert float(gap[n]) > 4 * bar("O", ref[1]), (what, n)


def test_key_padding_equals_the_shorter_problem():
    Sq, Sk, L = _M(), 145, 100
    q, k, v, do = sdpa_inputs(N, H, Sq, Sk, 64, 64, 17 * Sq + Sk, DEV)
    mask = (torch.arange(Sk) < L).view(1, 1, 1, Sk).expand(N, 1, 1, Sk)
    ref = sdpa_reference(q, k[:, :, :L], v[:, :, :L], do, 0.125)
    p, o, dq, dk_, dv_ = _run(q, k, v, do, 0.125, mask=mask)
    _check_exact((p[..., :L], o, dq, dk_[:, :, :L], dv_[:, :, :L]), ref, (Sq, Sk, L))
    assert bool((p[..., L:] == 0).all()) and bool((dk_[:, :, L:] == 0).all()) and bool((dv_[:, :, L:] == 0).all())


def _equal(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape and torch.equal(x, y), (what, name)


def test_strided_operands_are_bitwise_the_contiguous_call():
    Sq, Sk, d, p_drop, seed = min(4, _M()), 145, 64, 0.2, 4242
    q, k, v, do = sdpa_inputs(N, H, Sq, Sk, d, d, seed, DEV)
    mask, _ = make_mask_x("rows", N, H, Sq, Sk, seed + 1)
    base = _run(q, k, v, do, 0.125, p_drop, seed, mask)

    def token_major(t):
        tm = t.transpose(1, 2).contiguous()
        view = tm.transpose(1, 2)
        assert view.data_ptr() == tm.data_ptr() and torch.equal(view, t)
        return view
    got = _run(token_major(q), token_major(k), token_major(v), token_major(do), 0.125, p_drop, seed, mask)
    _equal(got, base, "transpose(1, 2) view")
    assert got[3].stride() == token_major(k).stride()

    def wide(ts, l, cols=3 * H * d, shift=0):
        buf = torch.randn(N * l * cols + shift, device=DEV)[shift:].view(N, l, cols)
        views = []
        for slot, t in ts:
            dst = buf[:, :, slot * H * d: (slot + 1) * H * d].view(N, l, H, d).transpose(1, 2)
            dst.copy_(t)
            views.append(dst)
        return views
    (qw,) = wide([(1, q)], Sq)
    kw, vw = wide([(0, k), (2, v)], Sk)
    _equal(_run(qw, kw, vw, do, 0.125, p_drop, seed, mask), base, "slices of a wider buffer")
    # bases that are not 16-byte aligned: the scalar-load paths, same sums
    (qu,) = wide([(1, q)], Sq, shift=1)
    ku, vu = wide([(0, k), (2, v)], Sk, shift=3)
    assert qu.data_ptr() % 16 and ku.data_ptr() % 16
    _equal(_run(qu, ku, vu, do, 0.125, p_drop, seed, mask), base, "unaligned slices")


def test_two_runs_are_bitwise_equal():
    Sq, Sk, p_drop, seed = min(5, _M()), 200, 0.2, 99
    q, k, v, do = sdpa_inputs(N, H, Sq, Sk, 64, 48, seed, DEV)
    mask, _ = make_mask_x("rows", N, H, Sq, Sk, seed + 1)
    a = _run(q, k, v, do, 0.125, p_drop, seed, mask)
    b = _run(q, k, v, do, 0.125, p_drop, seed, mask)
    _equal(a, b, "run to run")
    keep = lambda s: _keep((N, H, Sq, Sk), p_drop, s)
    assert not torch.equal(a[0] * keep(seed), a[0] * keep(seed + 1))
    assert not torch.equal(a[1], _run(q, k, v, do, 0.125, p_drop, seed + 1, mask)[1])       # the seed matters


@pytest.mark.parametrize("Sk", [49, 200])
def test_one_query_against_the_cls_kernels(Sk):
    """Sq = 1 and lstc_attn_cls_* on the same numbers: O, P and dQ, dK, dV of both lie inside the bars of one f64 restatement."""
    Fn = _Fn()
    d, seed = 64, 7 * Sk
    g = torch.Generator(device=DEV).manual_seed(seed)
    qc, doc = (torch.randn(N, H * d, device=DEV, generator=g) for _ in range(2))
    k2, v2 = (torch.randn(N * Sk, H * d, device=DEV, generator=g) for _ in range(2))
    q4, do4 = qc.view(N, 1, H, d).transpose(1, 2), doc.view(N, 1, H, d).transpose(1, 2)
    k4, v4 = k2.view(N, Sk, H, d).transpose(1, 2), v2.view(N, Sk, H, d).transpose(1, 2)
    ref = sdpa_reference(q4, k4, v4, do4, 1.0 / d ** 0.5)
    got = _run(q4, k4, v4, do4, 1.0 / d ** 0.5)
    _check_exact(got, ref, (Sk, "few-query kernels"))
    oc, pc = Fn.attn_cls_fwd(qc, k2, v2, N, Sk, H, d, d, 0.0, 0)
    dqc, dkc, dvc = Fn.attn_cls_bwd(doc, qc, k2, v2, pc, N, Sk, H, d, d, 0.0, 0)
    torch.cuda.synchronize()
    heads = lambda t, l: t.view(N, l, H, d).transpose(1, 2)
    _check_exact((pc.view(N, H, 1, Sk), heads(oc, 1), heads(dqc, 1), heads(dkc, Sk), heads(dvc, Sk)), ref, (Sk, "CLS kernels"))
