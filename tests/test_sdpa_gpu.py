"""Rectangular attention on the GPU (csrc/attention_x.hip behind ``lstc_sdpa_fwd`` / ``lstc_sdpa_bwd``): the kernels against the
float64 restatement of tests/util_sdpa.py, and the ``ScaledDotProductAttention`` module against fixtures made by the real
reference class (tests/golden/sdpa_*.npz).

Bars are the project's own (tests/test_attention_sweep_gpu.py): against f64, P within 2e-6 and O, dQ, dK, dV within
2e-5 * max|ref| + 1e-6; against the reference fixtures forward and ``attn`` within 1e-4 and every gradient within 2e-4 of its
tensor's maximum (tests/test_attn_mask_gpu.py).  N = 2, H = 2 unless a case says otherwise."""
import numpy as np
import pytest
import torch

from util import attn_reference
from util_sdpa import MASK_KINDS, NAMES, bar, load_sdpa_case, make_mask_x, sdpa_inputs, sdpa_reference

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, H = 2, 2


def _Fn():
    from lstc_vad_amd import functional as Fn
    return Fn


def _run(q, k, v, do, scale, p_drop=0.0, seed=0, mask=None):
    """Forward and backward through functional.sdpa_fwd / sdpa_bwd with ``mask`` (a raw mask tensor or None); returns
    (P, O, dQ, dK, dV)."""
    Fn = _Fn()
    marg = Fn.attn_mask_arg(mask, q.shape[0], q.shape[1], q.shape[2], device=DEV, Sk=k.shape[2]) if mask is not None else None
    o, probs = Fn.sdpa_fwd(q, k, v, scale, p_drop, seed, marg)
    dq, dk_, dv_ = Fn.sdpa_bwd(do, q, k, v, probs, scale, p_drop, seed, marg)
    torch.cuda.synchronize()
    return probs, o, dq, dk_, dv_


def _keep(shape, p_drop, seed):
    """The dropout decisions of a launch, replayed by lstc_dropout_mask over the flat [N, H, Sq, Sk] index."""
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


# each of 1, 2, 31, 32, 33, 64, 65, 128, 129, 511, 512 at least once on each axis
EDGE_PAIRS = [(1, 1), (1, 512), (512, 1), (2, 31), (31, 2), (32, 33), (33, 32), (64, 65), (65, 64), (128, 129), (129, 128),
              (511, 32), (32, 511), (512, 64), (64, 512), (2, 128)]


def test_edge_pairs_cover_both_axes():
    values = {1, 2, 31, 32, 33, 64, 65, 128, 129, 511, 512}
    assert {a for a, _ in EDGE_PAIRS} == values and {b for _, b in EDGE_PAIRS} == values


@pytest.mark.parametrize("Sq,Sk", EDGE_PAIRS)
def test_block_edges_on_both_axes(Sq, Sk):
    *_, ref, got = _case(Sq, Sk, 64, 64, 1000 * Sq + Sk)
    _check_exact(got, ref, (Sq, Sk))


@pytest.mark.parametrize("dk,dv", [(16, 16), (48, 16), (16, 272), (256, 256), (512, 512)])
def test_head_widths(dk, dv):
    *_, ref, got = _case(33, 145, dk, dv, 7 * dk + dv)
    _check_exact(got, ref, (dk, dv))


@pytest.mark.parametrize("Sq,Sk", [(49, 145), (145, 49)])
def test_dropout_replayed_from_the_counter_hash(Sq, Sk):
    """p = 0.2: the f64 side takes its keep mask from lstc_dropout_mask over [N, H, Sq, Sk] with the launch's seed."""
    _, _, _, _, keep, ref, got = _case(Sq, Sk, 64, 64, 11 * Sq + Sk, p_drop=0.2)
    frac = float(keep.float().mean())
    assert 0.77 < frac < 0.83, frac
    _check_exact(got, ref, (Sq, Sk, "p=0.2"))


def _check_mask_properties(got, mask, dead, Sq, Sk, what):
    """Exact zeros at masked keys of rows that keep a key; fully masked rows within 2e-6 of 1 / Sk and dQ exactly 0 there."""
    probs, dq = got[0], got[2]
    kept = mask.to(DEV).expand(N, H, Sq, Sk)
    alive = kept.any(-1, keepdim=True).expand(N, H, Sq, Sk)
    assert bool((~kept & alive).any()) and bool((probs[~kept & alive] == 0.0).all()), (what, "masked key with non-zero probability")
    if dead is not None:
        n, i = dead
        assert not bool(kept[n, :, i].any())
        assert float((probs[n, :, i] - 1.0 / Sk).abs().max()) <= 2e-6, (what, "fully masked row is not uniform")
        assert bool((dq[n, :, i] == 0.0).all()), (what, "dQ of a fully masked row is not zero")
    else:
        assert bool(alive.all())


def _check_bar_sees_mask(ops, scale, keep, p_drop, mask, ref_o, what):
    """The f64 O computed WITHOUT the mask is more than 4 bars from the masked f64 O in every sequence that masks a key: a kernel
    that ignores the mask cannot pass."""
    q, k, v, _ = ops
    o_plain = sdpa_reference(q, k, v, None, scale, keep, p_drop, None)[1]
    gap = (o_plain - ref_o).abs().amax((1, 2, 3))
    has_masked = (~mask.expand(N, H, q.shape[2], k.shape[2])).reshape(N, -1).any(-1)
    assert bool(has_masked.any()), what
    for n in range(N):
        if bool(has_masked[n]):
            assert float(gap[n]) > 4 * bar("O", ref_o), (what, n, float(gap[n]), bar("O", ref_o))


@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("Sq,Sk", [(1, 49), (49, 17), (145, 49), (200, 333)])
def test_masks(Sq, Sk, kind):
    p_drop = 0.2
    ops, scale, mask, dead, keep, ref, got = _case(Sq, Sk, 64, 64, 13 * Sq + Sk, p_drop=p_drop, kind=kind)
    what = (Sq, Sk, kind)
    _check_exact(got, ref, what)
    _check_mask_properties(got, mask, dead, Sq, Sk, what)
    _check_bar_sees_mask(ops, scale, keep, p_drop, mask, ref[1], what)


@pytest.mark.parametrize("Sq,Sk,L", [(49, 145, 100), (145, 49, 17), (33, 64, 32)])
def test_key_padding_equals_the_shorter_problem(Sq, Sk, L):
    """Keys >= L masked in every sequence: P, O, dQ and the first L rows of dK, dV are the unmasked (Sq, L) problem's, within that
    problem's f64 bars; the masked keys get probability and gradient exactly 0."""
    q, k, v, do = sdpa_inputs(N, H, Sq, Sk, 64, 64, 17 * Sq + Sk, DEV)
    mask = (torch.arange(Sk) < L).view(1, 1, 1, Sk).expand(N, 1, 1, Sk)
    scale = 0.125
    ref = sdpa_reference(q, k[:, :, :L], v[:, :, :L], do, scale)
    p, o, dq, dk_, dv_ = _run(q, k, v, do, scale, mask=mask)
    _check_exact((p[..., :L], o, dq, dk_[:, :, :L], dv_[:, :, :L]), ref, (Sq, Sk, L))
    assert bool((p[..., L:] == 0).all()) and bool((dk_[:, :, L:] == 0).all()) and bool((dv_[:, :, L:] == 0).all())


def _equal(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape and torch.equal(x, y), (what, name)


def test_strided_operands_are_bitwise_the_contiguous_call():
    """A transpose(1, 2) view of a token-major [b, l, H, d] tensor, and head views into a wider [b, l, 3 H d] buffer (Q from one
    buffer, K and V from another): no copy, and bit for bit what the head-major contiguous tensors give, forward and backward."""
    Sq, Sk, d, p_drop, seed = 49, 145, 64, 0.2, 4242
    q, k, v, do = sdpa_inputs(N, H, Sq, Sk, d, d, seed, DEV)
    mask, _ = make_mask_x("rows", N, H, Sq, Sk, seed + 1)
    base = _run(q, k, v, do, 0.125, p_drop, seed, mask)

    def token_major(t):
        tm = t.transpose(1, 2).contiguous()                     # [b, l, H, d]
        view = tm.transpose(1, 2)
        assert view.data_ptr() == tm.data_ptr() and not view.is_contiguous() and torch.equal(view, t)
        return view
    got = _run(token_major(q), token_major(k), token_major(v), token_major(do), 0.125, p_drop, seed, mask)
    _equal(got, base, "transpose(1, 2) view")
    assert got[2].stride() == token_major(q).stride()          # dQ in Q's layout

    def wide(ts, l):
        buf = torch.randn(N, l, 3 * H * d, device=DEV)
        views = []
        for slot, t in ts:
            dst = buf[:, :, slot * H * d: (slot + 1) * H * d].view(N, l, H, d).transpose(1, 2)
            dst.copy_(t)
            assert dst.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr() and dst.stride() == (l * 3 * H * d, d, 3 * H * d, 1)
            views.append(dst)
        return views
    (qw,) = wide([(1, q)], Sq)
    kw, vw = wide([(0, k), (2, v)], Sk)
    got = _run(qw, kw, vw, do, 0.125, p_drop, seed, mask)
    _equal(got, base, "slices of a wider buffer")


def test_two_runs_are_bitwise_equal():
    Sq, Sk, p_drop, seed = 145, 200, 0.2, 99
    q, k, v, do = sdpa_inputs(N, H, Sq, Sk, 64, 48, seed, DEV)
    mask, _ = make_mask_x("rows", N, H, Sq, Sk, seed + 1)
    a = _run(q, k, v, do, 0.125, p_drop, seed, mask)
    b = _run(q, k, v, do, 0.125, p_drop, seed, mask)
    _equal(a, b, "run to run")
    assert not torch.equal(a[1], _run(q, k, v, do, 0.125, p_drop, seed + 1, mask)[1])       # the seed matters


@pytest.mark.parametrize("S", [49, 200])
def test_square_continuity_with_the_square_kernels(S):
    """Sq = Sk, no bias, same inputs and seed: the rectangular kernels and functional.attn_fwd / attn_bwd both lie within the f64
    bars of one restatement (the dropout index of (n, h, i, j) is the same in both families)."""
    Fn = _Fn()
    d, p_drop, seed = 64, 0.2, 5 * S
    g = torch.Generator(device=DEV).manual_seed(seed)
    q2, k2, v2, do2 = (torch.randn(N * S, H * d, device=DEV, generator=g) for _ in range(4))      # token-major, as attn_fwd takes them
    keep = _keep((N, H, S, S), p_drop, seed)
    ref_sq = attn_reference(q2, k2, v2, do2, N, S, H, d, d, None, None, keep, p_drop)[:5]
    o, probs = Fn.attn_fwd(q2, k2, v2, N, S, H, d, d, None, None, p_drop, seed)
    dq, dk_, dv_, _ = Fn.attn_bwd(do2, q2, k2, v2, probs, N, S, H, d, d, None, None, p_drop, seed)
    _check_exact((probs, o, dq, dk_, dv_), ref_sq, (S, "square kernels"))
    heads = lambda t: t.view(N, S, H, d).transpose(1, 2)
    ref = sdpa_reference(heads(q2), heads(k2), heads(v2), heads(do2), 1.0 / d ** 0.5, keep, p_drop)
    got = _run(heads(q2), heads(k2), heads(v2), heads(do2), 1.0 / d ** 0.5, p_drop, seed)
    _check_exact(got, ref, (S, "rectangular kernels"))
    # one restatement: the two f64 references are the same numbers in two layouts
    tokens = lambda t: t.transpose(1, 2).reshape(N * S, -1)
    assert torch.allclose(ref[0], ref_sq[0], rtol=0, atol=1e-12)
    for a, b in zip(ref[1:], ref_sq[1:]):
        assert torch.allclose(tokens(a), b, rtol=0, atol=1e-10)


@pytest.mark.parametrize("Sk", [49, 200])
def test_single_query_is_row_0_of_the_square_problem(Sk):
    q, k, v, _ = sdpa_inputs(N, H, Sk, Sk, 64, 64, 3 * Sk, DEV)
    p_sq, o_sq, *_ = sdpa_reference(q, k, v, None, 0.125)
    o, p = _Fn().sdpa_fwd(q[:, :, :1], k, v, 0.125)
    torch.cuda.synchronize()
    assert p.shape == (N, H, 1, Sk) and o.shape == (N, H, 1, 64)
    assert float((p.double() - p_sq[:, :, :1]).abs().max()) <= bar("P", p_sq)
    assert float((o.double() - o_sq[:, :, :1]).abs().max()) <= bar("O", o_sq[:, :, :1])


# ------------------------------------------------------------------------------------------ the module
def _module(temperature, p=0.1):
    from models.MultiHeadAttention import ScaledDotProductAttention
    return ScaledDotProductAttention(temperature, attn_dropout=p).to(DEV)


@pytest.mark.parametrize("name", ["sdpa_1x49_pad", "sdpa_49x17_rows", "sdpa_17x145", "sdpa_145x49_pad", "sdpa_200x333_rows"])
def test_module_against_reference_fixtures(name):
    z, case = load_sdpa_case(name)
    mod = _module(case["dk"] ** 0.5).eval()
    q, k, v = (torch.from_numpy(z[f]).to(DEV).requires_grad_(True) for f in ("q", "k", "v"))
    mask = torch.from_numpy(z["mask"]).to(DEV) if "mask" in z.files else None
    assert (mask is None) == (case["kind"] == "none")
    out, attn = mod(q, k, v, mask=mask)
    (out * torch.from_numpy(z["w"]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert not attn.requires_grad
    for what, a, b in (("output", out, z["output"]), ("attn", attn, z["attn"])):
        err = float((a.detach().cpu() - torch.from_numpy(b)).abs().max())
        print(name, what, "max|err| %.3e" % err)
        assert a.shape == b.shape and err <= 1e-4, (name, what, err)
    for f, t in (("grad_q", q), ("grad_k", k), ("grad_v", v)):
        ref = torch.from_numpy(z[f])
        err, top = float((t.grad.cpu() - ref).abs().max()), float(ref.abs().max())
        print(name, f, "max|err| %.3e of max %.3e" % (err, top))
        assert err <= 2e-4 * top, (name, f, err, top)


def test_module_training_returns_the_dropped_probabilities():
    """Training, p = 0.25: ``attn`` is P * keep / (1 - p) element for element with the seed the call drew, ``output`` is attn V,
    and q, k, v receive the f64 restatement's gradients; ``eval()`` returns P itself."""
    Fn = _Fn()
    Sq, Sk, d, p = 33, 70, 32, 0.25
    q, k, v, do = sdpa_inputs(N, H, Sq, Sk, d, d, 31, DEV)
    mod = _module(d ** 0.5, p).train()
    Fn.reset_rng(1234)
    seed = Fn.next_seed()
    Fn.reset_rng(1234)
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    out, attn = mod(qg, kg, vg)
    out.backward(do)
    torch.cuda.synchronize()
    keep = Fn.dropout_mask((N, H, Sq, Sk), p, seed, DEV)
    _, probs = Fn.sdpa_fwd(q, k, v, 1.0 / d ** 0.5)
    scale = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32, device=DEV)
    assert torch.equal(attn, torch.where(keep != 0, probs * scale, torch.zeros_like(probs)))
    assert 0.2 < float((attn == 0).float().mean()) < 0.3 and not attn.requires_grad
    ref = sdpa_reference(q, k, v, do, 1.0 / d ** 0.5, keep, p)
    _check_exact((probs, out.detach(), qg.grad, kg.grad, vg.grad), ref, "module, training")
    mod.eval()
    out_e, attn_e = mod(q, k, v)
    assert torch.equal(attn_e, probs) and float((attn_e.sum(-1) - 1).abs().max()) < 1e-5
    mod = _module(d ** 0.5, 0.0).train()                      # p = 0 in training: nothing dropped
    assert torch.equal(mod(q, k, v)[1], probs)


def test_module_arguments():
    """The two unused arguments are accepted, an [Sq, Sk] mask broadcasts, and the shape errors are ValueErrors."""
    Sq, Sk, d = 20, 45, 16
    q, k, v, _ = sdpa_inputs(N, H, Sq, Sk, d, 48, 5, DEV)
    mod = _module(4.0).eval()
    out, attn = mod(q, k, v)
    out2, attn2 = mod(q, k, v, None, True, 7)
    out3, attn3 = mod(q, k, v, mask=None, relative_pe=True, window_size=2)
    assert torch.equal(out, out2) and torch.equal(attn, attn2) and torch.equal(out, out3) and torch.equal(attn, attn3)
    assert out.shape == (N, H, Sq, 48) and attn.shape == (N, H, Sq, Sk)
    m2 = torch.rand(Sq, Sk, generator=torch.Generator().manual_seed(3)) >= 0.4
    m2[:, 0] = True
    o_a, p_a = mod(q, k, v, mask=m2.to(DEV))
    o_b, p_b = mod(q, k, v, mask=m2.float().view(1, 1, Sq, Sk).expand(N, H, Sq, Sk).contiguous())
    assert torch.equal(o_a, o_b) and torch.equal(p_a, p_b) and not torch.equal(p_a, attn)
    assert bool((p_a[:, :, ~m2.to(DEV)] == 0).all())
    ref = sdpa_reference(q, k, v, None, 0.25, mask=m2)
    assert float((p_a.double() - ref[0]).abs().max()) <= bar("P", ref[0])
    with pytest.raises(ValueError, match="len_k"):
        mod(q, k, v[:, :, :-1])
    with pytest.raises(ValueError, match="d_k"):
        mod(q, torch.cat([k, k], -1), v)
    with pytest.raises(ValueError):
        mod(q, k, v, mask=torch.ones(Sk, Sq, device=DEV))
