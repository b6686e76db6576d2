"""Attention masks on the GPU: the masked instantiations of the first-generation kernels (S <= 128), of the key-tiled kernels
(128 < S <= 512) and of the CLS-query kernels against the float64 restatement of tests/util_mask.py, and the modules against
fixtures made by the real reference ``Encoder`` with ``src_mask`` (tests/golden/mask_*.npz).

Bars are the project's own (tests/test_attention_sweep_gpu.py): against f64, P within 2e-6 and O, dQ, dK, dV, dtable within
2e-5 * max|ref| + 1e-6; bf16 products above S = 128 in the relative-Frobenius window of test_head_width_matrix; against the
reference fixtures forward 1e-4 and every gradient within 2e-4 of its maximum.  Inputs as in the sweep tests: the models' own
index, a 0.4 * randn table (|bias| < 32: -1e9f + bias is -1e9f), attention dropout 0.2; N * H stays small."""
import numpy as np
import pytest
import torch

from util import attn_reference
from util_mask import (MASK_KINDS, NAMES, attn_reference_masked, bar, key_lengths, load_mask_case, make_mask, model_index,
                       sweep_inputs)

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _Fn():
    from lstc_vad_amd import functional as Fn
    return Fn


def _run(q, k, v, do, N, S, H, dk, dv, table, index, p_drop, seed, mask, mode="fp32", out=None):
    """Forward and backward through functional.attn_fwd / attn_bwd with ``mask`` (a raw mask tensor or None); returns
    (P, O, dQ, dK, dV, dtable)."""
    Fn = _Fn()
    prev = Fn.get_compute_dtype()
    Fn.set_compute_dtype(mode)
    try:
        marg = Fn.attn_mask_arg(mask, N, H, S, device=DEV) if mask is not None else None
        o, probs = Fn.attn_fwd(q, k, v, N, S, H, dk, dv, table, index, p_drop, seed, mask=marg)
        if out is None:
            out = tuple(torch.empty_strided(t.shape, t.stride(), device=DEV) for t in (q, k, v))
        dq, dk_, dv_, dtab = Fn.attn_bwd(do, q, k, v, probs, N, S, H, dk, dv, table, index, p_drop, seed, out=out, mask=marg)
        torch.cuda.synchronize()
    finally:
        Fn.set_compute_dtype(prev)
    return probs, o, dq, dk_, dv_, dtab


def _keep(N, H, S, p_drop, seed):
    return _Fn().dropout_mask((N, H, S, S), p_drop, seed, DEV) if p_drop > 0 else None


def _check_exact(got, ref, what):
    errs = {}
    for name, a, b in zip(NAMES, got, ref):
        a = a.double()
        assert torch.isfinite(a).all(), (what, name)
        errs[name] = (float((a - b).abs().max()), bar(name, b))
        print(what, name, "max|err| %.3e bar %.3e" % errs[name])
    bad = {n: e for n, e in errs.items() if e[0] > e[1]}
    assert not bad, (what, "max |err| > bar", bad)


def _check_mask_properties(probs, mask, N, H, S, what):
    """Semantics points 2 and 3 on the kernel's own P: exact zeros at masked keys of rows that keep a key, fully masked rows
    within 2e-6 of 1 / S."""
    kept = mask.to(DEV).expand(N, H, S, S)
    alive = kept.any(-1, keepdim=True).expand(N, H, S, S)
    assert bool((probs[~kept & alive] == 0.0).all()), (what, "masked key with non-zero probability")
    dead = ~alive
    if bool(dead.any()):
        assert float((probs[dead] - 1.0 / S).abs().max()) <= 2e-6, (what, "fully masked row is not uniform")


def _check_bar_sees_mask(q, k, v, N, S, H, dk, dv, table, index, keep, p_drop, mask, ref_o, what):
    """The f64 O computed WITHOUT the mask is more than 4 bars from the masked f64 O in every sequence that has a masked key: a
    kernel that ignores the mask cannot pass."""
    o_plain = attn_reference(q, k, v, None, N, S, H, dk, dv, table, index, keep, p_drop)[1]
    gap = (o_plain - ref_o).abs().view(N, S, -1).amax((1, 2))
    has_masked = (~mask.expand(N, H, S, S)).reshape(N, -1).any(-1)
    assert bool(has_masked.any()), what
    for n in range(N):
        if bool(has_masked[n]):
            assert float(gap[n]) > 4 * bar("O", ref_o), (what, n, float(gap[n]), bar("O", ref_o))


def _case(N, S, H, dk, dv, kind, p_drop, seed, layout=None, mode="fp32"):
    q, k, v, do, table, index = sweep_inputs(N, S, H, dk, dv, seed, DEV)
    mask, info = make_mask(kind, N, H, S, seed + 1)
    keep = _keep(N, H, S, p_drop, seed)
    ref = attn_reference_masked(q, k, v, do, N, S, H, dk, dv, table, index, keep, p_drop, mask)
    ops, out = (q, k, v, do), None
    if layout is not None:
        ops = _layout(layout, (q, k, v, do))
        out = _layout(layout, tuple(torch.zeros_like(t) for t in (q, k, v, do)))[:3]
    got = _run(*ops, N, S, H, dk, dv, table, index, p_drop, seed, mask, mode=mode, out=out)
    return (q, k, v, do, table, index), mask, info, keep, ref, got


# ---------------------------------------------------------------------------------------------------- 1, 2. kernels against f64

MASK_S = [2, 17, 33, 49, 81, 96, 97, 128, 129, 160, 257, 449, 512]


@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("S", MASK_S)
def test_masked_kernels_match_float64(S, kind):
    """Every 32-row block count of both kernel families, d_k = d_v = 64, N = 3, H = 2, each mask kind."""
    N, H, d, p_drop, seed = 3, 2, 64, 0.2, 211 + S
    (q, k, v, do, table, index), mask, info, keep, ref, got = _case(N, S, H, d, d, kind, p_drop, seed)
    what = (S, kind)
    _check_exact(got, ref, what)
    _check_mask_properties(got[0], mask, N, H, S, what)
    _check_bar_sees_mask(q, k, v, N, S, H, d, d, table, index, keep, p_drop, mask, ref[1], what)


def _layout(kind, ts):
    """tests/test_attention_sweep_gpu.py ``_layout``: "odd_ld" = Q | K | V column blocks of one buffer with an odd row length,
    dO in its own odd-length rows; "offset" = every base one float past a 16-B boundary."""
    M = ts[0].shape[0]
    cols = [t.shape[1] for t in ts]
    if kind == "odd_ld":
        buf = torch.zeros(M, sum(cols[:3]) + 1, device=DEV)
        c0 = [0, cols[0], cols[0] + cols[1]]
        views = [buf[:, c: c + n] for c, n in zip(c0, cols[:3])] + [torch.zeros(M, cols[3] + 1, device=DEV)[:, : cols[3]]]
    else:
        views = [torch.zeros(t.numel() + 4, device=DEV)[1: 1 + t.numel()].view(t.shape) for t in ts]
    for dst, src in zip(views, ts):
        dst.copy_(src)
    return views


@pytest.mark.parametrize("S,dk,dv,layout", [(113, 64, 64, "odd_ld"), (113, 40, 24, None), (81, 48, 80, "offset"),
                                            (200, 64, 64, "odd_ld"), (200, 32, 128, None), (145, 80, 48, "offset")])
def test_masked_kernels_unaligned_and_unequal_widths(S, dk, dv, layout):
    """On each side of S = 128: operands whose rows or bases are not 16-B aligned (scalar operand loads) and d_k != d_v, with
    the [N, 1, S, S] mask that holds a fully masked row and a fully masked 32-key block."""
    N, H, p_drop, seed = 2, 2, 0.2, 17 * S + dk
    (q, k, v, do, table, index), mask, info, keep, ref, got = _case(N, S, H, dk, dv, "rows", p_drop, seed, layout=layout)
    what = (S, dk, dv, layout)
    _check_exact(got, ref, what)
    _check_mask_properties(got[0], mask, N, H, S, what)
    _check_bar_sees_mask(q, k, v, N, S, H, dk, dv, table, index, keep, p_drop, mask, ref[1], what)


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


@pytest.mark.parametrize("kind", ["lengths", "rows"])
@pytest.mark.parametrize("S,d", [(145, 64), (449, 128)])
def test_masked_long_kernels_bf16_products(S, d, kind):
    """bf16 products above S = 128 (the masked LSTC_BF16 instantiations): the relative-Frobenius window of
    test_head_width_matrix - above 10x the exact run's error (the bf16 path ran), below 8e-3 - and the mask's exact zeros and
    uniform rows, which do not depend on the products' precision."""
    N, H, p_drop, seed = 2, 2, 0.2, 3 * S + d
    (q, k, v, do, table, index), mask, info, keep, ref, exact = _case(N, S, H, d, d, kind, p_drop, seed)
    got = _run(q, k, v, do, N, S, H, d, d, table, index, p_drop, seed, mask, mode="bf16")
    _check_exact(exact, ref, (S, d, kind, "exact"))
    _check_mask_properties(got[0], mask, N, H, S, (S, d, kind, "bf16"))
    for name, a, e, r in zip(NAMES[1:], got[1:], exact[1:], ref[1:]):
        assert torch.isfinite(a).all(), name
        err, err_exact = _rel(a, r), _rel(e, r)
        print(S, d, kind, name, "rel err bf16 %.3e exact %.3e" % (err, err_exact))
        assert err_exact < 1e-5 and 10 * err_exact < err < 8e-3, (name, err, err_exact)


def test_masked_short_call_in_bf16_mode_computes_exact_products():
    """A masked call in bf16 mode at S <= 128 runs the first-generation kernels: exact-f32 products, bitwise the fp32-mode call."""
    N, S, H, d, p_drop, seed = 2, 81, 2, 64, 0.2, 77
    (q, k, v, do, table, index), mask, info, keep, ref, exact = _case(N, S, H, d, d, "rows", p_drop, seed)
    got = _run(q, k, v, do, N, S, H, d, d, table, index, p_drop, seed, mask, mode="bf16")
    for name, a, b in zip(NAMES, got, exact):
        assert torch.equal(a, b), name


# ---------------------------------------------------------------------------------------------------- 3. fully masked row, backward

@pytest.mark.parametrize("S", [49, 145])
def test_fully_masked_row_backward(S):
    """No gradient reaches q.k of a fully masked row: its dQ row is exactly zero, and dK does not change by a bit when that
    query's Q row is replaced (its contribution dA^T q is zero; the row's P is uniform whatever q is).  The bias-table gradient
    still receives the row's dA: it matches the f64 restatement, which is more than 4 bars away from the restatement that masks
    logit and bias alike - the bar tells the two apart."""
    N, H, d, p_drop, seed = 3, 2, 64, 0.2, 900 + S
    (q, k, v, do, table, index), mask, info, keep, ref, got = _case(N, S, H, d, d, "rows", p_drop, seed)
    n, i = info["dead_row"]
    assert i >= 1 and not bool(mask[n, 0, i].any())
    _check_exact(got, ref, (S, "dead row"))
    assert bool((got[2].view(N, S, H * d)[n, i] == 0).all()), "dQ of the fully masked row"
    assert float(ref[2].view(N, S, H * d)[n, i].abs().max()) == 0.0
    q2 = q.clone()
    q2.view(N, S, H * d)[n, i] = 3.0 * torch.randn(H * d, device=DEV)
    got2 = _run(q2, k, v, do, N, S, H, d, d, table, index, p_drop, seed, mask)
    assert torch.equal(got2[0], got[0])                            # the dead row stays uniform, the other rows never saw that q
    assert float((got2[0][n, :, i] - 1.0 / S).abs().max()) <= 2e-6
    assert torch.equal(got2[3], got[3]), "dK depends on the Q row of a fully masked query"
    assert torch.equal(got2[4], got[4]) and torch.equal(got2[5], got[5])
    other = attn_reference_masked(q, k, v, do, N, S, H, d, d, table, index, keep, p_drop, mask, fill_after_bias=True)
    gap = float((other[5] - ref[5]).abs().max())
    assert gap > 4 * bar("dtable", ref[5]), (gap, bar("dtable", ref[5]))
    for name in ("dQ", "dK", "dV"):                                # the two restatements agree on everything but the table
        j = NAMES.index(name)
        assert float((other[j] - ref[j]).abs().max()) <= 1e-12 * (1 + float(ref[j].abs().max())), name


# ---------------------------------------------------------------------------------------------------- 4. padding = a shorter sequence

@pytest.mark.parametrize("S,L", [(49, 30), (96, 33), (128, 97), (160, 97), (200, 129), (449, 300)])
def test_key_padding_equals_the_shorter_sequence(S, L):
    """Dropout 0, keys >= L masked, dO zero on the padded rows: P, O, dQ, dK, dV on [:L] are within the bars of the f64
    reference of the UNMASKED problem at S = L (the kernel's own unmasked call at S = L is checked against the same reference)."""
    N, H, d, seed = 2, 2, 64, 40 + S + L
    q, k, v, do, table, index = sweep_inputs(N, S, H, d, d, seed, DEV)
    do.view(N, S, -1)[:, L:] = 0
    mask = (torch.arange(S) < L).view(1, 1, 1, S).expand(N, 1, 1, S)
    got = _run(q, k, v, do, N, S, H, d, d, table, index, 0.0, 0, mask)
    cut = lambda t: t.view(N, S, -1)[:, :L].reshape(N * L, -1).contiguous()
    qs, ks, vs, dos = (cut(t) for t in (q, k, v, do))
    ref = attn_reference(qs, ks, vs, dos, N, L, H, d, d, table, index, None, 0.0)
    short = _run(qs, ks, vs, dos, N, L, H, d, d, table, index, 0.0, 0, None)
    got_cut = (got[0][:, :, :L, :L],) + tuple(cut(t) for t in got[1:5])
    assert bool((got[0][:, :, :, L:] == 0).all())
    _check_exact(got_cut, ref[:5], (S, L, "masked"))
    _check_exact(short[:5], ref[:5], (S, L, "short"))
    err = float((got[5].double() - ref[5]).abs().max())
    assert err <= bar("dtable", ref[5]), err


# ---------------------------------------------------------------------------------------------------- 5. reproducibility

def _chunked_bwd(monkeypatch, npw, *args, mask):
    Fn = _Fn()
    monkeypatch.setattr(Fn, "_BWD_NPW", npw)
    try:
        r = Fn.attn_bwd(*args, mask=mask)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    return r


@pytest.mark.parametrize("S", [49, 145])
@pytest.mark.parametrize("kind", ["lengths", "rows"])
def test_masked_runs_are_bit_reproducible_and_chunking_independent(S, kind, monkeypatch):
    """Two masked forward + backward runs are bitwise equal; with several sequences per backward workgroup (N = 7 in chunks of
    3) dQ, dK and dV equal the one-sequence-per-workgroup run bit for bit and the summed table gradient meets the f64 bar."""
    Fn = _Fn()
    N, H, d, p_drop, seed = 7, 2, 64, 0.2, 5 * S + 1
    q, k, v, do, table, index = sweep_inputs(N, S, H, d, d, seed, DEV)
    mask, _ = make_mask(kind, N, H, S, seed)
    a = _run(q, k, v, do, N, S, H, d, d, table, index, p_drop, seed, mask)
    b = _run(q, k, v, do, N, S, H, d, d, table, index, p_drop, seed, mask)
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), (name, "run to run")
    marg = Fn.attn_mask_arg(mask, N, H, S, device=DEV)
    args = (do, q, k, v, a[0], N, S, H, d, d, table, index, p_drop, seed)
    one = _chunked_bwd(monkeypatch, 1, *args, mask=marg)
    got = _chunked_bwd(monkeypatch, 3, *args, mask=marg)
    for name, x, y in zip(("dQ", "dK", "dV"), got[:3], one[:3]):
        assert torch.equal(x, y), (name, "chunks of 3 against chunks of 1")
    ref = attn_reference_masked(q, k, v, do, N, S, H, d, d, table, index, _keep(N, H, S, p_drop, seed), p_drop, mask)
    for r in (one, got):
        assert float((r[3].double() - ref[5]).abs().max()) <= bar("dtable", ref[5])


# ---------------------------------------------------------------------------------------------------- 6. CLS kernels

@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("kind", ["lengths", "rows", "full", "row0_dead"])
@pytest.mark.parametrize("S,dk", [(2, 64), (17, 40), (49, 64), (128, 64), (129, 64), (257, 80), (512, 64)])
def test_masked_cls_query_kernels(S, dk, kind, p_drop):
    """lstc_attn_cls_fwd_masked / _bwd_masked (both instantiations) read row 0 of the mask: against the f64 restatement with
    the output gradient on row 0 only; P and O equal row 0 of the full masked forward at the same seed (the tolerances of
    test_cls_query_kernels).  "row0_dead": the CLS row itself fully masked - uniform, finite, dQ = 0."""
    Fn = _Fn()
    N, H, dv, seed = 3, 2, dk, 61 + S
    q, k, v, do, table, index = sweep_inputs(N, S, H, dk, dv, S * 13 + dk, DEV)
    if kind == "row0_dead":
        mask, _ = make_mask("rows", N, H, S, seed)
        mask[1, 0, 0, :] = False
    else:
        mask, _ = make_mask(kind, N, H, S, seed)
    marg = Fn.attn_mask_arg(mask, N, H, S, device=DEV)
    qc = q.view(N, S, H * dk)[:, 0].contiguous()
    doc = do.view(N, S, H * dv)[:, 0].contiguous()
    oc, pc = Fn.attn_cls_fwd(qc, k, v, N, S, H, dk, dv, p_drop, seed, mask=marg)
    dqc, dk_, dv_ = Fn.attn_cls_bwd(doc, qc, k, v, pc, N, S, H, dk, dv, p_drop, seed, mask=marg)
    torch.cuda.synchronize()
    do0 = torch.zeros_like(do)
    do0.view(N, S, H * dv)[:, 0] = doc
    keep = _keep(N, H, S, p_drop, seed)
    ref = attn_reference_masked(q, k, v, do0, N, S, H, dk, dv, None, None, keep, p_drop, mask)     # row 0 carries no bias
    row0 = lambda t: t.view(N, S, -1)[:, 0]
    refs = (ref[0][:, :, 0], row0(ref[1]), row0(ref[2]), ref[3], ref[4])
    _check_exact((pc, oc, dqc, dk_, dv_), refs, ("cls", S, dk, kind, p_drop))
    kept0 = mask.to(DEV).expand(N, H, S, S)[:, :, 0]
    alive = kept0.any(-1, keepdim=True).expand(N, H, S)
    assert bool((pc[~kept0 & alive] == 0.0).all())
    if kind == "row0_dead":
        assert float((pc[1] - 1.0 / S).abs().max()) <= 2e-6 and bool((dqc[1] == 0).all())
    if S >= 2 and (S <= 128 or dk % 16 == 0):
        o_full, p_full = Fn.attn_fwd(q, k, v, N, S, H, dk, dv, table, index, p_drop, seed, mask=marg)
        torch.cuda.synchronize()
        assert float((p_full[:, :, 0] - pc).abs().max()) <= 2e-6
        assert float((row0(o_full) - oc).abs().max()) <= bar("O", refs[1])


# ---------------------------------------------------------------------------------------------------- 7. modules against the reference

def _encoder(case):
    from cases import fill_params
    from mask_cases import encoder_kw
    from lstc_vad_amd.models import Encoder
    enc = Encoder(**encoder_kw(case))
    fill_params(enc, case["seed"])
    return enc.to(DEV).train()


CASE_NAMES = ["mask_s49_pad", "mask_s49_rows", "mask_s145_pad", "mask_s145_rows"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_encoder_with_src_mask_matches_reference_fixture(name):
    """``Encoder.forward(x, src_mask, return_attn=True)`` in fp32 against the real reference: output and every layer's
    probabilities within 1e-4, the gradient of sum(out * w) with respect to every parameter and to the input within 2e-4 of its
    maximum; ``forward_cls(x, src_mask=...)`` equals ``forward(...)[:, 0]`` (5e-6, as test_forward_cls_equals_full_forward_row0_long)."""
    z, case = load_mask_case(name)
    enc = _encoder(case)
    x = torch.from_numpy(z["x"]).to(DEV).requires_grad_(True)
    mask = torch.from_numpy(z["mask"]).to(DEV)
    out, attns = enc(x, src_mask=mask, return_attn=True)
    assert len(attns) == 2
    (out * torch.from_numpy(z["w"]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    err = float((out.detach().cpu() - torch.from_numpy(z["out"])).abs().max())
    print(name, "out err %.3e" % err)
    assert err < 1e-4
    for i, a in enumerate(attns):
        e = float((a.cpu() - torch.from_numpy(z[f"attn.{i}"])).abs().max())
        print(name, "attn", i, "err %.3e" % e)
        assert e < 1e-4, (i, e)
    n = 0
    for kname, g in [("grad." + k, p.grad) for k, p in enc.named_parameters()] + [("grad_x", x.grad)]:
        ref = torch.from_numpy(z[kname])
        if g is None:                        # a parameter the run does not use (the input LayerNorm): the fixture holds zeros
            assert float(ref.abs().max()) == 0.0, kname
            continue
        tol = 2e-4 * float(ref.abs().max()) + 1e-7
        e = float((g.cpu() - ref).abs().max())
        print(name, kname, "err %.3e tol %.3e" % (e, tol))
        assert e < tol, (kname, e, tol)
        n += 1
    assert n >= 20
    enc.eval()
    with torch.no_grad():
        full = enc(x.detach(), src_mask=mask)
        cls = enc.forward_cls(x.detach(), src_mask=mask)
    assert cls.shape == (case["N"], 32)
    e = float((cls - full[:, 0]).abs().max())
    print(name, "forward_cls err %.3e" % e)
    assert e < 5e-6
    assert float((full.cpu() - torch.from_numpy(z["out"])).abs().max()) < 1e-4       # dropout 0: eval = train


def test_forward_cls_with_src_mask_backward_matches_full_forward():
    """Training through ``forward_cls(x, src_mask)``: the gradients of an objective on the CLS row equal those through
    ``forward(x, src_mask)[:, 0]`` within the golden step's gradient bar (2e-4 of each tensor's maximum)."""
    z, case = load_mask_case("mask_s49_rows")
    enc = _encoder(case)
    x = torch.from_numpy(z["x"]).to(DEV)
    mask = torch.from_numpy(z["mask"]).to(DEV)
    w = torch.from_numpy(z["w"]).to(DEV)[:, 0] * 49
    res = []
    for cls_only in (False, True):
        enc.zero_grad(set_to_none=True)
        y = enc.forward_cls(x, src_mask=mask) if cls_only else enc(x, src_mask=mask)[:, 0]
        (y * w).sum().backward()
        res.append({k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None})
    assert set(res[0]) == set(res[1])
    for k, g in res[0].items():
        tol = 2e-4 * float(g.abs().max()) + 1e-7
        assert float((res[1][k] - g).abs().max()) < tol, k


@pytest.mark.parametrize("name", ["mask_s49_pad", "mask_s145_pad", "mask_s145_rows"])
def test_encoder_with_src_mask_bf16_compute_close_to_fixture(name):
    """The same step in bf16 compute mode at the bars of test_bf16_compute_training_step_close_to_golden: the objective (a mean
    of O(1) terms, the size of a loss) within 2e-2, the direction of every large gradient tensor preserved (cosine > 0.9)."""
    Fn = _Fn()
    z, case = load_mask_case(name)
    enc = _encoder(case)
    x = torch.from_numpy(z["x"]).to(DEV)
    mask = torch.from_numpy(z["mask"]).to(DEV)
    Fn.set_compute_dtype("bf16")
    try:
        out = enc(x, src_mask=mask)
        obj = (out * torch.from_numpy(z["w"]).to(DEV)).sum()
        obj.backward()
        torch.cuda.synchronize()
    finally:
        Fn.set_compute_dtype("fp32")
    ref_obj = float((z["out"].astype(np.float64) * z["w"].astype(np.float64)).sum())
    assert torch.isfinite(out).all() and abs(float(obj.detach()) - ref_obj) < 2e-2, (float(obj.detach()), ref_obj)
    for k, p in enc.named_parameters():
        g = torch.from_numpy(z["grad." + k])
        if g.numel() > 64 and float(g.norm()) > 0:
            cos = float((p.grad.cpu() * g).sum() / (p.grad.cpu().norm() * g.norm() + 1e-20))
            assert cos > 0.9, (k, cos)


def test_bf16_mode_with_packed_products_takes_row_operands_under_a_mask():
    """bf16 mode with every product on the packed kernel (thresholds 0) and N * S a multiple of 256 - the shape where MHAFunction
    asks the attention core for packed operands: with a mask it asks for f32 rows (the masked kernels take nothing else), and
    forward and backward track the fp32 run at the bars of test_bf16_mode_packed_products_at_s145."""
    from lstc_vad_amd.models import Encoder
    Fn = _Fn()
    torch.manual_seed(0)
    enc = Encoder(n_layers=2, MHA_attn_dropout=0.0, MHA_fc_dropout=0.0, FFN_dropout=0.0, weight_init=True, n_head=2, d_k=128,
                  d_v=128, d_model=256, d_inner=512, MHA_layerNorm=True, FFN_layerNorm=True, relative_pe=True, window_size=4,
                  window_depth=3).to(DEV).train()
    N, S = 256, 49
    x = torch.randn(N, S - 1, 256, device=DEV)
    mask = (torch.arange(S)[None, :] < (S - torch.arange(N) % 20)[:, None]).view(N, 1, 1, S)
    res = {}
    for mode in ("fp32", "bf16"):
        Fn.set_compute_dtype(mode)
        if mode == "bf16":
            Fn.set_x3_threshold(0, 0, 0)
        try:
            if mode == "bf16":
                assert Fn.attn_fwd_pack(N, S, 2, 128)
            enc.zero_grad(set_to_none=True)
            y, attns = enc(x, src_mask=mask, return_attn=True)
            y.square().mean().backward()
            torch.cuda.synchronize()
        finally:
            Fn.set_compute_dtype("fp32")
            Fn.set_x3_threshold()
        for a in attns:
            assert bool((a[~mask.to(DEV).expand(N, 2, S, S)] == 0).all())
        res[mode] = (y.detach().clone(), {k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None})
    a, b = res["bf16"][0].double().flatten(), res["fp32"][0].double().flatten()
    assert torch.isfinite(a).all() and float(torch.dot(a, b) / (a.norm() * b.norm())) > 0.999
    for k, g in res["fp32"][1].items():
        h = res["bf16"][1][k]
        if g.numel() > 64 and float(g.norm()) > 0:
            assert torch.isfinite(h).all(), k
            assert float((h * g).sum() / (h.norm() * g.norm())) > 0.9, k


def test_multi_head_attention_mask_forms_and_return_values():
    """``MultiHeadAttention.forward(q, q, q, mask=...)``: return_attn and return_attn_v work with a mask, the probabilities carry
    it, an [S, S] mask broadcasts, and a PackedAct input with a mask raises."""
    from lstc_vad_amd.functional import PackedAct
    from lstc_vad_amd.models import MultiHeadAttention
    torch.manual_seed(0)
    mha = MultiHeadAttention(2, 32, 16, 16, layerNorm=True, attn_dropout=0.0, fc_dropout=0.0, relative_pe=True, window_size=4,
                             window_depth=3).to(DEV).eval()
    x = torch.randn(3, 49, 32, device=DEV)
    causal = torch.ones(49, 49).tril()
    with torch.no_grad():
        out, probs = mha(x, x, x, mask=causal, return_attn=True)
        out2, probs2, vv = mha(x, x, x, mask=causal.bool().view(1, 1, 49, 49), return_attn_v=True)
        assert mha(x, x, x, mask=causal)[1] is None
    assert probs.shape == (3, 2, 49, 49) and vv.shape == (3, 2, 49, 16)
    assert bool((probs[:, :, ~causal.bool().to(DEV)] == 0).all()) and float((probs.sum(-1) - 1).abs().max()) < 1e-6
    assert torch.equal(out, out2) and torch.equal(probs, probs2)
    xa = PackedAct(x.to(torch.bfloat16), (3, 49, 32))
    with pytest.raises(NotImplementedError):
        mha(xa, xa, xa, mask=causal)


# ---------------------------------------------------------------------------------------------------- 8. all-ones mask, mask dtypes

@pytest.mark.parametrize("S", [49, 128, 200])
def test_all_ones_mask_gives_the_unmasked_results(S):
    """Within the bars of the f64 reference of the unmasked problem (not bitwise below S = 128, where the unmasked call runs other
    kernels); above S = 128 the masked instantiation runs the same sums: bitwise."""
    N, H, d, p_drop, seed = 2, 2, 64, 0.2, 300 + S
    q, k, v, do, table, index = sweep_inputs(N, S, H, d, d, seed, DEV)
    ref = attn_reference(q, k, v, do, N, S, H, d, d, table, index, _keep(N, H, S, p_drop, seed), p_drop)
    plain = _run(q, k, v, do, N, S, H, d, d, table, index, p_drop, seed, None)
    for mask in (torch.ones(N, 1, 1, S), torch.ones(S, S, dtype=torch.bool)):
        got = _run(q, k, v, do, N, S, H, d, d, table, index, p_drop, seed, mask)
        _check_exact(got, ref, (S, "all ones", tuple(mask.shape)))
        if S > 128:
            for name, a, b in zip(NAMES, got, plain):
                assert torch.equal(a, b), name


@pytest.mark.parametrize("S", [49, 145])
def test_mask_dtypes_give_bitwise_equal_results(S):
    N, H, d, p_drop, seed = 2, 2, 64, 0.2, 500 + S
    q, k, v, do, table, index = sweep_inputs(N, S, H, d, d, seed, DEV)
    mask, _ = make_mask("rows", N, H, S, seed)
    forms = (mask, mask.to(torch.uint8), torch.where(mask, torch.full(mask.shape, -2.5), torch.zeros(mask.shape)),
             mask.to(torch.int64) * 7, mask.expand(N, H, S, S))
    runs = [_run(q, k, v, do, N, S, H, d, d, table, index, p_drop, seed, m) for m in forms]
    for r in runs[1:]:
        for name, a, b in zip(NAMES, r, runs[0]):
            assert torch.equal(a, b), name
