"""Attention kernels from S = 97 to 512 (the first-generation T = 4 kernels of csrc/attention.hip up to S = 128, the key-tiled
kernels of csrc/attention_long.hip above, the CLS-query kernels at every S) against a float64 restatement of the contract
(include/lstc_hip.h, "attention"; tests/util.py attn_reference, on the device).

Bars, exact-f32 products: P within 2e-6; O, dQ, dK, dV and the table gradient within 2e-5 * max|ref| + 1e-6 (the short path's
bars, tests/test_hip_parity.py).  Every sweep case also checks that the bar can see one lost key: the f64 O without key S - 1
differs from the true O by more than 4x the bar.  bf16 products (LSTC_BF16, S > 128): relative Frobenius error of O and every
gradient above 10x the exact run's (the bf16 path ran) and below 8e-3 (bf16 operand rounding level); P within 4e-6 of the f64
softmax of the logits of the RNE-rounded operands the kernel contracts (K and Q * scale, csrc/attention_long.hip tile_xt).

Inputs use the models' own index (relative_position_index_3d(ceil((S-1)/16), 4): sliced whenever S - 1 < 16 L), a table
scaled by 0.4 and attention dropout 0.2; N * H stays small except in the one case that needs N * H > 4096."""
import pytest
import torch

from util import attn_layout as _layout, attn_reference, attn_rounded_probs

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("P", "O", "dQ", "dK", "dV", "dtable")


def _Fn():
    from lstc_vad_amd import functional as Fn
    return Fn


def _index(S):
    """The models' index for S tokens at 16 patches and its table row count."""
    from lstc_vad_amd.models.MultiHeadAttention import relative_position_index_3d
    L = max(1, -(-(S - 1) // 16))
    return relative_position_index_3d(L, 4).to(DEV), (2 * L - 1) * 49


def _inputs(N, S, H, dk, dv, seed, bias=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    q, k = (torch.randn(N * S, H * dk, device=DEV, generator=g) for _ in range(2))
    v, do = (torch.randn(N * S, H * dv, device=DEV, generator=g) for _ in range(2))
    table = index = None
    if bias:
        index, rows = _index(S)
        table = 0.4 * torch.randn(rows, H, device=DEV, generator=g)
    return q, k, v, do, table, index


def _run(q, k, v, do, N, S, H, dk, dv, table, index, p_drop, seed, mode="fp32", out=None):
    """Forward and backward through functional.attn_fwd / attn_bwd; dQ / dK / dV land in ``out`` (views with the row strides of
    Q / K / V) or in fresh tensors of those strides.  Returns (P, O, dQ, dK, dV, dtable)."""
    Fn = _Fn()
    prev = Fn.get_compute_dtype()
    Fn.set_compute_dtype(mode)
    try:
        o, probs = Fn.attn_fwd(q, k, v, N, S, H, dk, dv, table, index, p_drop, seed)
        if out is None:
            out = tuple(torch.empty_strided(t.shape, t.stride(), device=DEV) for t in (q, k, v))
        dq, dk_, dv_, dtab = Fn.attn_bwd(do, q, k, v, probs, N, S, H, dk, dv, table, index, p_drop, seed, out=out)
        torch.cuda.synchronize()
    finally:
        Fn.set_compute_dtype(prev)
    return probs, o, dq, dk_, dv_, dtab


def _keep(N, H, S, p_drop, seed):
    return _Fn().dropout_mask((N, H, S, S), p_drop, seed, DEV) if p_drop > 0 else None


def _bar(name, ref):
    return 2e-6 if name == "P" else 2e-5 * float(ref.abs().max()) + 1e-6


def _check_exact(got, ref, what):
    errs = {}
    for name, a, b in zip(NAMES, got, ref):
        if b is None:
            assert a is None, (what, name)
            continue
        a = a.double()
        assert torch.isfinite(a).all(), (what, name)
        errs[name] = (float((a - b).abs().max()), _bar(name, b))
    bad = {n: e for n, e in errs.items() if e[0] > e[1]}
    assert not bad, (what, "max |err| > bar", bad)


def _check_sensitive(q, k, v, N, S, H, dk, dv, table, index, keep, p_drop, ref_o):
    """The O bar sees a lost key: f64 O without key S - 1 is more than 4 bars away from the true O."""
    o_cut = attn_reference(q, k, v, None, N, S, H, dk, dv, table, index, keep, p_drop, cut_key=S - 1)[1]
    gap = float((o_cut - ref_o).abs().max())
    assert gap > 4 * _bar("O", ref_o), (gap, _bar("O", ref_o))


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


# ---------------------------------------------------------------------------------------------------- 1. sequence lengths

SWEEP_S = [97, 113, 127, 128, 129, 130, 159, 160, 161, 192, 193, 224, 255, 256, 257, 288, 320, 383, 384, 416, 449, 480, 497,
           511, 512]


@pytest.mark.parametrize("S,H", [(S, 1) for S in SWEEP_S] + [(129, 2), (257, 2), (512, 2)])
def test_sequence_length_sweep_fp32(S, H):
    """Both sides of the short / long boundary and every 32-row block edge, d_k = d_v = 64, N = 3: 3 ceil(S / 32) query blocks
    are rarely a multiple of the forward's 4 waves per workgroup, so its last workgroup has idle waves."""
    N, d, p_drop, seed = 3, 64, 0.2, 101 + S
    q, k, v, do, table, index = _inputs(N, S, H, d, d, seed=S * 7 + H)
    got = _run(q, k, v, do, N, S, H, d, d, table, index, p_drop, seed)
    keep = _keep(N, H, S, p_drop, seed)
    ref = attn_reference(q, k, v, do, N, S, H, d, d, table, index, keep, p_drop)
    _check_exact(got, ref, (S, H))
    _check_sensitive(q, k, v, N, S, H, d, d, table, index, keep, p_drop, ref[1])


# ---------------------------------------------------------------------------------------------------- 2. head widths

WIDTHS = [(16, 16), (48, 48), (64, 64), (80, 80), (96, 96), (128, 128), (144, 144), (256, 256), (320, 320), (512, 512),
          (64, 128), (128, 64), (32, 256), (256, 32), (16, 272)]


@pytest.mark.parametrize("S,dk,dv", [(S, dk, dv) for S in (113, 145, 449) for dk, dv in WIDTHS] +
                         [(113, 8, 8), (113, 24, 24), (113, 40, 40)])
def test_head_width_matrix(S, dk, dv):
    """Every 32-column group count of the long kernels (DT = 1, 2, 4, 8 and a second 256-column group past d = 256),
    d = 16 mod 32 (the second lane half of a 32-wide k step loads nothing), d_k != d_v both ways.  S = 113 runs the
    first-generation T = 4 kernels, whose loops are bounded by d_k and d_v (any width); above S = 128 also the bf16 form."""
    N = H = 2
    p_drop, seed = 0.2, 7 * S + dk
    q, k, v, do, table, index = _inputs(N, S, H, dk, dv, seed=1000 * S + 10 * dk + dv)
    keep = _keep(N, H, S, p_drop, seed)
    ref = attn_reference(q, k, v, do, N, S, H, dk, dv, table, index, keep, p_drop)
    exact = _run(q, k, v, do, N, S, H, dk, dv, table, index, p_drop, seed)
    _check_exact(exact, ref, (S, dk, dv))
    _check_sensitive(q, k, v, N, S, H, dk, dv, table, index, keep, p_drop, ref[1])
    if S <= 128:
        return
    got = _run(q, k, v, do, N, S, H, dk, dv, table, index, p_drop, seed, mode="bf16")
    p_rounded = attn_rounded_probs(q, k, N, S, H, dk, table, index)
    err_p = float((got[0].double() - p_rounded).abs().max())
    assert err_p < 4e-6, ("P vs softmax of the rounded operands", err_p)
    for name, a, e, r in zip(NAMES[1:], got[1:], exact[1:], ref[1:]):
        err, err_exact = _rel(a, r), _rel(e, r)
        assert err_exact < 1e-5 and 10 * err_exact < err < 8e-3, (name, err, err_exact)


# ---------------------------------------------------------------------------------------------------- 3. strides, alignment

@pytest.mark.parametrize("kind", ["odd_ld", "offset", "strides"])
@pytest.mark.parametrize("d", [64, 80])
@pytest.mark.parametrize("S", [113, 200, 512])
def test_unaligned_and_strided_operands(S, d, kind):
    """Row strides or bases that are not 16-B aligned take the scalar operand loads (lload16 / load16 without float4).  Above
    S = 128 the same MFMA order runs on both load widths: bitwise equal to the call on contiguous aligned copies.  At S = 113
    both runs against f64 at the bars."""
    N, H, p_drop, seed = 2, 2, 0.2, 31 * S + d
    q, k, v, do, table, index = _inputs(N, S, H, d, d, seed=S + 3 * d)
    ql, kl, vl, dol = _layout(kind, (q, k, v, do))
    assert (ql.stride(0) % 4 or ql.data_ptr() % 16) and (dol.stride(0) % 4 or dol.data_ptr() % 16)
    out = _layout(kind, tuple(torch.zeros_like(t) for t in (q, k, v, do)))[:3]
    got = _run(ql, kl, vl, dol, N, S, H, d, d, table, index, p_drop, seed, out=out)
    ref_run = _run(q, k, v, do, N, S, H, d, d, table, index, p_drop, seed)
    if S > 128:
        for name, a, b in zip(NAMES, got, ref_run):
            assert torch.equal(a, b), (name, float((a - b).abs().max()))
    else:
        keep = _keep(N, H, S, p_drop, seed)
        ref = attn_reference(q, k, v, do, N, S, H, d, d, table, index, keep, p_drop)
        _check_exact(got, ref, (S, d, kind))
        _check_exact(ref_run, ref, (S, d, "contiguous"))


# ---------------------------------------------------------------------------------------------------- 4. backward chunks

def _chunked_bwd(monkeypatch, npw, q, k, v, do, probs, N, S, H, dk, dv, table, index, p_drop, seed):
    """attn_bwd with ``npw`` sequences per workgroup asked for (0: functional's own choice); returns its results and the
    number of partial tables (= workgroups per head) it summed."""
    Fn = _Fn()
    seen = []
    colsum = Fn.colsum

    def spy(parts, *a, **kw):
        seen.append(parts.shape[0])
        return colsum(parts, *a, **kw)
    monkeypatch.setattr(Fn, "colsum", spy)
    monkeypatch.setattr(Fn, "_BWD_NPW", npw)
    try:
        r = Fn.attn_bwd(do, q, k, v, probs, N, S, H, dk, dv, table, index, p_drop, seed)
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
    assert len(seen) == 1
    return r, seen[0]


@pytest.mark.parametrize("S,d,npw", [(145, 64, 2), (145, 64, 3), (145, 64, 5), (257, 64, 2), (257, 64, 3), (257, 64, 5),
                                     (145, 128, 3), (257, 256, 3)])
def test_backward_workgroups_with_several_sequences(S, d, npw, monkeypatch):
    """N = 7 sequences in chunks of npw (uneven last chunk): the rowsum image Dr is reused across a workgroup's sequences and
    the per-wave bias tables sum over all of them.  dQ / dK / dV have one writer per element and a chunking-independent sum
    order: bitwise equal to the one-sequence-per-workgroup run, and two runs bitwise equal (d = 128: DT = 4, d = 256: DT = 8).
    The summed table gradient against f64."""
    N, H, p_drop, seed = 7, 2, 0.2, 5 * S + npw
    q, k, v, do, table, index = _inputs(N, S, H, d, d, seed=S + npw + d)
    _, probs = _Fn().attn_fwd(q, k, v, N, S, H, d, d, table, index, p_drop, seed)
    args = (q, k, v, do, probs, N, S, H, d, d, table, index, p_drop, seed)
    one, c1 = _chunked_bwd(monkeypatch, 1, *args)
    got, c = _chunked_bwd(monkeypatch, npw, *args)
    again, _ = _chunked_bwd(monkeypatch, npw, *args)
    per = -(-N // -(-N // npw))
    assert c1 == N and c == -(-N // per) and per >= 2 and N % per != 0, (c1, c, per)
    for name, a, b, b2 in zip(("dQ", "dK", "dV"), got[:3], one[:3], again[:3]):
        assert torch.equal(a, b), (name, "npw", npw, float((a - b).abs().max()))
        assert torch.equal(a, b2), (name, "run to run")
    assert torch.equal(got[3], again[3])
    ref = attn_reference(q, k, v, do, N, S, H, d, d, table, index, _keep(N, H, S, p_drop, seed), p_drop)
    for name, a, b in (("dtable", got[3], ref[5]), ("dtable npw=1", one[3], ref[5])):
        err = float((a.double() - b).abs().max())
        assert err <= _bar(name, b), (name, err, _bar(name, b))


def test_backward_picks_several_sequences_per_workgroup_at_large_n(monkeypatch):
    """N * H > 4096: functional.attn_bwd chooses 2 sequences per workgroup by itself (1050 partial tables)."""
    N, S, H, d, p_drop, seed = 2100, 129, 2, 16, 0.2, 404
    q, k, v, do, table, index = _inputs(N, S, H, d, d, seed=9)
    _, probs = _Fn().attn_fwd(q, k, v, N, S, H, d, d, table, index, p_drop, seed)
    args = (q, k, v, do, probs, N, S, H, d, d, table, index, p_drop, seed)
    got, chunks = _chunked_bwd(monkeypatch, 0, *args)
    assert chunks == 1050
    one, _ = _chunked_bwd(monkeypatch, 1, *args)
    for name, a, b in zip(("dQ", "dK", "dV"), got[:3], one[:3]):
        assert torch.equal(a, b), name
    ref = attn_reference(q, k, v, do, N, S, H, d, d, table, index, _keep(N, H, S, p_drop, seed), p_drop)
    err = float((got[3].double() - ref[5]).abs().max())
    assert err <= _bar("dtable", ref[5]), (err, _bar("dtable", ref[5]))


# ---------------------------------------------------------------------------------------------------- 5. CLS-query kernels

@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("dk", [16, 40, 64, 256, 320])
@pytest.mark.parametrize("S", [1, 2, 17, 113, 128, 129, 200, 257, 512])
def test_cls_query_kernels(S, dk, p_drop):
    """lstc_attn_cls_fwd / _bwd (both instantiations: S <= 128 and S <= 512) against the f64 row-0 restatement: row 0 carries no
    bias, its mask is row 0 of dropout_mask((N, H, S, S)).  Where the full kernels take the shape (S >= 2; above S = 128 d_k a
    multiple of 16), P and O also agree with row 0 of the full forward at the same seed: the shared dropout index."""
    Fn = _Fn()
    N, H, dv, seed = 3, 2, dk, 59 + S
    g = torch.Generator(device=DEV).manual_seed(S * 11 + dk)
    q = torch.randn(N * S, H * dk, device=DEV, generator=g)
    k = torch.randn(N * S, H * dk, device=DEV, generator=g)
    v = torch.randn(N * S, H * dv, device=DEV, generator=g)
    doc = torch.randn(N, H * dv, device=DEV, generator=g)
    qc = q.view(N, S, H * dk)[:, 0].contiguous()
    oc, pc = Fn.attn_cls_fwd(qc, k, v, N, S, H, dk, dv, p_drop, seed)
    dqc, dk_, dv_ = Fn.attn_cls_bwd(doc, qc, k, v, pc, N, S, H, dk, dv, p_drop, seed)
    torch.cuda.synchronize()

    keep = _keep(N, H, S, p_drop, seed)
    qd = qc.double().view(N, H, 1, dk).requires_grad_(True)
    kd, vd = (t.double().view(N, S, H, -1).transpose(1, 2).requires_grad_(True) for t in (k, v))
    pr = torch.softmax(torch.matmul(qd * (1.0 / dk ** 0.5), kd.transpose(-1, -2)), -1)          # [N, H, 1, S]
    pdr = pr * keep[:, :, :1].double() / (1.0 - p_drop) if p_drop > 0 else pr
    o = torch.matmul(pdr, vd)                                                                     # [N, H, 1, dv]
    o.backward(doc.double().view(N, H, 1, dv))
    ref = {"P": pr.detach().view(N, H, S), "O": o.detach().view(N, H * dv), "dQ": qd.grad.view(N, H * dk),
           "dK": kd.grad.transpose(1, 2).reshape(N * S, H * dk), "dV": vd.grad.transpose(1, 2).reshape(N * S, H * dv)}
    _check_exact([pc, oc, dqc, dk_, dv_], [ref[n] for n in ("P", "O", "dQ", "dK", "dV")] , ("cls", S, dk, p_drop))
    if S >= 2 and (S <= 128 or dk % 16 == 0):
        index, rows = _index(S)
        table = 0.4 * torch.randn(rows, H, device=DEV, generator=g)
        o_full, p_full = Fn.attn_fwd(q, k, v, N, S, H, dk, dv, table, index, p_drop, seed)
        torch.cuda.synchronize()
        assert float((p_full[:, :, 0] - pc).abs().max()) <= 2e-6
        o0 = o_full.view(N, S, H * dv)[:, 0]
        assert float((o0 - oc).abs().max()) <= _bar("O", ref["O"])
