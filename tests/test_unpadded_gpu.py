"""Unpadded batches on the GPU: attention over sequence offsets, the unpadded CLS concat, the three CLS passes over an unpadded X,
``Encoder.forward_unpadded`` / ``forward_cls_unpadded`` and ``ragged="unpadded"`` scoring.

Kernel level, against the float64 references of tests/util_unpadded.py (checked on the CPU by tests/test_unpadded_host.py): the
attention and the CLS passes under util_mask.bar, the concat under util_rowops.tol.  Model level, against the oracle run on every
sequence ALONE (oracle.lstc_oracle, float32 on the CPU): outputs within 1e-4 absolute, parameter and input gradients within
2e-4 * max|g| + 1e-7 per tensor (tests/test_hip_parity.py:94), with the padded ``lengths=`` path as the control arm at the same bar.
The length set (util_unpadded.LENGTHS) crosses every 32-token tile edge of S = 2 .. 128 in one unsorted batch."""
import pytest
import torch

import util_ragged as R
import util_unpadded as U
from util import _LibSpy
from util_mask import bar, model_index
from util_rowops import tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
LENS = U.LENGTHS
GUARD = 7.0


def _Fn():
    from lstc_vad_amd import functional as Fn
    return Fn


def _lib():
    from lstc_vad_amd import _lib
    return _lib


def _bitwise_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _block(data, ld, fill):
    """``data`` [M, c] inside a [M + 4, ld] buffer of ``fill``: two guard rows in front, two behind, ld - c guard columns.
    Returns (buffer, the [M, ld] block, its [M, c] data view)."""
    M, c = data.shape
    buf = torch.full((M + 4, ld), fill, device=DEV, dtype=F32)
    buf[2:2 + M, :c] = data.to(DEV)
    return buf, buf[2:2 + M], buf[2:2 + M, :c]


def _guards_intact(buf, M, c):
    return bool((buf[:2] == GUARD).all() and (buf[2 + M:] == GUARD).all() and (buf[2:2 + M, c:] == GUARD).all())


# ---------------------------------------------------------------------------------------------------- attention over offsets
WIDTHS = [(16, 16), (40, 24), (64, 64)]
H = 2

_attn_in = {}


def _attn_inputs(dk, dv, lens=LENS):
    """CPU inputs of the attention tests, built once per (widths, lengths) and never modified."""
    key = (dk, dv, tuple(lens))
    if key not in _attn_in:
        g = torch.Generator().manual_seed(1000 + dk + dv)
        M = sum(lens) + len(lens)
        q, k = (torch.randn(M, H * dk, generator=g) for _ in range(2))
        v, do = (torch.randn(M, H * dv, generator=g) for _ in range(2))
        index, rows = model_index(128, "cpu")
        table = 0.4 * torch.randn(rows, H, generator=g)
        _attn_in[key] = (q, k, v, do, table, index)
    return _attn_in[key]


def _run_attn(lens, dk, dv, q, k, v, do, table, index, p_drop, seed, pad=None, buckets=False):
    """Forward and backward through functional.attn_var_fwd / _bwd with every operand inside guarded, wider blocks.  ``pad``: extra
    columns of the row pitch (default: 3 for the unaligned widths - a misaligned pitch - and 4 otherwise).  ``buckets``: one launch
    per tile count over a device list of its sequences (functional._ATTN_VAR_BUCKETS) instead of one launch for all."""
    Fn = _Fn()
    lay = Fn.unpadded_layout(lens)
    was, Fn._ATTN_VAR_BUCKETS = Fn._ATTN_VAR_BUCKETS, buckets
    try:
        return _run_attn_now(Fn, lay, dk, dv, q, k, v, do, table, index, p_drop, seed, pad)
    finally:
        Fn._ATTN_VAR_BUCKETS = was


def _run_attn_now(Fn, lay, dk, dv, q, k, v, do, table, index, p_drop, seed, pad):
    M, npr = lay.M, lay.n_probs(H)
    pad = (4 if dk % 4 == 0 and dv % 4 == 0 and dk != 40 else 3) if pad is None else pad
    nan = float("nan")
    ins = [_block(t, t.shape[1] + pad, nan)[1] for t in (q, k, v, do)]
    qb, kb, vb, dob = ins
    o_buf, o_blk, _ = _block(torch.full((M, H * dv), GUARD), H * dv + pad, GUARD)
    gbufs = [_block(torch.full((M, w), GUARD), w + pad, GUARD) for w in (H * dk, H * dk, H * dv)]
    pbuf = torch.full((npr + 64,), GUARD, device=DEV)
    probs = pbuf[32:32 + npr]
    tb, ix = table.to(DEV), index.to(DEV)
    Fn.attn_var_fwd(qb, kb, vb, lay, H, dk, dv, tb, ix, p_drop, seed, out=o_blk, probs=probs)
    _, _, _, dtable = Fn.attn_var_bwd(dob, qb, kb, vb, probs, lay, H, dk, dv, tb, ix, p_drop, seed, out=tuple(b[1] for b in gbufs))
    torch.cuda.synchronize()
    assert _guards_intact(o_buf, M, H * dv) and all(_guards_intact(b[0], M, w) for b, w in zip(gbufs, (H * dk, H * dk, H * dv)))
    assert bool((pbuf[:32] == GUARD).all() and (pbuf[32 + npr:] == GUARD).all())
    got = {"P": probs.clone(), "O": o_blk[:, :H * dv].clone(), "dQ": gbufs[0][2].clone(), "dK": gbufs[1][2].clone(),
           "dV": gbufs[2][2].clone(), "dtable": dtable}
    return lay, got


@pytest.mark.parametrize("buckets", [False, True])
@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("dk,dv", WIDTHS)
def test_attention_over_offsets_against_f64(dk, dv, p_drop, buckets):
    """P, O, dQ, dK, dV, dtable within util_mask.bar of the float64 reference on every sequence alone; inputs between NaN rows and
    beside NaN columns, outputs between guards that survive; the keep mask replayed with lstc_dropout_mask over the ragged
    buffer; every probability row sums to 1.  One launch for the whole batch, and one per tile count over sequence-id lists."""
    Fn = _Fn()
    q, k, v, do, table, index = _attn_inputs(dk, dv)
    seed = 4242 + dk
    lay, got = _run_attn(LENS, dk, dv, q, k, v, do, table, index, p_drop, seed, buckets=buckets)
    keep = Fn.dropout_mask((lay.n_probs(H),), p_drop, seed, DEV).cpu() if p_drop > 0 else None
    ref = dict(zip(("P", "O", "dQ", "dK", "dV", "dtable"), U.attn_var_reference(q, k, v, do, LENS, H, dk, dv, table, index, keep, p_drop)))
    errs = {}
    for name, r in ref.items():
        assert torch.isfinite(got[name]).all(), name
        errs[name] = (float((got[name].cpu().double() - r).abs().max()), bar(name, r))
    print(dk, dv, p_drop, {n: "%.3e / %.3e" % e for n, e in errs.items()})
    assert all(e <= b for e, b in errs.values()), errs
    prob0 = lay.prob0(H)
    for n, S in enumerate(lay.S):
        rows = got["P"][prob0[n]:prob0[n + 1]].view(H * S, S).sum(-1)
        assert float((rows - 1).abs().max()) < 1e-5, n


def test_a_sequence_does_not_depend_on_its_neighbours():
    """Each sequence of the mixed batch run alone (N = 1), and the batch permuted, give the batch's bits for P, O, dQ, dK, dV; two
    runs of the same batch are equal, the bias-table gradient included; and the bucketing changes no bit of P, O, dQ, dK, dV,
    with dropout on as well (a sequence alone runs in its own tile count, the batch's single launch in the longest one's)."""
    dk, dv = 40, 24
    q, k, v, do, table, index = _attn_inputs(dk, dv)
    lay, got = _run_attn(LENS, dk, dv, q, k, v, do, table, index, 0.0, 0)
    _, again = _run_attn(LENS, dk, dv, q, k, v, do, table, index, 0.0, 0)
    for name in got:
        assert torch.equal(got[name], again[name]), name
    for p_drop in (0.0, 0.25):
        _, one = _run_attn(LENS, dk, dv, q, k, v, do, table, index, p_drop, 5)
        _, per_t = _run_attn(LENS, dk, dv, q, k, v, do, table, index, p_drop, 5, buckets=True)
        for name in ("P", "O", "dQ", "dK", "dV"):
            assert torch.equal(one[name], per_t[name]), (p_drop, name)
        assert float((one["dtable"] - per_t["dtable"]).abs().max()) <= bar("dtable", one["dtable"].double())      # another chunking
    prob0 = lay.prob0(H)
    rows = lambda t, n: t[lay.row0[n]:lay.row0[n + 1]]
    for n, L in enumerate(LENS):
        _, one = _run_attn([L], dk, dv, *(rows(t, n) for t in (q, k, v, do)), table, index, 0.0, 0)
        assert torch.equal(one["P"], got["P"][prob0[n]:prob0[n + 1]]), n
        for name in ("O", "dQ", "dK", "dV"):
            assert torch.equal(one[name], rows(got[name], n)), (n, name)
    perm = [7, 2, 9, 0, 5, 3, 8, 1, 6, 4]
    pl = [LENS[i] for i in perm]
    play, pgot = _run_attn(pl, dk, dv, *(torch.cat([rows(t, i) for i in perm], 0) for t in (q, k, v, do)), table, index, 0.0, 0)
    pp0 = play.prob0(H)
    for j, i in enumerate(perm):
        assert torch.equal(pgot["P"][pp0[j]:pp0[j + 1]], got["P"][prob0[i]:prob0[i + 1]]), i
        for name in ("O", "dQ", "dK", "dV"):
            assert torch.equal(pgot[name][play.row0[j]:play.row0[j + 1]], rows(got[name], i)), (i, name)


@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("L", [48, 127])
def test_equal_lengths_are_the_first_generation_kernels_bit_for_bit(L, p_drop, monkeypatch):
    """The offset kernels are instantiations of the first-generation ones (attn_fwd_kernel / attn_bwd_kernel<T, false, VAR = true>),
    so at equal lengths P, O, dQ, dK, dV are torch.equal - not merely within bar - to lstc_attn_fwd / _bwd with variant = 1 on the
    [N, S, ...] view, dropout included (the ragged offset of an element is its flat index there).  The bias-table gradient is summed
    over a different chunking of the sequences: within bar."""
    Fn = _Fn()
    N, S, dk, dv = 3, L + 1, 16, 16
    lens = [L] * N
    q, k, v, do, table, index = _attn_inputs(dk, dv, lens)
    _, got = _run_attn(lens, dk, dv, q, k, v, do, table, index, p_drop, 99, pad=0)
    monkeypatch.setattr(Fn, "_ATTN_VARIANT", 1)
    qd, kd, vd, dod, tb, ix = (t.to(DEV) for t in (q, k, v, do, table, index))
    o, probs = Fn.attn_fwd(qd, kd, vd, N, S, H, dk, dv, tb, ix, p_drop, 99)
    dq, dk_, dv_, dtable = Fn.attn_bwd(dod, qd, kd, vd, probs, N, S, H, dk, dv, tb, ix, p_drop, 99)
    torch.cuda.synchronize()
    assert torch.equal(got["P"], probs.reshape(-1))
    for name, ref in (("O", o), ("dQ", dq), ("dK", dk_), ("dV", dv_)):
        assert torch.equal(got[name], ref), name
    assert float((got["dtable"] - dtable).abs().max()) <= bar("dtable", dtable.double())


def test_attention_entry_points_check_before_any_launch():
    """The refusals of lstc_attn_var_fwd / _bwd by return code (include/lstc_hip.h: LSTC_E_NULL -1, _SHAPE -2, _UNSUPPORTED -4,
    _RANGE -5); a correct call on the same descriptor returns 0."""
    import ctypes as C
    L = _lib()
    lib = L.load()
    t = torch.zeros(64, device=DEV)
    d = L.AttnDesc()
    d.N, d.S, d.H, d.dk, d.dv, d.ldq, d.ldk, d.ldv, d.ldo = 1, 4, 1, 4, 4, 4, 4, 4, 4
    d.scale = 0.5
    d.Q = d.K = d.V = d.O = d.probs = d.dO = d.dQ = d.dK = d.dV = t.data_ptr()
    i32 = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    i64 = torch.tensor([0, 16], dtype=torch.int64, device=DEV)

    def seqs(**kw):
        return L.Seqs(**{**dict(row0=i32.data_ptr(), prob0=i64.data_ptr(), seq_ids=None, n_ids=1, n_probs=16), **kw})
    st = L.stream_ptr()
    for fn in (lib.lstc_attn_var_fwd, lib.lstc_attn_var_bwd):
        assert fn(None, C.byref(seqs()), st) == -1 and fn(C.byref(d), None, st) == -1
        assert fn(C.byref(d), C.byref(seqs(row0=None)), st) == -1 and fn(C.byref(d), C.byref(seqs(prob0=None)), st) == -1
        assert fn(C.byref(d), C.byref(seqs(n_probs=2 ** 32)), st) == -5
        assert fn(C.byref(d), C.byref(seqs(n_ids=0)), st) == -2
        d.S = 129
        assert fn(C.byref(d), C.byref(seqs()), st) == -5
        d.S = 4
        d.O_pack = t.data_ptr()
        assert fn(C.byref(d), C.byref(seqs()), st) == -4
        d.O_pack = None
        d.in_pack_cols = 64
        assert fn(C.byref(d), C.byref(seqs()), st) == -4
        d.in_pack_cols = 0
        d.Q = None
        assert fn(C.byref(d), C.byref(seqs()), st) == -1
        d.Q = t.data_ptr()
    tab = torch.zeros(8, device=DEV)
    idx = torch.zeros(9, dtype=torch.int64, device=DEV)
    d.index_ld, d.table_rows, d.table, d.index, d.dtable, d.dtable_chunks = 3, 8, tab.data_ptr(), idx.data_ptr(), tab.data_ptr(), 0
    assert lib.lstc_attn_var_bwd(C.byref(d), C.byref(seqs()), st) == -4          # no atomics: partial tables only
    d.dtable_chunks = 1
    assert lib.lstc_attn_var_fwd(C.byref(d), C.byref(seqs()), st) == 0 and lib.lstc_attn_var_bwd(C.byref(d), C.byref(seqs()), st) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- CLS concat
def _concat_fwd(x, row0, cls, pos, M):
    L = _lib()
    d = x.shape[1]
    y = torch.full((M, d), float("nan"), device=DEV)
    L.check(L.load().lstc_cls_concat_var_fwd(L.dev_ptr(x), L.dev_ptr(row0), L.dev_ptr(cls), L.dev_ptr(pos), L.dev_ptr(y), row0.numel() - 1, d,
                                             L.stream_ptr()), "lstc_cls_concat_var_fwd")
    return y


def _concat_bwd(dy, row0, rows_in, S_max, mean_cls):
    L = _lib()
    d = dy.shape[1]
    dx = torch.full((rows_in, d), float("nan"), device=DEV)
    dtok = torch.full((S_max, d), float("nan"), device=DEV)
    L.check(L.load().lstc_cls_concat_var_bwd(L.dev_ptr(dy), L.dev_ptr(row0), L.dev_ptr(dx), L.dev_ptr(dtok), row0.numel() - 1, S_max, d,
                                             int(mean_cls), L.stream_ptr()), "lstc_cls_concat_var_bwd")
    return dx, dtok


def _misaligned(t):
    """A copy of ``t`` 4 bytes off a 16-byte boundary: the entry points then take their 4-byte path."""
    buf = torch.empty(t.numel() + 4, device=t.device, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    assert v.data_ptr() % 16 == 4
    v.copy_(t)
    return v


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("learned", [False, True])
@pytest.mark.parametrize("d,lens", [(36, LENS), (30, LENS), (2048, LENS), (36, [5]), (30, [127])])
def test_cls_concat_var_kernels_against_f64(d, lens, learned, with_pos):
    """lstc_cls_concat_var_fwd / _bwd: d = 36 the 16-byte path, d = 30 the 4-byte path, d = 2048 several workgroups per row; the mixed
    set and batches of one sequence; the 4-byte path gives the 16-byte path's bits."""
    in0, row0, _ = U.offsets(lens, 1)
    S_max = max(lens) + 1
    g = torch.Generator().manual_seed(200 + d + 2 * learned + with_pos + len(lens))
    x = torch.randn(in0[-1], d, generator=g) + 0.5
    cls = torch.randn(d, generator=g) if learned else None
    pos = torch.randn(S_max, d, generator=g) if with_pos else None
    dy = torch.randn(row0[-1], d, generator=g)
    r0 = torch.tensor(row0, dtype=torch.int32, device=DEV)
    dev = lambda t: None if t is None else t.to(DEV)
    y = _concat_fwd(dev(x), r0, dev(cls), dev(pos), row0[-1])
    dx, dtok = _concat_bwd(dev(dy), r0, in0[-1], S_max, not learned)
    torch.cuda.synchronize()
    ref = U.concat_var_fwd(x, lens, cls, pos)
    t_y = tol(ref, U.concat_var_fwd(x, lens, cls, pos, dtype=F32), U.concat_var_terms(x, lens, cls, pos))
    rdx, rtok = U.concat_var_bwd(dy, lens, not learned)
    fdx, ftok = U.concat_var_bwd(dy, lens, not learned, dtype=F32)
    adx, atok = U.concat_var_bwd_terms(dy, lens, not learned)
    errs = {"y": (float((y.cpu().double() - ref).abs().max()), t_y),
            "dx": (float((dx.cpu().double() - rdx).abs().max()), tol(rdx, fdx, adx)),
            "dtok": (float((dtok.cpu().double() - rtok).abs().max()), tol(rtok, ftok, atok))}
    print(d, len(lens), learned, with_pos, {k: "%.3e / %.3e" % v for k, v in errs.items()})
    for t in (y, dx, dtok):
        assert torch.isfinite(t).all()
    assert all(e <= t for e, t in errs.values()), errs
    if d % 4 == 0:
        y4 = _concat_fwd(_misaligned(dev(x)), r0, dev(cls), dev(pos), row0[-1])
        dx4, dtok4 = _concat_bwd(_misaligned(dev(dy)), r0, in0[-1], S_max, not learned)
        torch.cuda.synchronize()
        assert torch.equal(y4, y) and torch.equal(dx4, dx) and torch.equal(dtok4, dtok)


# ---------------------------------------------------------------------------------------------------- the three CLS passes
CLS_LENS = {2: [1, 1, 1], 49: [48, 1, 16, 33], 128: [127, 1, 63, 64]}


@pytest.mark.parametrize("S_max", [2, 49, 128])
@pytest.mark.parametrize("d", [32, 2048])
@pytest.mark.parametrize("Hc", [2, 8])
def test_cls_passes_over_an_unpadded_x_against_f64(Hc, d, S_max):
    """lstc_cls_dot_var in modes 0 / 1 / 2 (dropout 0.2 replayed), lstc_cls_wsum_var, lstc_cls_outer_var (with add0) against float64
    under util_mask.bar; exact zeros behind S_n."""
    Fn = _Fn()
    lens = CLS_LENS[S_max]
    N = len(lens)
    lay = Fn.unpadded_layout(lens)
    g = torch.Generator().manual_seed(7 * S_max + Hc + d)
    Uv = torch.randn(N, Hc, d, generator=g) * (d ** -0.5)
    G = torch.randn(N, Hc, d, generator=g)
    X = torch.randn(lay.M, d, generator=g)
    add0 = torch.randn(N, d, generator=g)
    p_drop, seed = 0.2, 31 + S_max
    keep = Fn.dropout_mask((N, Hc, S_max, S_max), p_drop, seed, DEV)[:, :, 0].cpu()
    Ud, Gd, Xd = Uv.to(DEV), G.to(DEV), X.to(DEV)
    raw, _ = Fn.cls_dot_var(Ud, Xd, lay, 0)
    out, probs = Fn.cls_dot_var(Ud, Xd, lay, 1, None, p_drop, seed)
    ds, _ = Fn.cls_dot_var(Gd, Xd, lay, 2, probs, p_drop, seed)
    ws = Fn.cls_wsum_var(out, Xd, lay)
    dX = Fn.cls_outer_var(out, Gd, ds, Ud, add0.to(DEV), lay, d)
    torch.cuda.synchronize()
    r_raw, _ = U.cls_dot_var(Uv, X, lens, 0)
    r_out, r_p = U.cls_dot_var(Uv, X, lens, 1, keep=keep, p_drop=p_drop)
    r_ds, _ = U.cls_dot_var(G, X, lens, 2, probs=probs.cpu().double(), keep=keep, p_drop=p_drop)
    r_ws = U.cls_wsum_var(out.cpu(), X, lens)
    r_dX = U.cls_outer_var(out.cpu(), G, ds.cpu(), Uv, add0, lens)
    errs = {}
    for name, kind, got, ref in (("raw", "O", raw, r_raw), ("P", "P", probs, r_p), ("out", "O", out, r_out), ("ds", "O", ds, r_ds),
                                 ("wsum", "O", ws, r_ws), ("outer", "O", dX, r_dX)):
        assert torch.isfinite(got).all(), name
        errs[name] = (float((got.cpu().double() - ref).abs().max()), bar(kind, ref))
    for got in (raw, probs, out, ds):
        for n, L in enumerate(lens):
            assert _bitwise_zero(got[n, :, L + 1:]), n
    print(Hc, d, S_max, {k: "%.3e / %.3e" % v for k, v in errs.items()})
    assert all(e <= b for e, b in errs.values()), errs
    for n, L in enumerate(lens):
        assert float((probs[n, :, :L + 1].sum(-1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("S", [2, 49, 128])
def test_cls_passes_at_equal_lengths_are_the_fixed_kernels_bit_for_bit(S):
    Fn = _Fn()
    N, Hc, d = 3, 8, 64
    lay = Fn.unpadded_layout([S - 1] * N)
    g = torch.Generator().manual_seed(S)
    Uv, G = (torch.randn(N, Hc, d, generator=g).to(DEV) for _ in range(2))
    X = torch.randn(N, S, d, generator=g).to(DEV)
    X2 = X.view(N * S, d)
    for mode in (0, 1):
        a = Fn.cls_dot_var(Uv, X2, lay, mode, None, 0.2, 5)
        b = Fn.cls_dot(Uv, X, mode, None, 0.2, 5)
        assert torch.equal(a[0], b[0]) and (mode == 0 or torch.equal(a[1], b[1])), mode
    out, probs = b
    ds_a, _ = Fn.cls_dot_var(G, X2, lay, 2, probs, 0.2, 5)
    ds_b, _ = Fn.cls_dot(G, X, 2, probs, 0.2, 5)
    assert torch.equal(ds_a, ds_b)
    assert torch.equal(Fn.cls_wsum_var(out, X2, lay), Fn.cls_wsum(out, X))
    assert torch.equal(Fn.cls_outer_var(out, G, ds_b, Uv, None, lay, d), Fn.cls_outer(out, G, ds_b, Uv, N, S, d).view(N * S, d))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- model level
VARIANTS = {"plain": {}, "cls_learned": {"CLS_learned": True}, "position": {"position_encoding": True, "max_position_tokens": 128},
            "input_ln": {"input_layerNorm": True}, "no_ffn": {"FFN_need": False}, "gather_fallback": {}}

_built = {}


def _case(name, dropout=0.0):
    """(encoder on the GPU, oracle parameters, oracle cfg, sequences on the CPU); built once per (variant, dropout) - the sequences
    and the parameter values are never modified.  window_depth = 8: the relative index covers 127 patch tokens."""
    key = (name, dropout)
    if key not in _built:
        from lstc_vad_amd.models import Encoder
        kw = R.encoder_kw(8, dropout, **VARIANTS[name])
        torch.manual_seed(29)
        enc = Encoder(**kw)
        with torch.no_grad():
            for layer in enc.layer_stack:
                layer.slf_attn.relative_position_bias_table.normal_(0.0, 0.4)
                for ln in (layer.slf_attn.layer_norm, layer.pos_ffn.layer_norm):
                    ln.weight.add_(0.1 * torch.randn_like(ln.weight))
                    ln.bias.add_(0.1 * torch.randn_like(ln.bias))
            enc.layer_norm.weight.add_(0.1 * torch.randn_like(enc.layer_norm.weight))
            enc.layer_norm.bias.add_(0.1 * torch.randn_like(enc.layer_norm.bias))
        if name == "gather_fallback":
            enc.layer_stack[-1].slf_attn.cls_assoc = False
        P = {k: v.detach().clone() for k, v in enc.state_dict().items()}
        g = torch.Generator().manual_seed(31)
        seqs = [torch.randn(L, 32, generator=g) for L in LENS]
        _built[key] = (enc.to(DEV), P, R.oracle_cfg(kw), seqs)
    return _built[key]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_unpadded_batch_matches_oracle_on_every_sequence_alone(name):
    """eval(): the rows of forward_unpadded and row n of forward_cls_unpadded within 1e-4 of the oracle on sequence n alone; the
    control arm (the padded ``lengths=`` path on the same data) at the same bar."""
    from oracle import lstc_oracle as orc
    enc, P, cfg, seqs = _case(name)
    enc.eval()
    x = torch.cat(seqs, 0).to(DEV)
    _, row0, _ = U.offsets(LENS, 1)
    xp, _ = R.pad_sequences(seqs, 127)
    with torch.no_grad():
        full = enc.forward_unpadded(x, LENS).cpu()
        cls = enc.forward_cls_unpadded(x, torch.tensor(LENS)).cpu()
        cfull = enc(xp.to(DEV), lengths=LENS).cpu()
        ccls = enc.forward_cls(xp.to(DEV), lengths=LENS).cpu()
        torch.cuda.synchronize()
        assert full.shape == (row0[-1], 32) and cls.shape == (len(LENS), 32)
        assert torch.isfinite(full).all() and torch.isfinite(cls).all()
        errs = {}
        for n, (seq, L) in enumerate(zip(seqs, LENS)):
            ref = orc.encoder_forward(P, seq[None], cfg)[0]
            errs[L] = {"unpadded forward": float((full[row0[n]:row0[n + 1]] - ref).abs().max()),
                       "unpadded forward_cls": float((cls[n] - ref[0]).abs().max()),
                       "control forward": float((cfull[n, :L + 1] - ref).abs().max()),
                       "control forward_cls": float((ccls[n] - ref[0]).abs().max())}
    print(name, {L: {k: "%.2e" % v for k, v in e.items()} for L, e in errs.items()})
    bad = {(L, k): v for L, e in errs.items() for k, v in e.items() if not v < 1e-4}
    assert not bad, bad


@pytest.mark.parametrize("name", ["plain", "gather_fallback"])
def test_a_score_does_not_depend_on_what_shares_its_batch(name):
    """Exact-f32 eval(): row n of forward_cls_unpadded on the mixed batch is torch.equal to the call on sequence n alone (every GEMM
    tile form keeps an element's k order and evaluation never chunks K; the offset kernels give a sequence the same bits in any
    batch)."""
    enc, _, _, seqs = _case(name)
    enc.eval()
    with torch.no_grad():
        cls = enc.forward_cls_unpadded(torch.cat(seqs, 0).to(DEV), LENS)
        full = enc.forward_unpadded(torch.cat(seqs, 0).to(DEV), LENS)
        _, row0, _ = U.offsets(LENS, 1)
        bad = []
        for n, s in enumerate(seqs):
            one = enc.forward_cls_unpadded(s.to(DEV), [s.shape[0]])
            one_full = enc.forward_unpadded(s.to(DEV), [s.shape[0]])
            if not (torch.equal(one[0], cls[n]) and torch.equal(one_full, full[row0[n]:row0[n + 1]])):
                bad.append((n, float((one[0] - cls[n]).abs().max()), float((one_full - full[row0[n]:row0[n + 1]]).abs().max())))
    torch.cuda.synchronize()
    assert not bad, bad


@pytest.mark.parametrize("which", ["forward_cls_unpadded", "forward_unpadded"])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_unpadded_gradients_match_oracle_autograd(name, which):
    """Training mode, dropout 0: the gradients of a fixed random projection of the output - every parameter's and the input's - against
    the oracle's autograd summed over the sequences alone, per tensor within 2e-4 * max|g| + 1e-7.  Control arm: the padded path."""
    from oracle import lstc_oracle as orc
    enc, P, cfg, seqs = _case(name)
    enc.train()
    _, row0, _ = U.offsets(LENS, 1)
    cls_only = which == "forward_cls_unpadded"
    g = torch.Generator().manual_seed(77)
    W = torch.randn(len(LENS) if cls_only else row0[-1], 32, generator=g)
    Pg = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in P.items()}
    xs = [s.clone().requires_grad_(True) for s in seqs]
    total = 0.0
    for n, s in enumerate(xs):
        out = orc.encoder_forward(Pg, s[None], cfg, training=True)[0]
        total = total + ((out[0] * W[n]).sum() if cls_only else (out * W[row0[n]:row0[n + 1]]).sum())
    total.backward()
    ref = {k: v.grad for k, v in Pg.items() if v.is_floating_point() and v.grad is not None}
    ref["input"] = torch.cat([s.grad for s in xs], 0)
    arms = {}
    x = torch.cat(seqs, 0).to(DEV).requires_grad_(True)
    enc.zero_grad(set_to_none=True)
    (getattr(enc, which)(x, LENS) * W.to(DEV)).sum().backward()
    arms["unpadded"] = {k: p.grad.detach().cpu().clone() for k, p in enc.named_parameters() if p.grad is not None}
    arms["unpadded"]["input"] = x.grad.cpu()
    enc.zero_grad(set_to_none=True)
    xp = R.pad_sequences(seqs, 127, fill=0.0)[0].to(DEV).requires_grad_(True)
    if cls_only:
        (enc.forward_cls(xp, lengths=LENS) * W.to(DEV)).sum().backward()
    else:
        Wp = torch.zeros(len(LENS), 128, 32)
        for n, L in enumerate(LENS):
            Wp[n, :L + 1] = W[row0[n]:row0[n + 1]]
        (enc(xp, lengths=LENS) * Wp.to(DEV)).sum().backward()
    arms["control"] = {k: p.grad.detach().cpu().clone() for k, p in enc.named_parameters() if p.grad is not None}
    arms["control"]["input"] = torch.cat([xp.grad[n, :L].cpu() for n, L in enumerate(LENS)], 0)
    enc.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    bad = {}
    for arm, grads in arms.items():
        assert set(grads) == set(ref), (arm, set(grads) ^ set(ref))
        for k, gr in grads.items():
            err, t = float((gr - ref[k]).abs().max()), 2e-4 * float(ref[k].abs().max()) + 1e-7
            assert torch.isfinite(gr).all(), (arm, k)
            if not err < t:
                bad[(arm, k)] = (err, t)
    print(name, which, "worst err / bar", {arm: max(float((gr - ref[k]).abs().max()) / (2e-4 * float(ref[k].abs().max()) + 1e-7)
                                                    for k, gr in grads.items()) for arm, grads in arms.items()})
    assert not bad, bad


def test_dropout_draws_are_reproducible_and_ragged():
    """All dropout rates 0.2, training mode: two runs from the same RNG state are equal; the recorded sites carry the ragged shapes -
    the attention counters run over the flat probabilities buffer, the row-wise sites over the M unpadded rows."""
    Fn = _Fn()
    enc, _, _, seqs = _case("position", dropout=0.2)
    enc.train()
    x = torch.cat(seqs, 0).to(DEV)
    lay = Fn.unpadded_layout(LENS)
    outs, notes = [], None
    for _ in range(2):
        Fn.reset_rng(7000)
        torch.manual_seed(3)
        with torch.no_grad(), Fn.record_dropout() as rec:
            outs.append((enc.forward_cls_unpadded(x, LENS), enc.forward_unpadded(x, LENS)))
        notes = list(rec)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    shapes = {}
    for site, p, seed, shape in notes:
        shapes.setdefault(site, set()).add(shape)
    N, M, S_max = lay.N, lay.M, lay.S_max
    assert shapes["position_dropout"] == {(M, 32)}
    assert shapes["layer_stack.0.slf_attn.attn_dropout"] == {(lay.n_probs(2),)}
    assert shapes["layer_stack.0.slf_attn.dropout"] == shapes["layer_stack.0.pos_ffn.dropout"] == {(1, M, 32)}
    assert shapes["layer_stack.2.slf_attn.attn_dropout#cls"] == {(N, 2, S_max, S_max)} and shapes["layer_stack.2.slf_attn.dropout#cls"] == {(N, 32)}
    assert shapes["layer_stack.2.pos_ffn.dropout"] == {(N, 32), (1, M, 32)}          # the CLS-only call and the full one


def _spy(monkeypatch):
    L = _lib()
    spy = _LibSpy(L.load())
    monkeypatch.setattr(L, "load", lambda: spy)
    return spy


@pytest.mark.parametrize("mode,limit", [("f32x3", 1e-4), ("bf16", 2e-2)])
def test_compute_modes(mode, limit, monkeypatch):
    """forward_cls_unpadded in f32x3 within 1e-4 of the oracle, in bf16 mode within the bf16 score bar (2e-2); the offset attention
    entry points ran in both."""
    from oracle import lstc_oracle as orc
    Fn = _Fn()
    enc, P, cfg, seqs = _case("plain")
    enc.eval()
    Fn.set_compute_dtype(mode)
    Fn.set_x3_threshold(0, 0, 0)
    try:
        spy = _spy(monkeypatch)
        with torch.no_grad():
            cls = enc.forward_cls_unpadded(torch.cat(seqs, 0).to(DEV), LENS).cpu()
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
        Fn.set_compute_dtype("fp32")
        Fn.set_x3_threshold()
    with torch.no_grad():
        ref = torch.stack([orc.encoder_forward(P, s[None], cfg)[0, 0] for s in seqs])
    err = float((cls - ref).abs().max())
    print(mode, "%.3e" % err)
    assert err < limit
    assert spy.calls.count("lstc_attn_var_fwd") == 2 and "lstc_attn_fwd" not in spy.calls


def test_routing_of_forward_cls_unpadded(monkeypatch):
    """One launch chain for the whole mixed batch: one concat, per full layer one attention launch and no masked or length kernel, one re-associated CLS layer on the offset passes, and every GEMM on M rows (or N for the CLS-only
    layer) - never N * S_max."""
    Fn = _Fn()
    enc, _, _, seqs = _case("plain")
    enc.train()
    lay = Fn.unpadded_layout(LENS)
    spy = _spy(monkeypatch)
    enc.forward_cls_unpadded(torch.cat(seqs, 0).to(DEV).requires_grad_(True), LENS).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    enc.zero_grad(set_to_none=True)
    c = spy.calls
    assert c.count("lstc_cls_concat_var_fwd") == 1 and c.count("lstc_cls_concat_var_bwd") == 1
    assert c.count("lstc_attn_var_fwd") == 2 and c.count("lstc_attn_var_bwd") == 2
    assert c.count("lstc_cls_dot_var") == 2 and c.count("lstc_cls_wsum_var") == 2 and c.count("lstc_cls_outer_var") == 1
    for name in ("lstc_attn_fwd", "lstc_attn_bwd", "lstc_attn_fwd_masked", "lstc_attn_bwd_masked", "lstc_attn_cls_fwd_masked",
                 "lstc_cls_dot_len", "lstc_cls_dot", "lstc_cls_concat_len_fwd", "lstc_cls_concat_fwd"):
        assert name not in c, name
    rows = set(spy.gemm_rows)
    assert lay.M in rows and lay.N * lay.S_max not in rows
    assert max(rows) == lay.M, rows          # the others: N rows (the CLS-only layer) or a weight's own rows (its gradient)


# ---------------------------------------------------------------------------------------------------- scoring
def test_unpadded_scoring_matches_grouped_scoring_and_the_oracle():
    """The 40-sequence pool of tests/test_ragged_gpu.py (1, 2 and 3 parts at P = 16 plus 1-, 3- and 7-token sequences):
    ``ragged="unpadded"`` within 1e-4 of ``ragged=False`` and of the oracle on every sequence alone, in input order, in one chunk
    and in chunks of 16; a pool with a 129-token sequence raises before any launch."""
    from lstc_vad_amd.models import Classifier
    from lstc_vad_amd.scoring import ltn_sequence_scores
    from oracle import lstc_oracle as orc
    enc, P, cfg, _ = _case("plain")
    enc.eval()
    torch.manual_seed(41)
    head = Classifier(32, 0.0)
    hP = {k: v.detach().clone() for k, v in head.state_dict().items()}
    head = head.to(DEV).eval()
    g = torch.Generator().manual_seed(42)
    lens = [16 * (1 + int(v)) for v in torch.randint(0, 3, (40,), generator=g)] + [1, 3, 7, 1]
    seqs = [torch.randn(L, 32, generator=g) for L in lens]
    dseqs = [s.to(DEV) for s in seqs]
    with torch.no_grad():
        grouped = ltn_sequence_scores(enc, head, dseqs).cpu()
        unpadded = ltn_sequence_scores(enc, head, dseqs, ragged="unpadded").cpu()
        small = ltn_sequence_scores(enc, head, dseqs, max_batch=16, ragged="unpadded").cpu()
        ref = torch.stack([orc.head_forward(hP, orc.encoder_forward(P, s[None], cfg)[:, 0], "classifier", 0.0)[0, 1] for s in seqs])
    errs = {"grouped vs oracle": float((grouped - ref).abs().max()), "unpadded vs oracle": float((unpadded - ref).abs().max()),
            "unpadded vs grouped": float((unpadded - grouped).abs().max()), "unpadded in chunks of 16 vs oracle": float((small - ref).abs().max())}
    print({k: "%.2e" % v for k, v in errs.items()})
    assert float(ref.max() - ref.min()) > 1e-3          # the scores tell the sequences apart: order mistakes would show
    assert all(v < 1e-4 for v in errs.values()), errs
    with pytest.raises(ValueError, match="ragged=True"):
        ltn_sequence_scores(enc, head, dseqs + [torch.randn(128, 32, device=DEV)], ragged="unpadded")
