"""Unpadded batches above 128 tokens on the GPU: the key-tiled attention kernels over sequence offsets (lstc_attn_var_long_fwd /
_bwd), the launch groups of a mixed batch, ``Encoder.forward_unpadded`` / ``forward_cls_unpadded`` / ``forward_cls_spans`` with
``max_tokens=512`` and ``ragged="unpadded_long"`` scoring.

Kernel level, by the recipe of tests/test_unpadded_gpu.py: against the float64 reference on every sequence alone
(util_unpadded.attn_var_reference) under util_mask.bar - the bars the first-generation offset kernels and the fixed key-tiled
kernels meet, and these are the same arithmetic -, operands inside wider blocks between NaN rows and beside NaN columns, outputs and
the probabilities between guards that must survive.  Model level against the oracle on every sequence ALONE within 1e-4, gradients
within 2e-4 * max|g| + 1e-7 per tensor."""
import pytest
import torch

import util_ragged as R
import util_unpadded as U
from util_mask import bar, model_index

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
GUARD = 7.0
H = 2
# S_n = 129, 2, 512, 160, 161, 257, 32, 288: the first length past the old limit, both sides of 32-token tile edges, the maximum, and
# two short sequences that must take the first-generation kernels, unsorted
LENS = [128, 1, 511, 159, 160, 256, 31, 287]
LENS_WIDE = [128, 140]          # with d_k = 272: a second 256-column output group
CASES = [(16, 16, LENS), (48, 32, LENS), (64, 64, LENS), (272, 16, LENS_WIDE)]


def _Fn():
    from lstc_vad_amd import functional as Fn
    return Fn


def _lib():
    from lstc_vad_amd import _lib
    return _lib


def _block(data, ld, fill):
    """``data`` [M, c] inside a [M + 4, ld] buffer of ``fill``: two guard rows in front, two behind, ld - c guard columns.
    Returns (buffer, the [M, ld] block, its [M, c] data view)."""
    M, c = data.shape
    buf = torch.full((M + 4, ld), fill, device=DEV, dtype=F32)
    buf[2:2 + M, :c] = data.to(DEV)
    return buf, buf[2:2 + M], buf[2:2 + M, :c]


def _guards_intact(buf, M, c):
    return bool((buf[:2] == GUARD).all() and (buf[2 + M:] == GUARD).all() and (buf[2:2 + M, c:] == GUARD).all())


_attn_in = {}


def _attn_inputs(dk, dv, lens):
    """CPU inputs of the attention tests, built once per (widths, lengths) and never modified.  The index covers 511 patch tokens."""
    key = (dk, dv, tuple(lens))
    if key not in _attn_in:
        g = torch.Generator().manual_seed(3000 + dk + dv)
        M = sum(lens) + len(lens)
        q, k = (torch.randn(M, H * dk, generator=g) for _ in range(2))
        v, do = (torch.randn(M, H * dv, generator=g) for _ in range(2))
        index, rows = model_index(512, "cpu")
        table = 0.4 * torch.randn(rows, H, generator=g)
        _attn_in[key] = (q, k, v, do, table, index)
    return _attn_in[key]


def _run_attn(lens, dk, dv, q, k, v, do, table, index, p_drop, seed, pad=None, max_tokens=512):
    """Forward and backward through functional.attn_var_fwd / _bwd on ``unpadded_layout(lens, max_tokens)`` with every operand
    inside guarded, wider blocks.  ``pad``: extra columns of the row pitch (default 4; 3 - a misaligned pitch, the scalar operand
    loads - for d_k = 48)."""
    Fn = _Fn()
    lay = Fn.unpadded_layout(lens, max_tokens=max_tokens) if max_tokens else Fn.unpadded_layout(lens)
    M, npr = lay.M, lay.n_probs(H)
    pad = (3 if dk == 48 else 4) if pad is None else pad
    nan = float("nan")
    qb, kb, vb, dob = [_block(t, t.shape[1] + pad, nan)[1] for t in (q, k, v, do)]
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


# ---------------------------------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("dk,dv,lens", CASES, ids=["16x16", "48x32", "64x64", "272x16"])
def test_attention_over_offsets_above_128_tokens_against_f64(dk, dv, lens, p_drop):
    """P, O, dQ, dK, dV, dtable within util_mask.bar of the float64 reference on every sequence alone; the keep mask replayed with
    lstc_dropout_mask over the ragged buffer; every probability row sums to 1 within 1e-5; guards intact (checked in _run_attn)."""
    Fn = _Fn()
    q, k, v, do, table, index = _attn_inputs(dk, dv, lens)
    seed = 5151 + dk
    lay, got = _run_attn(lens, dk, dv, q, k, v, do, table, index, p_drop, seed)
    assert [S > 128 for S, _ in lay.launch_groups()] == ([False, True] if lens is LENS else [True])
    keep = Fn.dropout_mask((lay.n_probs(H),), p_drop, seed, DEV).cpu() if p_drop > 0 else None
    ref = dict(zip(("P", "O", "dQ", "dK", "dV", "dtable"), U.attn_var_reference(q, k, v, do, lens, H, dk, dv, table, index, keep, p_drop)))
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


# ---------------------------------------------------------------------------------------------------- 2. equal lengths
@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("L", [255, 299])
def test_equal_lengths_are_the_fixed_key_tiled_kernels_bit_for_bit(L, p_drop):
    """The offset kernels are instantiations of the key-tiled ones (attn_long_fwd_kernel / attn_long_bwd_kernel with VAR), so at
    equal lengths P, O, dQ, dK, dV are torch.equal to lstc_attn_fwd / _bwd on the [N, S, ...] view in fp32, dropout included (the
    ragged offset of an element is its flat index there).  The bias-table gradient is summed over another chunking: within bar."""
    Fn = _Fn()
    N, S, dk, dv = 3, L + 1, 16, 16
    lens = [L] * N
    q, k, v, do, table, index = _attn_inputs(dk, dv, lens)
    _, got = _run_attn(lens, dk, dv, q, k, v, do, table, index, p_drop, 77, pad=0)
    qd, kd, vd, dod, tb, ix = (t.to(DEV) for t in (q, k, v, do, table, index))
    o, probs = Fn.attn_fwd(qd, kd, vd, N, S, H, dk, dv, tb, ix, p_drop, 77)
    dq, dk_, dv_, dtable = Fn.attn_bwd(dod, qd, kd, vd, probs, N, S, H, dk, dv, tb, ix, p_drop, 77)
    torch.cuda.synchronize()
    assert torch.equal(got["P"], probs.reshape(-1))
    for name, ref in (("O", o), ("dQ", dq), ("dK", dk_), ("dV", dv_)):
        assert torch.equal(got[name], ref), name
    assert float((got["dtable"] - dtable).abs().max()) <= bar("dtable", dtable.double())


# ---------------------------------------------------------------------------------------------------- 3. independence
def test_a_sequence_does_not_depend_on_its_neighbours_above_128_tokens():
    """On the batch of test 1: each sequence alone (N = 1, unpadded_layout([L], max_tokens=512)) and a permutation of the batch give
    the batch's bits for P, O, dQ, dK, dV; two runs are equal, dtable included; and the short sequences' bits are what
    unpadded_layout at the default limit gives for them alone - the kernel that computes a sequence follows S_n alone."""
    dk, dv = 48, 32
    q, k, v, do, table, index = _attn_inputs(dk, dv, LENS)
    lay, got = _run_attn(LENS, dk, dv, q, k, v, do, table, index, 0.0, 0)
    _, again = _run_attn(LENS, dk, dv, q, k, v, do, table, index, 0.0, 0)
    for name in got:
        assert torch.equal(got[name], again[name]), name
    prob0 = lay.prob0(H)
    rows = lambda t, n: t[lay.row0[n]:lay.row0[n + 1]]
    for n, L in enumerate(LENS):
        for max_tokens in ((512, None) if L + 1 <= 128 else (512,)):          # None: the default limit, the 128-token route
            _, one = _run_attn([L], dk, dv, *(rows(t, n) for t in (q, k, v, do)), table, index, 0.0, 0, max_tokens=max_tokens)
            assert torch.equal(one["P"], got["P"][prob0[n]:prob0[n + 1]]), (n, max_tokens)
            for name in ("O", "dQ", "dK", "dV"):
                assert torch.equal(one[name], rows(got[name], n)), (n, name, max_tokens)
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    pl = [LENS[i] for i in perm]
    play, pgot = _run_attn(pl, dk, dv, *(torch.cat([rows(t, i) for i in perm], 0) for t in (q, k, v, do)), table, index, 0.0, 0)
    pp0 = play.prob0(H)
    for j, i in enumerate(perm):
        assert torch.equal(pgot["P"][pp0[j]:pp0[j + 1]], got["P"][prob0[i]:prob0[i + 1]]), i
        for name in ("O", "dQ", "dK", "dV"):
            assert torch.equal(pgot[name][play.row0[j]:play.row0[j + 1]], rows(got[name], i)), (i, name)


# ---------------------------------------------------------------------------------------------------- 4. refusals
def test_long_entry_points_check_before_any_launch():
    """Every refusal of lstc_attn_var_long_fwd / _bwd by return code (include/lstc_hip.h: LSTC_E_NULL -1, _SHAPE -2, _UNSUPPORTED -4,
    _RANGE -5); a correct call to each returns 0."""
    import ctypes as C
    L = _lib()
    lib = L.load()
    S, dk = 130, 16
    t = torch.zeros(S * S, device=DEV)
    d = L.AttnDesc()
    d.N, d.S, d.H, d.dk, d.dv, d.ldq, d.ldk, d.ldv, d.ldo = 1, S, 1, dk, dk, dk, dk, dk, dk
    d.scale = 0.25
    d.Q = d.K = d.V = d.O = d.probs = d.dO = d.dQ = d.dK = d.dV = t.data_ptr()
    i32 = torch.tensor([0, S], dtype=torch.int32, device=DEV)
    i64 = torch.tensor([0, S * S], dtype=torch.int64, device=DEV)

    def seqs(**kw):
        return L.Seqs(**{**dict(row0=i32.data_ptr(), prob0=i64.data_ptr(), seq_ids=None, n_ids=1, n_probs=S * S), **kw})
    st = L.stream_ptr()
    for fn in (lib.lstc_attn_var_long_fwd, lib.lstc_attn_var_long_bwd):
        assert fn(None, C.byref(seqs()), st) == -1 and fn(C.byref(d), None, st) == -1
        assert fn(C.byref(d), C.byref(seqs(row0=None)), st) == -1 and fn(C.byref(d), C.byref(seqs(prob0=None)), st) == -1
        for name in ("Q", "K", "V", "probs") + (("O",) if fn is lib.lstc_attn_var_long_fwd else ("dO", "dQ", "dK", "dV")):
            setattr(d, name, None)
            assert fn(C.byref(d), C.byref(seqs()), st) == -1, name
            setattr(d, name, t.data_ptr())
        for name in ("O_pack", "dQ_pack", "dK_pack", "dV_pack"):
            setattr(d, name, t.data_ptr())
            assert fn(C.byref(d), C.byref(seqs()), st) == -4, name
            setattr(d, name, None)
        for name in ("in_pack_cols", "dO_pack_cols"):
            setattr(d, name, 64)
            assert fn(C.byref(d), C.byref(seqs()), st) == -4, name
            setattr(d, name, 0)
        for s_bad in (128, 4, 513):
            d.S = s_bad
            assert fn(C.byref(d), C.byref(seqs()), st) == -5, s_bad
        d.S = S
        d.dk, d.ldq, d.ldk = 24, 24, 24
        assert fn(C.byref(d), C.byref(seqs()), st) == -5
        d.dk, d.ldq, d.ldk = dk, dk, dk
        d.dv, d.ldv, d.ldo = 8, 8, 8
        assert fn(C.byref(d), C.byref(seqs()), st) == -5
        d.dv, d.ldv, d.ldo = dk, dk, dk
        assert fn(C.byref(d), C.byref(seqs(n_probs=2 ** 32)), st) == -5
        assert fn(C.byref(d), C.byref(seqs(n_ids=0)), st) == -2 and fn(C.byref(d), C.byref(seqs(n_probs=-1)), st) == -2
    rows = 2 * ((S - 1 + 15) // 16) * 49
    tab = torch.zeros(rows, device=DEV)
    idx = torch.zeros((S - 1) * (S - 1), dtype=torch.int64, device=DEV)
    d.index_ld, d.table_rows, d.table, d.index, d.dtable, d.dtable_chunks = S - 1, rows, tab.data_ptr(), idx.data_ptr(), tab.data_ptr(), 0
    assert lib.lstc_attn_var_long_bwd(C.byref(d), C.byref(seqs()), st) == -4          # no atomics: partial tables only
    d.dtable_chunks = 2
    assert lib.lstc_attn_var_long_bwd(C.byref(d), C.byref(seqs()), st) == -2          # one sequence makes one chunk
    d.dtable_chunks = 1
    assert lib.lstc_attn_var_long_fwd(C.byref(d), C.byref(seqs()), st) == 0 and lib.lstc_attn_var_long_bwd(C.byref(d), C.byref(seqs()), st) == 0
    d.S = 129
    for fn in (lib.lstc_attn_var_fwd, lib.lstc_attn_var_bwd):          # the 128-token entry points keep their limit
        assert fn(C.byref(d), C.byref(seqs()), st) == -5
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 5. model level
MLENS = [160, 16, 130, 127, 128]          # S = 161, 17, 131, 128, 129

_built = {}


def _case():
    """(encoder on the GPU, oracle parameters, oracle cfg, sequences on the CPU), built once and never modified: 2 layers, d_model 32,
    H = 2, relative bias over window_depth = 10: the index covers 160 patch tokens."""
    if not _built:
        from lstc_vad_amd.models import Encoder
        kw = R.encoder_kw(10, 0.0, n_layers=2)
        torch.manual_seed(37)
        enc = Encoder(**kw)
        with torch.no_grad():
            for layer in enc.layer_stack:
                layer.slf_attn.relative_position_bias_table.normal_(0.0, 0.4)
                for ln in (layer.slf_attn.layer_norm, layer.pos_ffn.layer_norm):
                    ln.weight.add_(0.1 * torch.randn_like(ln.weight))
                    ln.bias.add_(0.1 * torch.randn_like(ln.bias))
        P = {k: v.detach().clone() for k, v in enc.state_dict().items()}
        g = torch.Generator().manual_seed(39)
        seqs = [torch.randn(L, 32, generator=g) for L in MLENS]
        _built["case"] = (enc.to(DEV), P, R.oracle_cfg(kw), seqs)
    return _built["case"]


def test_encoder_above_128_tokens_matches_oracle_on_every_sequence_alone():
    """eval(): the rows of forward_unpadded and row n of forward_cls_unpadded, both with max_tokens=512, within 1e-4 of the oracle
    on sequence n alone.  Bit for bit: the rows of a sequence in forward_unpadded are those of the call on it alone, and its row of
    forward_cls_unpadded does not change when a neighbour leaves the batch (the first sequence; the batch keeps a sequence above
    128 tokens, so the last layer keeps its form - the full block and a gather)."""
    from oracle import lstc_oracle as orc
    enc, P, cfg, seqs = _case()
    enc.eval()
    x = torch.cat(seqs, 0).to(DEV)
    _, row0, _ = U.offsets(MLENS, 1)
    with torch.no_grad():
        full_d = enc.forward_unpadded(x, MLENS, max_tokens=512)
        cls_d = enc.forward_cls_unpadded(x, torch.tensor(MLENS), max_tokens=512)
        less = enc.forward_cls_unpadded(torch.cat(seqs[1:], 0).to(DEV), MLENS[1:], max_tokens=512)
        alone = [enc.forward_unpadded(s.to(DEV), [s.shape[0]], max_tokens=512) for s in seqs]
        torch.cuda.synchronize()
        full, cls = full_d.cpu(), cls_d.cpu()
        assert full.shape == (row0[-1], 32) and cls.shape == (len(MLENS), 32)
        assert torch.isfinite(full).all() and torch.isfinite(cls).all()
        errs = {}
        for n, (seq, L) in enumerate(zip(seqs, MLENS)):
            ref = orc.encoder_forward(P, seq[None], cfg)[0]
            errs[L] = {"forward": float((full[row0[n]:row0[n + 1]] - ref).abs().max()), "forward_cls": float((cls[n] - ref[0]).abs().max())}
    print({L: {k: "%.2e" % v for k, v in e.items()} for L, e in errs.items()})
    bad = {(L, k): v for L, e in errs.items() for k, v in e.items() if not v < 1e-4}
    assert not bad, bad
    assert torch.equal(less, cls_d[1:])
    for n, one in enumerate(alone):
        assert torch.equal(one, full_d[row0[n]:row0[n + 1]]), n


@pytest.mark.parametrize("which", ["forward_cls_unpadded", "forward_unpadded"])
def test_gradients_above_128_tokens_match_oracle_autograd(which):
    """Training mode, dropout 0: the gradients of a fixed random projection of the output - every parameter's and the input's - against
    the oracle's autograd summed over the sequences alone, per tensor within 2e-4 * max|g| + 1e-7."""
    from oracle import lstc_oracle as orc
    enc, P, cfg, seqs = _case()
    enc.train()
    _, row0, _ = U.offsets(MLENS, 1)
    cls_only = which == "forward_cls_unpadded"
    g = torch.Generator().manual_seed(79)
    W = torch.randn(len(MLENS) if cls_only else row0[-1], 32, generator=g)
    Pg = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in P.items()}
    xs = [s.clone().requires_grad_(True) for s in seqs]
    total = 0.0
    for n, s in enumerate(xs):
        out = orc.encoder_forward(Pg, s[None], cfg, training=True)[0]
        total = total + ((out[0] * W[n]).sum() if cls_only else (out * W[row0[n]:row0[n + 1]]).sum())
    total.backward()
    ref = {k: v.grad for k, v in Pg.items() if v.is_floating_point() and v.grad is not None}
    ref["input"] = torch.cat([s.grad for s in xs], 0)
    x = torch.cat(seqs, 0).to(DEV).requires_grad_(True)
    enc.zero_grad(set_to_none=True)
    (getattr(enc, which)(x, MLENS, max_tokens=512) * W.to(DEV)).sum().backward()
    grads = {k: p.grad.detach().cpu().clone() for k, p in enc.named_parameters() if p.grad is not None}
    grads["input"] = x.grad.cpu()
    enc.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    assert set(grads) == set(ref), set(grads) ^ set(ref)
    bad = {}
    for k, gr in grads.items():
        err, t = float((gr - ref[k]).abs().max()), 2e-4 * float(ref[k].abs().max()) + 1e-7
        assert torch.isfinite(gr).all(), k
        if not err < t:
            bad[k] = (err, t)
    print(which, "worst err / bar", max(float((gr - ref[k]).abs().max()) / (2e-4 * float(ref[k].abs().max()) + 1e-7) for k, gr in grads.items()))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- 6. scoring
def _head():
    from lstc_vad_amd.models import Classifier
    torch.manual_seed(43)
    head = Classifier(32, 0.0)
    hP = {k: v.detach().clone() for k, v in head.state_dict().items()}
    return head.to(DEV).eval(), hP


def test_unpadded_long_scoring_matches_padded_scoring_and_the_oracle():
    """A pool of the model test's lengths, twice over in another order: ``ragged="unpadded_long"`` within 1e-4 of ``ragged=True``
    and of the oracle on every sequence alone, in input order, in one chunk and in chunks of 3; ``ragged="unpadded"`` still refuses
    the pool and points to ragged=True."""
    from lstc_vad_amd.scoring import ltn_sequence_scores
    from oracle import lstc_oracle as orc
    enc, P, cfg, _ = _case()
    enc.eval()
    head, hP = _head()
    g = torch.Generator().manual_seed(44)
    lens = MLENS + [128, 16, 160, 1, 130, 127]
    seqs = [torch.randn(L, 32, generator=g) for L in lens]
    dseqs = [s.to(DEV) for s in seqs]
    with torch.no_grad():
        padded = ltn_sequence_scores(enc, head, dseqs, ragged=True).cpu()
        unpadded = ltn_sequence_scores(enc, head, dseqs, ragged="unpadded_long").cpu()
        small = ltn_sequence_scores(enc, head, dseqs, max_batch=3, ragged="unpadded_long").cpu()
        ref = torch.stack([orc.head_forward(hP, orc.encoder_forward(P, s[None], cfg)[:, 0], "classifier", 0.0)[0, 1] for s in seqs])
    errs = {"padded vs oracle": float((padded - ref).abs().max()), "unpadded_long vs oracle": float((unpadded - ref).abs().max()),
            "unpadded_long vs padded": float((unpadded - padded).abs().max()), "chunks of 3 vs oracle": float((small - ref).abs().max())}
    print({k: "%.2e" % v for k, v in errs.items()})
    assert float(ref.max() - ref.min()) > 1e-3          # the scores tell the sequences apart: order mistakes would show
    assert all(v < 1e-4 for v in errs.values()), errs
    with pytest.raises(ValueError, match="ragged=True"):
        ltn_sequence_scores(enc, head, dseqs, ragged="unpadded")


def test_resident_spans_above_128_tokens_are_the_cut_out_tokens_bit_for_bit():
    """``resident_sequence_scores(..., ragged="unpadded_long")`` on spans of a bank - overlapping, repeated, unsorted - equals the head
    on ``forward_cls_unpadded(cut-out tokens, max_tokens=512)`` bit for bit, in one chunk and in the scorer's chunks at max_batch = 2
    (the same chunks on both sides: the last layer's form follows the longest sequence of a chunk)."""
    from lstc_vad_amd.scoring import UNPADDED_ROWS_PER_SEQUENCE, resident_sequence_scores, unpadded_chunks
    enc, _, _, _ = _case()
    enc.eval()
    head, _ = _head()
    g = torch.Generator().manual_seed(45)
    bank = torch.randn(400, 32, generator=g).to(DEV)
    spans = [(0, 160), (150, 16), (37, 130), (273, 127), (200, 128), (0, 160), (399, 1)]
    with torch.no_grad():
        got = resident_sequence_scores(enc, head, bank, spans, ragged="unpadded_long")
        by2 = resident_sequence_scores(enc, head, bank, spans, max_batch=2, ragged="unpadded_long")
        x = torch.cat([bank[r:r + t] for r, t in spans], 0)
        want = head(enc.forward_cls_unpadded(x, [t for _, t in spans], max_tokens=512)).view(-1, 2)[:, 1]
        chunks = unpadded_chunks([t for _, t in spans], 2, UNPADDED_ROWS_PER_SEQUENCE * 2, 2)          # the scorer's own rule
        assert len(chunks) > 2 and [i for c in chunks for i in c] == list(range(len(spans)))
        want2 = torch.cat([head(enc.forward_cls_unpadded(torch.cat([bank[spans[i][0]:sum(spans[i])] for i in c], 0),
                                                         [spans[i][1] for i in c], max_tokens=512)).view(-1, 2)[:, 1] for c in chunks])
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and float(got.max() - got.min()) > 1e-4
    assert torch.equal(got, want) and torch.equal(by2, want2)
    with pytest.raises(ValueError, match="at most 127"):
        resident_sequence_scores(enc, head, bank, spans, ragged="unpadded")
