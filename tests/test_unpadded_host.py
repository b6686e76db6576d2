"""Unpadded batches, host side (no GPU): the layout helper and its refusals, the ABI of the new POD, the float64 references of
tests/util_unpadded.py against torch.autograd on each sequence alone, and ``scoring.unpadded_batches``."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import util_unpadded as U
from util_mask import model_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------- 1. layout, refusals, ABI
def test_layout_offsets_and_buckets():
    from lstc_vad_amd.functional import unpadded_layout
    lens, H = U.LENGTHS, 2
    lay = unpadded_layout(lens)
    in0, row0, prob0 = U.offsets(lens, H)
    assert (lay.in0, lay.row0, lay.prob0(H)) == (in0, row0, prob0)
    assert lay.N == 10 and lay.M == sum(lens) + 10 and lay.S_max == 128 and lay.n_probs(H) == prob0[-1] and not lay.equal
    # S = 64, 2, 128, 16, 33, 97, 3, 65, 32, 96 -> T = ceil(S_n / 32) = 2, 1, 4, 1, 2, 4, 1, 3, 1, 3; ids ascending
    assert lay.buckets == {1: [1, 3, 6, 8], 2: [0, 4], 3: [7, 9], 4: [2, 5]}
    assert unpadded_layout(torch.tensor([4, 4, 4])).equal and unpadded_layout(torch.tensor([4, 4, 4])).row0 == [0, 5, 10, 15]


@pytest.mark.parametrize("bad", [[], [3, 0], [3, 128], [3, 2.5], [True, 2], torch.tensor([1.0, 2.0]), torch.ones(2, 2, dtype=torch.int64)])
def test_layout_refuses_bad_lengths(bad):
    from lstc_vad_amd.functional import unpadded_layout
    with pytest.raises(ValueError):
        unpadded_layout(bad)


def test_layout_names_the_limit():
    from lstc_vad_amd.functional import unpadded_layout
    with pytest.raises(ValueError, match="128"):
        unpadded_layout([5, 128])


def _enc(**extra):
    import util_ragged as R
    from lstc_vad_amd.models import Encoder
    return Encoder(**R.encoder_kw(2, **extra))


def test_every_refusal_is_raised_on_cpu_tensors_before_the_device_check():
    from lstc_vad_amd.functional import PackedAct
    enc = _enc()
    x = torch.randn(10, 32)
    lens = [4, 6]
    for fn in (enc.forward_unpadded, enc.forward_cls_unpadded):
        with pytest.raises(NotImplementedError):
            fn(x, lens, src_mask=torch.ones(7, 7))
        with pytest.raises(NotImplementedError):
            fn(PackedAct(x.to(torch.bfloat16), (1, 10, 32)), lens)
        with pytest.raises(ValueError, match="gather spec"):
            fn((x.view(1, 10, 32), torch.zeros(1, dtype=torch.int64), 1, 1), lens)
        with pytest.raises(ValueError, match="sum to"):
            fn(x, [4, 5])
        with pytest.raises(ValueError, match="128"):
            fn(torch.randn(132, 32), [4, 128])
        with pytest.raises(ValueError, match="relative position index"):
            fn(torch.randn(37, 32), [4, 33])                       # window_depth 2: the index covers 32 patch tokens
        with pytest.raises(ValueError):
            fn(x.view(1, 10, 32), lens)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, lens)                                            # everything in order: only the device is wrong
    with pytest.raises(NotImplementedError):
        enc.forward_unpadded(x, lens, return_attn=True)
    with pytest.raises(NotImplementedError):
        enc.forward_unpadded(x, lens, return_attn_v=True)
    with pytest.raises(ValueError, match="enc_output_hi"):
        enc.forward_cls_unpadded(x, lens, enc_output_hi=x)
    with pytest.raises(ValueError, match="max_position_tokens"):
        _enc(position_encoding=True, max_position_tokens=6).forward_cls_unpadded(x, lens)
    e2 = _enc(relative_pe=False, relative_pe_2D=True)
    with pytest.raises(ValueError, match="relative_pe_2D"):
        e2.forward_cls_unpadded(torch.randn(20, 32), [16, 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e2.forward_cls_unpadded(torch.randn(32, 32), [16, 16])


def test_seqs_struct_matches_the_header(tmp_path):
    from lstc_vad_amd import _lib
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lstc_hip.h"', 'int main(void) {',
             'printf("LstcSeqs %zu\\n", sizeof(LstcSeqs));', 'printf("version %d\\n", LSTC_VERSION);']
    for fname, _ in _lib.Seqs._fields_:
        lines.append(f'printf("LstcSeqs.{fname} %zu %zu\\n", offsetof(LstcSeqs, {fname}), sizeof(((LstcSeqs*)0)->{fname}));')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert int(got["LstcSeqs"][0]) == C.sizeof(_lib.Seqs) == 40
    assert int(got["version"][0]) == 112 == _lib.load().lstc_version()
    for fname, ctype in _lib.Seqs._fields_:
        off, size = (int(v) for v in got[f"LstcSeqs.{fname}"])
        assert off == getattr(_lib.Seqs, fname).offset and size == C.sizeof(ctype), fname
    assert [f for f, _ in _lib.Seqs._fields_] == ["row0", "prob0", "seq_ids", "n_ids", "n_probs"]
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("lstc_attn_var_fwd", "lstc_attn_var_bwd", "lstc_cls_dot_var", "lstc_cls_wsum_var", "lstc_cls_outer_var",
                 "lstc_cls_concat_var_fwd", "lstc_cls_concat_var_bwd"):
        assert hasattr(lib, name) and name in _lib.EXPORTS, name


# ---------------------------------------------------------------------------------------------------- 2. the references
LENS = [5, 1, 33, 2]


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("learned", [False, True])
def test_concat_reference_against_autograd(learned, with_pos):
    g = torch.Generator().manual_seed(3 + 2 * learned + with_pos)
    d, S_max = 6, max(LENS) + 1
    in0, row0, _ = U.offsets(LENS, 1)
    x = torch.randn(in0[-1], d, generator=g, dtype=F64, requires_grad=True)
    cls = torch.randn(d, generator=g, dtype=F64, requires_grad=True) if learned else None
    pos = torch.randn(S_max, d, generator=g, dtype=F64, requires_grad=True) if with_pos else None
    dy = torch.randn(row0[-1], d, generator=g, dtype=F64)
    ys = []
    for n, L in enumerate(LENS):          # each sequence alone, as the reference's Encoder builds it (models/Encoder.py:51-58)
        xs = x[in0[n]:in0[n + 1]]
        y = torch.cat([cls[None] if learned else xs.mean(0, keepdim=True), xs], 0)
        ys.append(y + pos[:L + 1] if with_pos else y)
    y = torch.cat(ys, 0)
    y.backward(dy)
    assert torch.allclose(U.concat_var_fwd(x.detach(), LENS, cls, pos), y.detach(), rtol=0, atol=1e-14)
    dx, dtok = U.concat_var_bwd(dy, LENS, not learned)
    assert torch.allclose(dx, x.grad, rtol=0, atol=1e-14)
    if learned:
        assert torch.allclose(dtok[0], cls.grad, rtol=0, atol=1e-13)
    if with_pos:
        assert torch.allclose(dtok, pos.grad, rtol=0, atol=1e-13)


@pytest.mark.parametrize("p_drop", [0.0, 0.25])
def test_attention_reference_against_autograd(p_drop):
    H, dk, dv = 2, 5, 3
    g = torch.Generator().manual_seed(11)
    _, row0, prob0 = U.offsets(LENS, H)
    M = row0[-1]
    q, k = (torch.randn(M, H * dk, generator=g, dtype=F64) for _ in range(2))
    v, do = (torch.randn(M, H * dv, generator=g, dtype=F64) for _ in range(2))
    index, rows = model_index(max(LENS) + 1, "cpu")
    table = 0.4 * torch.randn(rows, H, generator=g, dtype=F64)
    keep = (torch.rand(prob0[-1], generator=g) >= p_drop) if p_drop > 0 else None
    P, O, dQ, dK, dV, dT = U.attn_var_reference(q, k, v, do, LENS, H, dk, dv, table, index, keep, p_drop)
    t = table.clone().requires_grad_(True)
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    outs = []
    for n, L in enumerate(LENS):          # models/MultiHeadAttention.py:97-122 on each sequence alone
        S, r = L + 1, slice(row0[n], row0[n + 1])
        qh, kh, vh = (x[r].view(S, H, -1).transpose(0, 1) for x in leaves)
        a = (qh / dk ** 0.5) @ kh.transpose(1, 2)
        bias = t[index[:L, :L].reshape(-1)].view(L, L, H).permute(2, 0, 1)
        a = torch.cat([a[:, :1], torch.cat([a[:, 1:, :1], a[:, 1:, 1:] + bias], 2)], 1)
        p = torch.softmax(a, -1)
        assert torch.allclose(P[prob0[n]:prob0[n + 1]].view(H, S, S), p.detach(), rtol=0, atol=1e-14)
        if keep is not None:
            p = p * keep[prob0[n]:prob0[n + 1]].view(H, S, S) / (1 - p_drop)
        outs.append((p @ vh).transpose(0, 1).reshape(S, H * dv))
    o = torch.cat(outs, 0)
    o.backward(do)
    for got, ref in ((O, o.detach()), (dQ, leaves[0].grad), (dK, leaves[1].grad), (dV, leaves[2].grad), (dT, t.grad)):
        assert torch.allclose(got, ref, rtol=0, atol=1e-12)


def test_cls_pass_references_against_autograd():
    H, d = 2, 6
    g = torch.Generator().manual_seed(5)
    _, row0, _ = U.offsets(LENS, 1)
    N, S_max = len(LENS), max(LENS) + 1
    Uv = torch.randn(N, H, d, generator=g, dtype=F64, requires_grad=True)
    X = torch.randn(row0[-1], d, generator=g, dtype=F64, requires_grad=True)
    gy = torch.randn(N, H, d, generator=g, dtype=F64)
    ys = []
    for n, L in enumerate(LENS):
        xs = X[row0[n]:row0[n + 1]]
        p = torch.softmax(Uv[n] @ xs.t(), -1)                      # [H, S_n]
        ys.append(p @ xs)
    y = torch.stack(ys)
    y.backward(gy)
    raw, _ = U.cls_dot_var(Uv.detach(), X.detach(), LENS, 0)
    out, probs = U.cls_dot_var(Uv.detach(), X.detach(), LENS, 1)
    for n, L in enumerate(LENS):
        assert torch.allclose(raw[n, :, :L + 1], (Uv[n] @ X[row0[n]:row0[n + 1]].t()).detach(), rtol=0, atol=1e-13)
        assert (raw[n, :, L + 1:] == 0).all() and (probs[n, :, L + 1:] == 0).all()
    assert torch.allclose(U.cls_wsum_var(out, X.detach(), LENS), y.detach(), rtol=0, atol=1e-13)
    # backward of the chain: d(logit) = mode 2 on the gradient of the weighted sum, dU = wsum(ds), dX = outer(P, gy, ds, U)
    ds, _ = U.cls_dot_var(gy, X.detach(), LENS, 2, probs=probs)
    assert torch.allclose(U.cls_wsum_var(ds, X.detach(), LENS), Uv.grad, rtol=0, atol=1e-12)
    assert torch.allclose(U.cls_outer_var(out, gy, ds, Uv.detach(), None, LENS), X.grad, rtol=0, atol=1e-12)
    add0 = torch.randn(N, d, generator=g, dtype=F64)
    with_add = U.cls_outer_var(out, gy, ds, Uv.detach(), add0, LENS)
    diff = with_add - X.grad
    for n in range(N):
        assert torch.allclose(diff[row0[n]], add0[n], rtol=0, atol=1e-12) and float(diff[row0[n] + 1:row0[n + 1]].abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------------- 3. unpadded_batches
def test_unpadded_batches_ids_concatenation_cap_and_order():
    from lstc_vad_amd.scoring import unpadded_batches
    g = torch.Generator().manual_seed(1)
    lens = [16, 48, 1, 32, 7, 48, 16, 3]
    seqs = [torch.randn(L, 4, generator=g) for L in lens]
    one = unpadded_batches(seqs)
    assert len(one) == 1 and one[0][0] == list(range(8)) and one[0][2] == lens and torch.equal(one[0][1], torch.cat(seqs, 0))
    by3 = unpadded_batches(seqs, max_batch=3)
    assert [b[0] for b in by3] == [[0, 1, 2], [3, 4, 5], [6, 7]]
    # rows count the CLS tokens: 17 + 49 + 2 = 68 <= 70 < 68 + 33; 33 + 8 = 41 <= 70 < 41 + 49; 49 + 17 + 4 = 70
    capped = unpadded_batches(seqs, max_batch=100, max_rows=70)
    assert [b[0] for b in capped] == [[0, 1, 2], [3, 4], [5, 6, 7]]
    for ids, x, ls in by3 + capped:
        assert ls == [lens[i] for i in ids] and torch.equal(x, torch.cat([seqs[i] for i in ids], 0))
        assert ids == list(range(ids[0], ids[-1] + 1))                    # consecutive: results go back in input order
    assert [b[0] for b in unpadded_batches(seqs, max_batch=100, max_rows=10)] == [[i] for i in range(8)]      # a single sequence always fits
    assert unpadded_batches(seqs, max_batch=2)[0][0] == [0, 1] and 49 * 4096 == 200704      # the default cap: 49 rows per sequence


def test_unpadded_scoring_refuses_a_long_sequence_before_any_launch():
    from lstc_vad_amd.scoring import ltn_sequence_scores
    seqs = [torch.randn(16, 32), torch.randn(128, 32)]                   # CPU tensors: a launch would raise RuntimeError instead
    with pytest.raises(ValueError, match="ragged=True"):
        ltn_sequence_scores(None, None, seqs, ragged="unpadded")
    with pytest.raises(ValueError, match="unpadded"):
        ltn_sequence_scores(None, None, seqs[:1], ragged="packed")


@pytest.mark.parametrize("ragged,want", [(False, {}), (True, {"ragged": True}), ("unpadded", {"ragged": "unpadded"})])
def test_pipeline_passes_the_ragged_value_on(ragged, want, monkeypatch):
    """The score board of generate_pseudo_labels / evaluate_auc hands ``ragged`` to ltn_sequence_scores as it is (and nothing when
    it is False: the call that existed before the keyword)."""
    from lstc_vad_amd import pipeline
    seen = []

    def fake(enc, head, seqs, **kw):
        seen.append(kw)
        return torch.zeros(len(seqs))
    monkeypatch.setattr(pipeline.scoring, "ltn_sequence_scores", fake)
    board = pipeline._ScoreBoard(None, None, "cpu", 0, 1, None, 100, None, ragged)
    board.add_ltn(0, 2, lambda: [torch.zeros(16, 4), torch.zeros(3, 4)], lambda s: s)
    board.flush()
    assert seen == [want]
