"""Resident scoring, host side (no GPU): the argument checks of lstc_cls_concat_span_fwd / lstc_segment_mean, the span bookkeeping
of scoring.py against the sequences the host route cuts out, every refusal of the new entry points before the device matters, and
the --resident_eval flag."""
import ctypes as C
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import util_ragged as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------- 1. the C ABI
def test_library_exports_the_two_entries(lib):
    from lstc_vad_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "lstc_hip.h")).read()
    for name in ("lstc_cls_concat_span_fwd", "lstc_segment_mean"):
        assert hasattr(raw, name) and name in _lib.EXPORTS and name + "(" in hdr, name
    assert lib.lstc_version() == 112                    # additions only: the version stays


def test_host_side_validation_error_codes(lib):
    span, seg = lib.lstc_cls_concat_span_fwd, lib.lstc_segment_mean
    # (bank, bank_rows, src0, row0, cls, pos, y, N, d, stream): NULL operands -1, then shapes -2, as lstc_cls_concat_var_fwd
    ok = [16, 8, 16, 16, None, None, 16, 2, 32, None]
    for i in (0, 2, 3, 6):
        a = list(ok)
        a[i] = None
        assert span(*a) == -1, i
    for i, bad in ((7, 0), (7, -3), (8, 0), (8, -1), (1, 0), (1, -5)):
        a = list(ok)
        a[i] = bad
        assert span(*a) == -2, (i, bad)
    assert lib.lstc_cls_concat_var_fwd(None, 16, None, None, 16, 2, 32, None) == -1         # the neighbour's codes
    assert lib.lstc_cls_concat_var_fwd(16, 16, None, None, 16, 0, 32, None) == -2
    # (bank, bank_clips, first, count, n_seg, P, d, l2, out, stream)
    ok = [16, 8, 16, 16, 4, 9, 32, 0, 16, None]
    for i in (0, 2, 3, 8):
        a = list(ok)
        a[i] = None
        assert seg(*a) == -1, i
    for i, bad in ((1, 0), (4, 0), (4, -1), (5, 0), (6, 0), (6, -4), (4, 1 << 31)):          # the last: n_seg * P beyond the grid
        a = list(ok)
        a[i] = bad
        assert seg(*a) == -2, (i, bad)


# ---------------------------------------------------------------------------------------------------- 2. span bookkeeping
def _videos(counts, P, d, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, P, d, generator=g) for n in counts]


@pytest.mark.parametrize("tail", ["short", "rewindow"])
def test_part_spans_slice_the_bank_into_the_host_routes_sequences(tail):
    """n_clips 1, 2 (shorter than a part: the reference's negative slice start), 3 (an exact multiple), 7 at part_len 3, P = 4."""
    from lstc_vad_amd import scoring
    counts, P, d, L = [1, 2, 3, 7], 4, 8, 3
    vids = _videos(counts, P, d, 1)
    bank = torch.cat(vids, 0)
    rows = bank.view(-1, d)
    first = 0
    for v in vids:
        seqs, ranges = scoring.ltn_part_sequences(v, L, tail=tail)
        spans, ranges2 = scoring.part_spans(v.shape[0], L, P, tail, first)
        assert ranges2 == ranges == scoring.part_ranges(v.shape[0], L) and len(spans) == len(seqs)
        for (r, t), s in zip(spans, seqs):
            assert torch.equal(rows[r:r + t], s), (tail, v.shape[0], r, t)
        first += v.shape[0]
    # an STN is part_len 1: one span per clip
    spans, _ = scoring.part_spans(7, 1, P, first_clip=6)
    assert spans == [((6 + c) * P, P) for c in range(7)]


@pytest.mark.parametrize("n_clips", [5, 32, 33, 100])
def test_ucf_bin_table_against_the_bins_edges(n_clips):
    from lstc_vad_amd import scoring
    P, d, first_clip = 3, 4, 11
    g = torch.Generator().manual_seed(n_clips)
    bank = torch.randn(first_clip + n_clips + 2, P, d, generator=g, dtype=torch.float64)
    feats = bank[first_clip:first_clip + n_clips]
    n_frames = n_clips * 16 + 7
    bins, r = scoring.ucf_bins(feats, n_frames)
    first, count = scoring.ucf_bin_table(n_frames, first_clip=first_clip, n_clips=n_clips)
    assert np.array_equal(r, scoring.ucf_bin_edges(n_frames)) and len(first) == len(count) == 32
    for i in range(32):
        assert first[i] == first_clip + int(r[i]) and count[i] == max(int(r[i + 1] - r[i]), 1)
        if r[i] == r[i + 1]:
            assert count[i] == 1 and torch.equal(bank[first[i]], bins[i])             # an empty bin: clip r[i] alone
        want = bank[first[i]:first[i] + count[i]].mean(0)
        assert torch.allclose(want, bins[i], rtol=0, atol=1e-14)
    if n_clips == 5:
        assert sum(int(r[i] == r[i + 1]) for i in range(32)) == 27
    with pytest.raises(ValueError, match="starts at clip"):
        scoring.ucf_bin_table(n_frames, n_clips=int(r[31]))                # the list promises more clips than the video has


@pytest.mark.parametrize("rewindow", [True, False])
@pytest.mark.parametrize("part_len", [2, 3])
def test_ucf_bin_spans_against_the_bin_ranges(part_len, rewindow):
    from lstc_vad_amd import scoring
    P, d, first_bin = 3, 4, 64
    bins_bank = torch.randn(first_bin + 32, P, d, generator=torch.Generator().manual_seed(2))
    feats = torch.randn(40, P, d, generator=torch.Generator().manual_seed(3))
    seqs, ranges, _ = scoring.ltn_ucf_bin_sequences(feats, 40 * 16, part_len, normalize=False, rewindow=rewindow)
    spans = scoring.ucf_bin_spans(part_len, rewindow, P, first_bin)
    assert ranges == scoring.ucf_bin_ranges(part_len, rewindow) and len(spans) == len(ranges) == len(seqs)
    rows = bins_bank.view(-1, d)
    for (r, t), (b, e), s in zip(spans, ranges, seqs):
        assert torch.equal(rows[r:r + t], bins_bank[first_bin + b:first_bin + e].reshape(-1, d)) and t == s.shape[0]


def test_unpadded_chunks_is_the_rule_of_unpadded_batches():
    from lstc_vad_amd import scoring
    lens = [16, 48, 1, 32, 7, 48, 16, 3]
    seqs = [torch.zeros(L, 4) for L in lens]
    for mb, mr in ((4096, 49 * 4096), (3, 49 * 3), (100, 70), (100, 10)):
        assert scoring.unpadded_chunks(lens, mb, mr) == [b[0] for b in scoring.unpadded_batches(seqs, mb, mr)]


def test_resident_set_from_arrays_offsets_owners_and_bytes():
    from lstc_vad_amd.pipeline import ResidentSet
    arrays = [np.random.RandomState(i).randn(n, 6, 8).astype(np.float32) for i, n in enumerate([3, 1, 5, 2])]
    rs = ResidentSet.from_arrays(arrays, "cpu", keys=["a.npy", "b", "c", "d"], n_patch=4)
    assert rs.keys == ["a", "b", "c", "d"] and tuple(rs.bank.shape) == (11, 4, 8)
    assert rs.offsets.tolist() == [0, 3, 4, 9] and rs.lens.tolist() == [3, 1, 5, 2]
    for k, a in zip(rs.keys, arrays):
        o = rs.first_clip(k + ".npy")
        assert torch.equal(rs.bank[o:o + rs.n_clips(k)], torch.from_numpy(a[:, :4, :]))
    assert ResidentSet.bytes([a.shape for a in arrays], 4) == rs.bank.numel() * 4
    own = lambda i: i % 2 == 1
    half = ResidentSet.from_arrays(arrays, "cpu", keys=rs.keys, n_patch=4, owns=own)
    assert half.offsets.tolist() == [-1, 0, -1, 1] and half.lens.tolist() == [3, 1, 5, 2] and half.bank.shape[0] == 3
    assert ResidentSet.bytes([a.shape for a in arrays], 4, owns=own) == half.bank.numel() * 4
    with pytest.raises(ValueError, match="not uploaded"):
        half.first_clip("a")
    # view=True: any stored shape viewed [-1, n_patch, d] (the UCF routes)
    flat = ResidentSet.from_arrays([a.reshape(-1, 8) for a in arrays], "cpu", n_patch=6, view=True)
    assert tuple(flat.bank.shape) == (11, 6, 8) and torch.equal(flat.bank[3:4], torch.from_numpy(arrays[1]))
    with pytest.raises(ValueError, match="n_patch"):
        rs.patches(16, "evaluate_auc")


# ---------------------------------------------------------------------------------------------------- 3. refusals
def _enc(**extra):
    from lstc_vad_amd.models import Encoder
    return Encoder(**R.encoder_kw(2, **extra))


def test_every_refusal_of_forward_cls_spans_is_raised_before_the_device_check():
    from lstc_vad_amd.functional import PackedAct
    enc = _enc()
    bank = torch.randn(40, 32)
    with pytest.raises(ValueError, match="input LayerNorm"):
        _enc(input_layerNorm=True).forward_cls_spans(bank, [0, 4], [4, 6])
    with pytest.raises(ValueError, match="no gradient"):
        enc.forward_cls_spans(bank.clone().requires_grad_(True), [0, 4], [4, 6])
    with pytest.raises(NotImplementedError):
        enc.forward_cls_spans(PackedAct(bank.to(torch.bfloat16), (1, 40, 32)), [0], [4])
    for starts, lens in (([0, 36], [4, 6]), ([-1, 4], [4, 6]), ([40], [1])):
        with pytest.raises(ValueError, match="outside the bank"):
            enc.forward_cls_spans(bank, starts, lens)
    with pytest.raises(ValueError, match="starts for"):
        enc.forward_cls_spans(bank, [0, 4, 8], [4, 6])
    with pytest.raises(ValueError, match="128"):
        enc.forward_cls_spans(torch.randn(200, 32), [0, 4], [4, 128])
    with pytest.raises(ValueError, match="relative position index"):
        enc.forward_cls_spans(bank, [0, 4], [4, 33])                      # window_depth 2: the index covers 32 patch tokens
    with pytest.raises(ValueError, match="max_position_tokens"):
        _enc(position_encoding=True, max_position_tokens=6).forward_cls_spans(bank, [0, 4], [4, 6])
    with pytest.raises(ValueError, match="relative_pe_2D"):
        _enc(relative_pe=False, relative_pe_2D=True).forward_cls_spans(bank, [0, 16], [16, 4])
    with pytest.raises(ValueError):
        enc.forward_cls_spans(bank.to(torch.float64), [0], [4])
    for b in (bank, bank.view(10, 4, 32)):                                 # [R, d] or [clips, P, d] viewed as rows; a span may end at R
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            enc.forward_cls_spans(b, [36, 0, 0], [4, 6, 6])
    # the existing entries keep refusing tuples and gather specs
    with pytest.raises(ValueError, match="gather spec"):
        enc.forward_cls_unpadded((bank.view(1, 40, 32), torch.zeros(1, dtype=torch.int64), 1, 1), [4, 6])


def test_from_pairs_refuses_a_ten_crop_bank_and_wraps_a_single_crop_one():
    from lstc_vad_amd.pipeline import ResidentSet
    ds = Namespace(norm_keys=["n0.npy", "n1.npy"], abnorm_keys=["a0.npy"])
    bank = torch.zeros(9, 4, 8)
    with pytest.raises(ValueError, match="ten-crop"):
        ResidentSet.from_pairs(Namespace(crops=10, bank=bank, offsets=np.array([0, 3, 5, 9]), ds=ds))
    rs = ResidentSet.from_pairs(Namespace(crops=1, bank=bank, offsets=np.array([0, 3, 5, 9]), ds=ds))
    assert rs.bank.data_ptr() == bank.data_ptr()                           # no copy
    assert rs.keys == ["n0", "n1", "a0"] and rs.offsets.tolist() == [0, 3, 5] and rs.lens.tolist() == [3, 2, 4]
    assert rs.first_clip("a0.npy") == 5 and rs.n_clips("n1") == 2


def test_resident_sequence_scores_refusals():
    from lstc_vad_amd import scoring
    bank = torch.zeros(6, 4, 32)
    with pytest.raises(ValueError, match=r"ragged=False.*ragged='unpadded'"):
        scoring.resident_sequence_scores(None, None, bank, [(0, 4)], ragged=True)
    with pytest.raises(ValueError, match="unpadded"):
        scoring.resident_sequence_scores(None, None, bank, [(0, 4)], ragged="packed")
    with pytest.raises(ValueError, match="at most 127"):
        scoring.resident_sequence_scores(None, None, torch.zeros(50, 4, 32), [(0, 4), (0, 128)], ragged="unpadded")
    with pytest.raises(ValueError, match="whole clips"):
        scoring.resident_sequence_scores(_enc(), None, bank, [(0, 4), (2, 4)])
    with pytest.raises(ValueError, match="whole clips"):
        scoring.resident_sequence_scores(_enc(), None, bank, [(20, 8)])
    with pytest.raises(ValueError, match=r"\[clips, P, d\]"):
        scoring.resident_sequence_scores(_enc(), None, bank.view(24, 32), [(0, 4)])
    head = torch.nn.Linear(32, 2)
    for ragged in (False, "unpadded"):                                    # valid calls: only the device is wrong
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            scoring.resident_sequence_scores(_enc(), head, bank, [(0, 8), (4, 4), (16, 8)], ragged=ragged)


def test_segment_mean_refuses_before_the_device_matters():
    from lstc_vad_amd import functional as Fn
    with pytest.raises(TypeError):
        Fn.segment_mean(torch.zeros(4, 32), [0], [1])
    with pytest.raises(TypeError):
        Fn.segment_mean(torch.zeros(4, 2, 32), [0, 1], [1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.segment_mean(torch.zeros(4, 2, 32), [0, 1], [1, 2], l2=True)


def test_the_score_board_pools_spans_and_bin_tables(monkeypatch):
    """_ScoreBoard with a resident set: spans go to resident_sequence_scores as registered; UCF tables go through ONE segment_mean
    per flush and come back as spans of the bins bank; ltn_sequence_scores is not called."""
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd import pipeline
    seen = []

    def fake_scores(enc, head, bank, spans, **kw):
        seen.append((tuple(bank.shape), list(spans), kw))
        return torch.arange(len(spans), dtype=torch.float32)

    def fake_mean(bank, first, count, l2=False):
        seen.append(("mean", list(first), list(count), l2))
        return torch.zeros(len(first), bank.shape[1], bank.shape[2])
    monkeypatch.setattr(pipeline.scoring, "resident_sequence_scores", fake_scores)
    monkeypatch.setattr(pipeline.scoring, "ltn_sequence_scores", lambda *a, **k: pytest.fail("host route called"))
    monkeypatch.setattr(Fn, "segment_mean", fake_mean)
    rs = pipeline.ResidentSet(torch.zeros(10, 4, 8), [0, 6], [6, 4], ["a", "b"])
    board = pipeline._ScoreBoard(None, None, "cpu", 0, 1, None, 100, None, "unpadded", rs, classifier_head=False)
    board.add_spans(0, 2, lambda: [(0, 12), (12, 12)], lambda v: v.tolist())
    board.add_spans(1, 1, lambda: [(24, 16)], lambda v: v.tolist())
    assert board.results() == [[0.0, 1.0], [2.0]]
    assert seen == [((10, 4, 8), [(0, 12), (12, 12), (24, 16)], {"ragged": "unpadded", "classifier_head": False})]
    seen.clear()
    board = pipeline._ScoreBoard(None, None, "cpu", 0, 1, None, 100, None, False, rs, ucf=dict(part_len=3, rewindow=True, l2=True))
    t0, t1 = (list(range(32)), [1] * 32), (list(range(40, 72)), [2] * 32)
    board.add_bins(0, 11, lambda: t0, lambda v: len(v))
    board.add_bins(1, 11, lambda: t1, lambda v: len(v))
    assert board.results() == [11, 11]
    assert seen[0] == ("mean", t0[0] + t1[0], t0[1] + t1[1], True) and len(seen) == 2
    shape, spans, kw = seen[1]
    assert shape == (64, 4, 8) and kw == {"ragged": False, "classifier_head": True}
    assert spans == pipeline.scoring.ucf_bin_spans(3, True, 4, 0) + pipeline.scoring.ucf_bin_spans(3, True, 4, 32)


# ---------------------------------------------------------------------------------------------------- 4. command line
def test_resident_eval_flag_parses_on_every_script():
    from lstc_vad_amd import cli
    scripts = list(cli._FLAGS)
    assert set(cli.SCRIPTS) <= set(scripts) and any(s.startswith("evaluation") for s in scripts) and \
        any(s.startswith("pseudo_labels_generator") for s in scripts)
    for script in scripts:
        p = cli.build_parser(script)
        assert p.parse_args([]).resident_eval is False, script
        assert p.parse_args(["--resident_eval"]).resident_eval is True, script
        assert cli.complete_args(script, Namespace(batch_size=2)).resident_eval is False, script     # a caller-built namespace: the default
        assert cli.complete_args(script, Namespace(resident_eval=True)).resident_eval is True, script
        argv = cli.namespace_to_argv(script, p.parse_args(["--resident_eval"]))
        assert "--resident_eval" in argv and cli.complete_args(script, argv=argv).resident_eval is True, script   # a rank's command line
        assert "--resident_eval" not in cli.namespace_to_argv(script, p.parse_args([])), script
    assert cli._resident_set(Namespace(resident_eval=False), None, None, None, 16, False) is None      # off: nothing is touched
