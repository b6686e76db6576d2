"""Unpadded batches above 128 tokens, host side (no GPU): the launch groups of a layout, the 512-token limit and its refusals, the
chunker's probabilities cap, the ``ragged="unpadded_long"`` value and the two new entry points in the header and the binding."""
import ctypes as C
import os
import re

import pytest
import torch

import util_ragged as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enc(window_depth=32, **extra):
    from lstc_vad_amd.models import Encoder
    return Encoder(**R.encoder_kw(window_depth, **extra))


# ---------------------------------------------------------------------------------------------------- launch groups
def test_launch_groups_of_mixed_short_and_long_layouts():
    from lstc_vad_amd.functional import UNPADDED_LONG_MAX_TOKENS, UNPADDED_MAX_TOKENS, unpadded_layout
    assert (UNPADDED_MAX_TOKENS, UNPADDED_LONG_MAX_TOKENS) == (128, 512)
    # mixed: S = 129, 2, 512, 160, 128, 32 -> the sequences of at most 128 tokens, then the rest, each with its own longest S
    mixed = unpadded_layout([128, 1, 511, 159, 127, 31], max_tokens=512)
    assert mixed.S_max == 512 and mixed.launch_groups() == [(128, [1, 4, 5]), (512, [0, 2, 3])]
    assert mixed.launch_groups(buckets=True) == mixed.launch_groups()          # above 128 tokens the tile buckets do not apply
    # all long: one group through an id list, S = its longest
    assert unpadded_layout([200, 128, 300], max_tokens=512).launch_groups() == [(301, [0, 1, 2])]
    assert unpadded_layout([128], max_tokens=512).launch_groups() == [(129, [0])]
    # all short: exactly what the layout yields at the default limit, whatever limit was asked for
    for lens in ([63, 1, 127, 15], [5, 5, 5]):
        a, b = unpadded_layout(lens, max_tokens=512), unpadded_layout(lens)
        assert a.launch_groups() == b.launch_groups() == [(max(lens) + 1, None)]
        assert a.launch_groups(buckets=True) == b.launch_groups(buckets=True)
        assert (a.row0, a.in0, a.prob0(2), a.buckets) == (b.row0, b.in0, b.prob0(2), b.buckets)
    assert unpadded_layout([63, 1, 127, 15]).launch_groups(buckets=True) == [(16, [1, 3]), (64, [0]), (128, [2])]
    lay = unpadded_layout([511, 300], max_tokens=512)
    assert lay.prob0(16) == [0, 16 * 512 * 512, 16 * (512 * 512 + 301 * 301)] and lay.row0 == [0, 512, 813]


# ---------------------------------------------------------------------------------------------------- limits and refusals
def test_the_limits_named_in_the_refusals():
    from lstc_vad_amd.functional import unpadded_layout
    assert unpadded_layout([511], max_tokens=512).S_max == 512
    with pytest.raises(ValueError, match="512"):
        unpadded_layout([5, 512], max_tokens=512)                 # 513 tokens
    with pytest.raises(ValueError, match="512"):
        unpadded_layout([5], max_tokens=600)
    with pytest.raises(ValueError, match="128"):
        unpadded_layout([5, 128])                                 # the default keeps its limit
    with pytest.raises(ValueError, match="300"):
        unpadded_layout([5, 300], max_tokens=300)                 # any limit up to 512 holds as given


def test_encoder_refusals_above_128_tokens_come_before_the_device_check():
    enc = _enc()
    x = torch.randn(134, 32)
    for fn in (enc.forward_unpadded, enc.forward_cls_unpadded):
        with pytest.raises(ValueError, match="128"):
            fn(x, [4, 130])                                        # the default limit stays
        with pytest.raises(ValueError, match="512"):
            fn(torch.randn(516, 32), [4, 512], max_tokens=512)     # 513 tokens
        with pytest.raises(ValueError, match="512"):
            fn(x, [4, 130], max_tokens=600)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, [4, 130], max_tokens=512)                        # everything in order: only the device is wrong
    with pytest.raises(ValueError, match="relative position index"):
        _enc(8).forward_cls_unpadded(x, [4, 130], max_tokens=512)   # window_depth 8: the index covers 128 patch tokens
    with pytest.raises(ValueError, match="max_position_tokens"):
        _enc(position_encoding=True, max_position_tokens=128).forward_unpadded(x, [4, 130], max_tokens=512)
    odd = _enc(d_k=24, d_v=16)
    with pytest.raises(ValueError, match="multiples of 16"):
        odd.forward_unpadded(x, [4, 130], max_tokens=512)
    with pytest.raises(ValueError, match="multiples of 16"):
        _enc(d_k=16, d_v=8).forward_cls_unpadded(x, [4, 130], max_tokens=512)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        odd.forward_unpadded(x[:104], [4, 100], max_tokens=512)    # no sequence above 128 tokens: any d_k
    bank = torch.randn(600, 32)
    with pytest.raises(ValueError, match="128"):
        enc.forward_cls_spans(bank, [0, 10], [4, 130])
    with pytest.raises(ValueError, match="512"):
        enc.forward_cls_spans(bank, [0, 10], [4, 512], max_tokens=512)
    with pytest.raises(ValueError, match="multiples of 16"):
        odd.forward_cls_spans(bank, [0, 10], [4, 130], max_tokens=512)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.forward_cls_spans(bank, [0, 10], [4, 130], max_tokens=512)


# ---------------------------------------------------------------------------------------------------- the chunker
def test_chunks_close_before_the_probabilities_cap():
    from lstc_vad_amd.scoring import UNPADDED_MAX_PROBS, unpadded_batches, unpadded_chunks
    assert UNPADDED_MAX_PROBS == 2 ** 32 - 1
    lens = [9, 9, 9, 19, 9, 9]                # S = 10, 10, 10, 20, 10, 10: 2 heads -> 200, 200, 200, 800, 200, 200 floats
    assert unpadded_chunks(lens, 100, 10 ** 6) == [[0, 1, 2, 3, 4, 5]]
    assert unpadded_chunks(lens, 100, 10 ** 6, 2, 600) == [[0, 1, 2], [3], [4, 5]]          # a single sequence always fits
    assert unpadded_chunks(lens, 100, 10 ** 6, 2, 1000) == [[0, 1, 2], [3, 4], [5]]
    assert unpadded_chunks(lens, 100, 10 ** 6, 2, 1001) == [[0, 1, 2], [3, 4], [5]]
    assert unpadded_chunks(lens, 100, 10 ** 6, 2, 1799) == [[0, 1, 2, 3, 4], [5]]
    assert unpadded_chunks(lens, 100, 10 ** 6, 2, 1800) == [[0, 1, 2, 3, 4, 5]]
    assert unpadded_chunks(lens, 2, 10 ** 6, 2, 1800) == [[0, 1], [2, 3], [4, 5]]           # the other caps still hold
    assert unpadded_chunks(lens, 100, 35, 2, 1800) == [[0, 1, 2], [3, 4], [5]]
    assert unpadded_chunks(lens, 100, 10 ** 6, 0, 1) == [[0, 1, 2, 3, 4, 5]]                # heads = 0: no cap
    # at 512 tokens and 16 heads the default cap is 1 023 sequences
    assert [len(c) for c in unpadded_chunks([511] * 2050, 4096, 10 ** 9, 16)] == [1023, 1023, 4]
    seqs = [torch.zeros(v, 4) for v in lens]
    assert [b[0] for b in unpadded_batches(seqs, 100, 10 ** 6, heads=2, max_probs=600)] == [[0, 1, 2], [3], [4, 5]]
    long = [torch.zeros(v, 4) for v in (130, 5, 511)]
    got = unpadded_batches(long, max_tokens=512)
    assert [b[0] for b in got] == [[0, 1, 2]] and got[0][1].shape == (646, 4) and got[0][2] == [130, 5, 511]
    with pytest.raises(ValueError, match="ragged=True"):
        unpadded_batches(long)
    with pytest.raises(ValueError, match="511"):
        unpadded_batches(long + [torch.zeros(512, 4)], max_tokens=512)


# ---------------------------------------------------------------------------------------------------- the ragged value
def test_unpadded_long_takes_what_unpadded_refuses():
    from lstc_vad_amd import scoring
    from lstc_vad_amd.models import Classifier
    enc, head = _enc(), Classifier(32, 0.0)
    seqs = [torch.randn(16, 32), torch.randn(128, 32)]              # 128 patch tokens: 129 with the CLS token
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.ltn_sequence_scores(enc, head, seqs, ragged="unpadded_long")          # only the device is wrong
    with pytest.raises(ValueError, match="ragged=True"):
        scoring.ltn_sequence_scores(enc, head, seqs, ragged="unpadded")
    with pytest.raises(ValueError, match="ragged=True"):
        scoring.ltn_sequence_scores(None, None, seqs + [torch.randn(512, 32)], ragged="unpadded_long")
    with pytest.raises(ValueError, match="unpadded"):
        scoring.ltn_sequence_scores(None, None, seqs[:1], ragged="unpadded_wide")
    bank = torch.randn(40, 16, 32)
    spans = [(0, 16), (16, 128)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scoring.resident_sequence_scores(enc, head, bank, spans, ragged="unpadded_long")
    with pytest.raises(ValueError, match="at most 127"):
        scoring.resident_sequence_scores(enc, head, bank, spans, ragged="unpadded")
    with pytest.raises(ValueError, match="at most 511"):
        scoring.resident_sequence_scores(None, None, bank, [(0, 512)], ragged="unpadded_long")
    with pytest.raises(ValueError, match="unpadded"):
        scoring.resident_sequence_scores(None, None, bank, spans, ragged="unpadded_wide")


# ---------------------------------------------------------------------------------------------------- header and binding
def test_header_declares_and_the_binding_has_the_long_entry_points():
    from lstc_vad_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lstc_hip.h")).read()
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("lstc_attn_var_long_fwd", "lstc_attn_var_long_bwd"):
        assert re.search(r"\bint " + name + r"\(const LstcAttnDesc\* d, const LstcSeqs\* s, void\* stream\);", hdr), name
        assert name in _lib.EXPORTS and hasattr(raw, name)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 3
        assert fn(None, None, None) == -1                        # LSTC_E_NULL, before anything touches a device
    assert lib.lstc_version() == 112 and "#define LSTC_VERSION 112" in hdr
    assert C.sizeof(_lib.Seqs) == 40
