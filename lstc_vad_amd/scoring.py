"""Video scoring recipes of the reference's evaluation loops and pseudo-label generators, batched for the device.

The reference pushes ONE part of one video through the model per launch sequence (batch 1, e.g.
Test/evaluation_shanghaitech_ubnormal.py:75-92).  Sequences are independent, so here every part of a video that has
the same length goes through the encoder as one batch - and ``pipeline`` pools the parts of many videos into those
batches (``ltn_sequence_scores``; ``Encoder.forward_cls``: only the CLS row is computed in the last layer); results
are identical row by row (``test_full_width_scores_match_oracle`` checks batch invariance).

Recipes (all return per-part scores plus the ``(beg, end)`` clip ranges they stand for):

* ``stn_clip_scores``      - STN: one score per clip (Train/pseudo_labels_generator_spatio.py:79-86);
* ``ltn_part_scores``      - LTN on consecutive parts of ``part_len`` clips; the short tail part is either fed as a
                             shorter sequence (``tail='short'``, Train/pseudo_labels_generator_temporal.py:120-141) or
                             re-windowed to the video's last ``part_len`` clips (``tail='rewindow'``,
                             Test/evaluation_shanghaitech_ubnormal.py:83-84 and the in-loop evaluation
                             Train/temporal_transformer_shanghaitech.py:176-179) - including the reference's behaviour
                             for videos shorter than one part (a negative slice start);
* ``ltn_ucf_bin_scores``   - UCF: clips averaged into 32 bins (``np.linspace(0, n_frames // segment_len, 33)``), parts
                             of ``part_len`` bins, optional L2 normalisation (Test/evaluation_UCF.py:54-77 normalises,
                             Train/pseudo_labels_generator_temporal.py:73-99 does not).

The same parts on an HBM-resident bank (``pipeline.ResidentSet``) are not cut out but described: ``part_spans``, ``ucf_bin_table`` and
``ucf_bin_spans`` give every part as a span of bank rows (pure Python), ``resident_sequence_scores`` scores a pool of spans.
"""
from __future__ import annotations

import numpy as np
import torch


def part_ranges(n: int, part_len: int):
    """[(beg, end)] of consecutive parts; the last one ends at ``n`` and may be shorter."""
    n_parts = n // part_len + (1 if (n // part_len) * part_len < n else 0)
    return [(i * part_len, n if i == n_parts - 1 else (i + 1) * part_len) for i in range(n_parts)]


def ragged_batches(seqs, max_batch=4096):
    """The batches of ``ltn_sequence_scores(ragged=True)``: consecutive chunks of up to ``max_batch`` sequences of ANY lengths, each
    padded to the longest sequence of the whole call -> [(ids, x [n, T_max, d], lengths)] with ``ids`` the positions in ``seqs``
    (input order), ``x[k, :lengths[k]] = seqs[ids[k]]`` and zeros behind (the content of the padding is free: the encoder never
    reads it).  Pure torch; runs on CPU tensors."""
    t_max = max(s.shape[0] for s in seqs)
    d = seqs[0].shape[1]
    batches = []
    for c in range(0, len(seqs), max_batch):
        ids = list(range(c, min(c + max_batch, len(seqs))))
        x = seqs[0].new_zeros((len(ids), t_max, d))
        lengths = [int(seqs[i].shape[0]) for i in ids]
        for k, i in enumerate(ids):
            x[k, :lengths[k]] = seqs[i]
        batches.append((ids, x, lengths))
    return batches


UNPADDED_ROWS_PER_SEQUENCE = 49      # 3 clips of 16 patches + the CLS token: the longest part of the LTN workloads


UNPADDED_MAX_PROBS = 2 ** 32 - 1     # floats of a chunk's ragged probabilities: their offsets are the 32-bit dropout counters
_UNPADDED_TOKENS = {"unpadded": 128, "unpadded_long": 512}      # ragged value -> longest sequence, CLS token counted


def _unpadded_limit(ragged, lengths, what="sequence"):
    """ValueError where a sequence is beyond the route's limit, before anything is launched -> the limit in tokens."""
    limit = _UNPADDED_TOKENS[ragged]
    for i, v in enumerate(lengths):
        if v + 1 > limit:
            if ragged == "unpadded":
                if what == "span":
                    raise ValueError(f"ragged='unpadded': span {i} has {v} patch tokens, the unpadded route takes at most 127")
                raise ValueError(f"ragged='unpadded': sequence {i} has {v} patch tokens, the unpadded route takes at most 127 "
                                 "(128 tokens with the CLS token); use ragged=True for this pool")
            raise ValueError(f"ragged={ragged!r}: {what} {i} has {v} patch tokens, the route takes at most {limit - 1} ({limit} tokens "
                             "with the CLS token)" + ("; use ragged=True for this pool" if what == "sequence" else ""))
    return limit


def _n_head(enc):
    return int(enc.layer_stack[0].slf_attn.n_head)


def unpadded_batches(seqs, max_batch=4096, max_rows=None, max_tokens=128, heads=0, max_probs=UNPADDED_MAX_PROBS):
    """The batches of ``ltn_sequence_scores(ragged="unpadded")``: consecutive chunks of sequences of ANY lengths, concatenated
    without padding -> [(ids, x [sum of lengths, d], lengths)] with ``ids`` the positions in ``seqs`` (input order) and
    ``x`` the rows of ``seqs[ids[0]]``, ``seqs[ids[1]]``, ... back to back.  A chunk holds up to ``max_batch`` sequences and up to
    ``max_rows`` rows with the CLS tokens counted (default ``49 * max_batch``: a full chunk of 3-clip parts at 16 patches, the
    largest [N * S, d] the grouped path forms on the LTN workloads, so the activations of a chunk stay that size); a single
    sequence always fits.  A sequence above 127 patch tokens (128 with the CLS token, the unpadded attention kernels' tile) raises
    ValueError before anything is launched: score such a pool with ``ragged=True``.  ``max_tokens`` = 512 is the limit of
    ``ragged="unpadded_long"``; ``heads`` > 0 also closes a chunk before its ragged probabilities [heads, S_n, S_n] would pass
    ``max_probs`` floats (``unpadded_chunks``).  Pure torch; runs on CPU tensors."""
    max_rows = UNPADDED_ROWS_PER_SEQUENCE * max_batch if max_rows is None else max_rows
    _unpadded_limit("unpadded_long" if max_tokens > 128 else "unpadded", [int(s.shape[0]) for s in seqs])
    batches = unpadded_chunks([int(s.shape[0]) for s in seqs], max_batch, max_rows, heads, max_probs)
    return [(ids, torch.cat([seqs[i] for i in ids], 0), [int(seqs[i].shape[0]) for i in ids]) for ids in batches]


def unpadded_chunks(lengths, max_batch, max_rows, heads=0, max_probs=UNPADDED_MAX_PROBS):
    """The chunking rule of ``unpadded_batches`` on the lengths alone -> lists of consecutive positions: up to ``max_batch``
    sequences and ``max_rows`` rows (CLS tokens counted) per chunk, a single sequence always fits.  ``heads`` > 0: a chunk also
    closes before its ragged attention probabilities, ``heads * S_n * S_n`` floats per sequence, would pass ``max_probs`` (2^32 - 1:
    an element's offset in that buffer is its 32-bit dropout counter; at 512 tokens and 16 heads that is 1 023 sequences).
    Pure Python."""
    batches, ids, rows, probs = [], [], 0, 0
    for i, v in enumerate(lengths):
        r = int(v) + 1
        pr = heads * r * r
        if ids and (len(ids) >= max_batch or rows + r > max_rows or probs + pr > max_probs):
            batches.append(ids)
            ids, rows, probs = [], 0, 0
        ids.append(i)
        rows += r
        probs += pr
    if ids:
        batches.append(ids)
    return batches


def ltn_sequence_scores(enc, head, seqs, max_batch=4096, ragged=False):
    """seqs: list of [len_i * P, d] tensors (any mix of videos) -> tensor [len(seqs)] of P(abnormal).  Same-length
    sequences share a batch of up to ``max_batch`` rows, so a whole test set is scored in a handful of launch sequences
    that fill the GPU like a training step does.
    ``ragged``: sequences of ALL lengths share batches instead - padded to the longest of the call and scored through
    ``Encoder.forward_cls(x, lengths=...)``, one launch chain per ``max_batch`` sequences rather than one per distinct length;
    every score is what the sequence gets alone (up to float re-association), in input order.
    ``ragged="unpadded"``: sequences of all lengths share batches WITHOUT padding - concatenated (``unpadded_batches``) and scored
    through ``Encoder.forward_cls_unpadded``: one launch chain per chunk that costs the real tokens only.  Sequences of at most
    127 patch tokens; a longer one raises before any launch.
    ``ragged="unpadded_long"``: the same route with sequences of up to 511 patch tokens (``forward_cls_unpadded(...,
    max_tokens=512)``: the key-tiled offset kernels for the sequences above 128 tokens; d_k and d_v multiples of 16)."""
    if isinstance(ragged, str) and ragged not in _UNPADDED_TOKENS:
        raise ValueError(f"ragged: expected False, True, 'unpadded' or 'unpadded_long', got {ragged!r}")
    if isinstance(ragged, str):
        limit = _unpadded_limit(ragged, [int(s.shape[0]) for s in seqs])
        batches = unpadded_batches(seqs, max_batch, max_tokens=limit, heads=_n_head(enc))
        out = torch.empty(len(seqs), device=seqs[0].device, dtype=torch.float32)
        for ids, x, lengths in batches:
            cls = enc.forward_cls_unpadded(x, lengths) if limit == 128 else enc.forward_cls_unpadded(x, lengths, max_tokens=limit)
            out[ids[0]:ids[-1] + 1] = head(cls).view(-1, 2)[:, 1]
        return out
    out = torch.empty(len(seqs), device=seqs[0].device, dtype=torch.float32)
    if ragged:
        for ids, x, lengths in ragged_batches(seqs, max_batch):
            out[ids[0]:ids[-1] + 1] = head(enc.forward_cls(x, lengths=lengths)).view(-1, 2)[:, 1]
        return out
    by_len = {}
    for i, s in enumerate(seqs):
        by_len.setdefault(s.shape[0], []).append(i)
    for ids in by_len.values():
        for c in range(0, len(ids), max_batch):
            chunk = ids[c:c + max_batch]
            x = torch.stack([seqs[i] for i in chunk])
            out[torch.tensor(chunk, device=out.device)] = head(enc.forward_cls(x)).view(-1, 2)[:, 1]
    return out


_ltn_scores = ltn_sequence_scores


def stn_clip_scores(enc, head, feats, classifier_head=False):
    """feats [n_clips, P, d] -> [n_clips, 1].  ``classifier_head``: the generator's ``n_layers == 1`` branch pairs the
    encoder with a Classifier and keeps column 1 (Train/pseudo_labels_generator_spatio.py:81-82)."""
    y = head(enc.forward_cls(feats))
    return y[:, 1] if classifier_head else y


def ltn_part_sequences(feats, part_len, tail="rewindow"):
    """feats [n_clips, P, d] -> (list of [len*P, d] sequences, [(beg, end)])."""
    n, P, d = feats.shape
    ranges = part_ranges(n, part_len)
    seqs = []
    for beg, end in ranges:
        if end - beg < part_len and tail == "rewindow":
            part = feats[end - part_len:end]              # python slice semantics, as upstream (negative start allowed)
        else:
            part = feats[beg:end]
        seqs.append(part.reshape(-1, d))
    return seqs, ranges


def ltn_part_scores(enc, head, feats, part_len, tail="rewindow", ragged=False):
    """feats [n_clips, P, d] -> (scores [n_parts], [(beg, end)]).  ``ragged``: as in ``ltn_sequence_scores``."""
    seqs, ranges = ltn_part_sequences(feats, part_len, tail)
    return ltn_sequence_scores(enc, head, seqs, ragged=ragged), ranges


def ucf_bins(feats, n_frames, segment_len=16, max_clips=32):
    """feats [n_clips, P, d] -> (bins [32, P, d], r [33]): bin i is the mean of clips r[i]:r[i+1] (or clip r[i] when the
    range is empty)."""
    n_clips = n_frames // segment_len
    r = np.linspace(0, n_clips, max_clips + 1, dtype=np.int32)
    rows = []
    for i in range(max_clips):
        rows.append(feats[int(r[i])] if r[i] == r[i + 1] else feats[int(r[i]):int(r[i + 1])].mean(dim=0))
    return torch.stack(rows), r


def ucf_bin_ranges(part_len, rewindow=True, max_clips=32):
    """[(beg, end)] in bin units of the parts a UCF video is scored in - a function of the flags alone (every video has 32
    bins), so a rank that does not own a video still knows how many scores it contributes (pipeline, sharded passes)."""
    ranges = []
    for beg, end in part_ranges(max_clips, part_len):
        if rewindow and end - beg < part_len:
            beg = end - part_len
        ranges.append((beg, end))
    return ranges


def ucf_bin_edges(n_frames, segment_len=16, max_clips=32):
    """r [33]: bin i covers clips r[i]:r[i+1] (Test/evaluation_UCF.py:54)."""
    return np.linspace(0, n_frames // segment_len, max_clips + 1, dtype=np.int32)


def ltn_ucf_bin_sequences(feats, n_frames, part_len, segment_len=16, normalize=True, rewindow=True, max_clips=32):
    """-> (sequences, [(beg, end)] in bin units, r).  ``rewindow`` moves a short tail part back so that it spans
    ``part_len`` bins (Test/evaluation_UCF.py:66-67 - there ``beg`` itself moves, so the frames it labels move too)."""
    bins, r = ucf_bins(feats, n_frames, segment_len, max_clips)
    d = bins.shape[-1]
    ranges = ucf_bin_ranges(part_len, rewindow, max_clips)
    seqs = [bins[b:e].reshape(-1, d) for b, e in ranges]
    if normalize:
        seqs = [torch.nn.functional.normalize(s, p=2, dim=-1) for s in seqs]
    return seqs, ranges, r


def ltn_ucf_bin_scores(enc, head, feats, n_frames, part_len, segment_len=16, normalize=True, rewindow=True, max_clips=32,
                       ragged=False):
    seqs, ranges, r = ltn_ucf_bin_sequences(feats, n_frames, part_len, segment_len, normalize, rewindow, max_clips)
    return ltn_sequence_scores(enc, head, seqs, ragged=ragged), ranges, r


# -- spans of an HBM-resident bank: the same parts, described instead of cut out ---------------------------------------------------

def part_spans(n, part_len, n_patch=1, tail="rewindow", first_clip=0):
    """``ltn_part_sequences`` of a video of ``n`` clips that lies in a bank [clips, n_patch, d] from clip ``first_clip``, as spans
    of the bank's ROWS -> ([(first_row, n_tokens)], [(beg, end)]): span k holds the rows ``ltn_part_sequences`` stacks into sequence
    k.  ``tail='rewindow'`` moves a short tail part back with the slice semantics of the reference (``feats[end - part_len:end]``: a
    video shorter than one part yields the clips its negative slice start selects).  ``part_len=1`` are the clips of an STN.  Pure
    Python."""
    ranges = part_ranges(n, part_len)
    spans = []
    for beg, end in ranges:
        b, e = beg, end
        if end - beg < part_len and tail == "rewindow":
            b, e, _ = slice(end - part_len, end).indices(n)
        spans.append(((first_clip + b) * n_patch, (e - b) * n_patch))
    return spans, ranges


def ucf_bin_table(n_frames, segment_len=16, max_clips=32, first_clip=0, n_clips=None):
    """``ucf_bins`` as a table for ``functional.segment_mean`` -> (first [32], count [32]) in clips of the bank: bin i is the mean of
    ``count[i]`` clips from ``first[i]``; an empty bin (``r[i] == r[i + 1]``) is clip ``r[i]`` alone, a count of 1.  ``n_clips``: the
    clips the video really has - a bin ends there, as the host route's slices do.  Pure Python."""
    r = ucf_bin_edges(n_frames, segment_len, max_clips)
    first, count = [], []
    for i in range(max_clips):
        a, b = int(r[i]), int(r[i + 1])
        if n_clips is not None:
            if a >= n_clips:
                raise ValueError(f"ucf_bin_table: bin {i} starts at clip {a}, the video has {n_clips}")
            b = min(b, n_clips)
        first.append(first_clip + a)
        count.append(max(b - a, 1))
    return first, count


def ucf_bin_spans(part_len, rewindow=True, n_patch=1, first_bin=0, max_clips=32):
    """The parts of ``ucf_bin_ranges`` as spans of the rows of a bins bank [bins, n_patch, d] in which the video's 32 bins lie from
    bin ``first_bin`` -> [(first_row, n_tokens)].  Pure Python."""
    return [((first_bin + b) * n_patch, (e - b) * n_patch) for b, e in ucf_bin_ranges(part_len, rewindow, max_clips)]


def resident_sequence_scores(enc, head, bank, spans, max_batch=4096, ragged=False, classifier_head=True):
    """``ltn_sequence_scores`` on sequences that are SPANS ``(first_row, n_tokens)`` of the rows of an HBM-resident ``bank``
    ([clips, P, d] float32 on the device, or [rows, d]) -> tensor [len(spans)], input order.  No sequence is cut out or copied.
    ``ragged=False``: spans of the same length share a batch of up to ``max_batch`` and go through the encoder's gather spec
    (``enc.forward_cls((bank, clip_idx, N, Lc))``: the fixed-layout kernels; the spans must be whole clips of a 3-D bank); where
    that entry refuses (d % 4, an input LayerNorm) the group is gathered (``functional.gather_rows``) and scored by ``forward_cls``.
    ``ragged="unpadded"``: spans of all lengths share chunks (``unpadded_chunks``, the rule of ``unpadded_batches``) scored by
    ``Encoder.forward_cls_spans``; ``ragged="unpadded_long"``: the same with spans of up to 511 patch tokens (``max_tokens=512``).
    ``ragged=True`` (padded batches) does not exist on a bank.  ``classifier_head``: P(abnormal) is column 1 of the head's two
    outputs (False: a Regressor's single output)."""
    if ragged is True or (ragged and ragged not in _UNPADDED_TOKENS):
        raise ValueError(f"ragged={ragged!r}: a resident bank is scored with ragged=False (same-length groups through the gather "
                         "spec) or ragged='unpadded' (spans of all lengths, forward_cls_spans)")
    spans = [(int(r), int(t)) for r, t in spans]
    take = (lambda y: y.view(-1, 2)[:, 1]) if classifier_head else (lambda y: y.reshape(-1))
    out = torch.empty(len(spans), device=bank.device, dtype=torch.float32)
    if ragged:
        limit = _unpadded_limit(ragged, [t for _, t in spans], "span")
        for ids in unpadded_chunks([t for _, t in spans], max_batch, UNPADDED_ROWS_PER_SEQUENCE * max_batch, _n_head(enc)):
            starts, lens = [spans[i][0] for i in ids], [spans[i][1] for i in ids]
            cls = enc.forward_cls_spans(bank, starts, lens) if limit == 128 else enc.forward_cls_spans(bank, starts, lens, max_tokens=limit)
            out[ids[0]:ids[-1] + 1] = take(head(cls))
        return out
    if bank.dim() != 3:
        raise ValueError(f"ragged=False scores whole clips of a bank [clips, P, d], got {tuple(bank.shape)}; use ragged='unpadded'")
    clips, P, d = bank.shape
    by_len = {}
    for i, (r, t) in enumerate(spans):
        if r % P or t % P or t < P or r < 0 or r + t > clips * P:
            raise ValueError(f"ragged=False: span {i} = rows [{r}, {r + t}) is not a run of whole clips of the bank "
                             f"[{clips}, {P}, {d}]; use ragged='unpadded'")
        by_len.setdefault(t // P, []).append(i)
    spec = d % 4 == 0 and not enc.input_layerNorm
    if not spec and (P * d) % 4:
        raise ValueError(f"ragged=False: clips of {P} x {d} floats fit neither the gather spec nor gather_rows; use ragged='unpadded'")
    if not bank.is_cuda:
        raise RuntimeError("lstc_vad_amd: tensor is not on a HIP device; the hot path is HIP-only (no CPU fallback)")
    from . import functional as Fn
    for Lc, ids in by_len.items():
        for c in range(0, len(ids), max_batch):
            chunk = ids[c:c + max_batch]
            first = np.asarray([spans[i][0] // P for i in chunk], dtype=np.int64)
            idx = torch.from_numpy((first[:, None] + np.arange(Lc, dtype=np.int64)[None, :]).reshape(-1)).to(bank.device)
            if spec:
                cls = enc.forward_cls((bank, idx, len(chunk), Lc))
            else:
                cls = enc.forward_cls(Fn.gather_rows(bank, idx).view(len(chunk), Lc * P, d))
            out[torch.tensor(chunk, device=out.device)] = take(head(cls))
    return out


def frame_scores_sht(scores, ranges, anno, segment_len=16):
    """Expand per-part scores to frame level and cut the matching labels (…ubnormal.py:89-91)."""
    s = np.concatenate([np.full((e - b) * segment_len, float(v), np.float32) for v, (b, e) in zip(scores, ranges)])
    n = ranges[-1][1] * segment_len
    return s, np.asarray(anno[:n])


def frame_scores_ucf(scores, ranges, r, anno, segment_len=16):
    """Test/evaluation_UCF.py:82-85: part (beg, end) covers frames r[beg]*seg : r[end]*seg."""
    s, l = [], []
    for v, (b, e) in zip(scores, ranges):
        s.append(np.full(int(r[e] - r[b]) * segment_len, float(v), np.float32))
        l.append(np.asarray(anno[int(r[b]) * segment_len:int(r[e]) * segment_len]))
    return np.concatenate(s), np.concatenate(l)
