"""File-level stages around the training step: pseudo-label generation and frame-level AUC evaluation on feature
archives, with the reference's file formats.

* ``generate_pseudo_labels``  - Train/pseudo_labels_generator_spatio.py:67-90 and
  Train/pseudo_labels_generator_temporal.py:66-146.  Output: ``{"<video>.npy": float32 [n, 1]}`` written with
  ``np.save`` (a pickled dict; read back with ``np.load(..., allow_pickle=True).tolist()``, utils/load_dataset.py:20),
  scores at or below ``threshold`` zeroed.  STN: one row per clip.  LTN (SHT / UBnormal): one row per clip, the part's
  score repeated.  LTN (UCF): 32 rows - one per bin.
* ``evaluate_auc``            - Test/evaluation_shanghaitech_ubnormal.py:69-96, Test/evaluation_UCF.py:47-88 and the
  in-loop evaluation of the train scripts: frame-level ROC-AUC over the whole test list.

Both stages keep features on the device and pool the parts of many videos (``pool_sequences``, default 2048 - the
sequence count of a headline training step) into each launch sequence (``lstc_vad_amd.scoring``); the reference scores
one part per launch.

**Sharded over ranks (round 5).**  Videos are independent, so under N ranks (``rank`` / ``world``, default: the initialised
process group) rank r scores the videos ``i % N == r`` of the list and one zero-padded SUM all-reduce of the flat
per-sequence score vector hands every rank all scores - the exchange the training loss uses for its bag maxima.  Every rank
walks the whole list on the host (shapes, masks, list lines: a video's sequence count follows from its clip count and the
flags alone), but uploads and scores only its own videos; AUC, label files and therefore the checkpoint decisions are
computed from the complete vector on every rank and are bit-identical to a single-rank pass in fp32 mode (x + 0 = x, and a
sequence's score does not depend on what shares its batch).  In the reference this evaluation runs on GPU 0 every
``inter_epoch`` epochs over all test AND train videos (Train/temporal_transformer_shanghaitech.py:151-229) while the other
GPUs idle.

**Resident sets.**  ``resident=ResidentSet`` on any pass: the videos were uploaded once into one HBM bank, a pass registers every
part of every video as a SPAN of bank rows (``scoring.part_spans``, ``ucf_bin_table`` / ``ucf_bin_spans``) and the pool is scored
from the bank (``scoring.resident_sequence_scores``) - no archive read, no upload and no sequence cut out per pass; the UCF bins of
a pool come from one ``lstc_segment_mean`` launch.  Lists, masks, ``finish`` closures, thresholds, AUC and sharding are the same code.

**AUC on the device.**  ``device_auc=`` on the two AUC passes: every frame's score is one flat row's score, so the frame-level AUC is
a weighted pair count over the rows (``metrics.roc_auc_weighted``).  ``AucWeights`` turns the ``finish`` closures of a pass into the
per-row counts of label-1 / label-0 frames once; an evaluation is then ``lstc_auc_weighted`` on the flat device vector and 40 bytes
come back instead of the scores.

**Detection report on the device.**  ``device_auc=ReportWeights(group_of=, thresholds=)``: the same pass, the same return value, and
``weights.report`` (``metrics.DetectionReport``) holds AUC, AP, PR-AUC, the confusion counts at the thresholds (FAR, precision,
recall, ...) and the score sums (GAP, RMSE) of all frames and, with ``group_of`` (``ucf_class`` for UCF-Crime), of every class of
videos - ``eval_each_part``'s table.  ``lstc_det_report`` counts, for every row, the label-1 / label-0 frames at scores >= and ==
its own over the rows of its class; everything else follows from those integers (``metrics.detection_report_weighted``).
"""
from __future__ import annotations

import numpy as np
import torch

from . import scoring
from .archive import FeatureArchive
from .load_dataset import UBnormal_test, UCF_test, UCF_train, _ucf_line, shanghaitech_test, test_list
from .metrics import roc_auc


def _train_keys(dataset: str, training_txt: str):
    for line in open(training_txt, "r").readlines():
        if dataset == "UCF":
            yield line, line.strip().split(" ")[0].split("/")[-1].split(".")[0]
        else:                                   # SHT "name,label", UBnormal "name,..."
            yield line, line.strip().split(",")[0]


def _dev(a, device, n_patch=None):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    if n_patch is not None and t.dim() == 3:
        t = t[:, :n_patch, :]
    return t.to(device).contiguous()


def _plain_key(key):
    return key[:-4] if key.endswith(".npy") else key


class ResidentSet:
    """The videos of a test or label list in ONE ``[total_clips, P, d]`` float32 bank on the device: ``keys`` (list order, without
    ``.npy``), ``lens`` (clips of every video) and ``offsets`` (first clip of a video in the bank; -1 where this rank holds none).
    Built once, then handed to ``evaluate_auc`` / ``evaluate_train_auc`` / ``generate_pseudo_labels`` as ``resident=``: those passes
    read no archive and upload nothing.  ``n_patch`` / ``view`` say how a stored array becomes clips, as the host-fed pass of the
    same data does: ``view=False`` a 3-D array [n, P_stored, d] cut to its first ``n_patch`` patches (None: all - the STN label
    generator), ``view=True`` any array viewed ``[-1, n_patch, d]`` (the UCF routes).  ``owns(i)``: upload only the videos this rank
    scores (``i % world == rank``); the others keep their clip counts, which every rank needs."""

    def __init__(self, bank, offsets, lens, keys):
        self.bank, self.keys = bank, [_plain_key(k) for k in keys]
        self.offsets, self.lens = np.asarray(offsets, dtype=np.int64), np.asarray(lens, dtype=np.int64)
        self._at = {k: i for i, k in enumerate(self.keys)}

    @staticmethod
    def clip_shape(shape, n_patch=None, view=False):
        """(clips, P, d) a stored array of ``shape`` contributes."""
        shape = tuple(int(v) for v in shape)
        if view or len(shape) != 3:
            P = int(n_patch or 1)
            return int(np.prod(shape)) // (P * shape[-1]), P, shape[-1]
        return shape[0], (shape[1] if n_patch is None else min(int(n_patch), shape[1])), shape[2]

    @staticmethod
    def bytes(shapes, n_patch=None, view=False, owns=None) -> int:
        """Bytes of the bank (fp32) of videos with the stored ``shapes`` (``archive_shapes``), from the shapes alone."""
        return int(sum(4 * int(np.prod(ResidentSet.clip_shape(shp, n_patch, view)))
                       for i, shp in enumerate(shapes) if owns is None or owns(i)))

    @staticmethod
    def archive_shapes(path, keys):
        with FeatureArchive(path) as arc:
            return [tuple(arc.shape(_plain_key(k) + ".npy")) for k in keys]

    @classmethod
    def _build(cls, shapes, fetch, keys, device, n_patch, view, owns):
        cs = [cls.clip_shape(shp, n_patch, view) for shp in shapes]
        if not cs:
            raise ValueError("ResidentSet: no videos")
        if any(c[1:] != cs[0][1:] for c in cs):
            raise ValueError("ResidentSet: the videos do not share one clip shape [P, d]")
        mine = [owns is None or bool(owns(i)) for i in range(len(cs))]
        lens = [c[0] for c in cs]
        offsets, tot = [], 0
        for n, m in zip(lens, mine):
            offsets.append(tot if m else -1)
            tot += n if m else 0
        _, P, d = cs[0]
        bank = torch.empty((tot, P, d), dtype=torch.float32, device=device)
        for i, (o, n, m) in enumerate(zip(offsets, lens, mine)):      # one staged copy per video: only the video in flight is on the host
            if not m or n == 0:
                continue
            a = np.asarray(fetch(i))
            a = a.reshape(-1, P, d) if (view or a.ndim != 3) else a[:, :P, :]
            a = np.ascontiguousarray(a, dtype=np.float32)
            if not a.flags.writeable:                 # a memory-mapped member of a directory archive: read it (torch wants writable memory)
                a = a.copy()
            bank[o:o + n].copy_(torch.from_numpy(a))
        return cls(bank, offsets, lens, keys)

    @classmethod
    def from_arrays(cls, arrays, device, keys=None, n_patch=None, view=False, owns=None):
        """From host arrays, one per video (``keys`` default to their positions)."""
        arrays = list(arrays)
        keys = [str(i) for i in range(len(arrays))] if keys is None else list(keys)
        if len(keys) != len(arrays):
            raise ValueError(f"ResidentSet: {len(keys)} keys for {len(arrays)} videos")
        return cls._build([np.shape(a) for a in arrays], lambda i: arrays[i], keys, device, n_patch, view, owns)

    @classmethod
    def from_archive(cls, path, keys, device, n_patch=None, view=False, owns=None):
        """From a feature archive: a shape pass, then one read and one staged copy per video."""
        keys = [_plain_key(k) for k in keys]
        with FeatureArchive(path) as arc:
            shapes = [tuple(arc.shape(k + ".npy")) for k in keys]
            return cls._build(shapes, lambda i: arc[keys[i] + ".npy"], keys, device, n_patch, view, owns)

    @classmethod
    def from_pairs(cls, pairs):
        """Wrap the bank of a ``load_dataset.ResidentPairs`` - the training set already in HBM - without a copy: for
        ``evaluate_train_auc``.  Single-crop banks only."""
        if getattr(pairs, "crops", 1) != 1:
            raise ValueError("ResidentSet.from_pairs: a ten-crop bank holds ten crops per clip; only single-crop banks are scored "
                             "from HBM")
        bank = pairs.bank if pairs.bank.dim() == 3 else pairs.bank.view(pairs.bank.shape[0], 1, -1)
        offsets = np.asarray(pairs.offsets, dtype=np.int64)
        return cls(bank, offsets[:-1], np.diff(offsets), list(pairs.ds.norm_keys) + list(pairs.ds.abnorm_keys))

    def __len__(self):
        return len(self.keys)

    def n_clips(self, key):
        return int(self.lens[self._at[_plain_key(key)]])

    def first_clip(self, key):
        """First clip of the video in the bank; ValueError where this rank did not upload it."""
        o = int(self.offsets[self._at[_plain_key(key)]])
        if o < 0:
            raise ValueError(f"ResidentSet: video {key!r} was not uploaded on this rank (owns)")
        return o

    def patches(self, n_patch, what):
        if self.bank.shape[1] != n_patch:
            raise ValueError(f"{what}: the resident bank holds {self.bank.shape[1]} patches per clip, the pass scores n_patch = {n_patch}")
        return int(n_patch)


def _ranks(rank, world, group):
    """(rank, world) of a pass: explicit arguments, else the initialised process group, else a single rank."""
    if world is None:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(group), dist.get_world_size(group)
        return 0, 1
    return int(rank or 0), int(world)


class _ScoreBoard:
    """Scores of one pass over a video list.  Videos are registered in list order with the number of scores they contribute
    (sequences of an LTN, clips of an STN) and a ``finish(scores) -> result`` closure; the rank that owns a video (``i % world ==
    rank``) also hands over the work (sequences to pool, or a closure that scores the clips).  ``results()`` scores what is
    owned, sums the zero-padded flat vector over the ranks and runs every video's ``finish`` on every rank."""

    def __init__(self, enc, head, device, rank, world, group, pool_sequences, exchange=None, ragged=False, resident=None,
                 classifier_head=True, ucf=None):
        # resident: the pool holds spans of resident.bank's rows (add_spans) or, with ``ucf`` = dict(part_len, rewindow, l2), the
        # (first, count) bin tables of UCF videos (add_bins); classifier_head: the head's output of a pooled span (STN: a Regressor)
        self.enc, self.head, self.device, self.ragged = enc, head, device, ragged
        self.resident, self.classifier_head, self.ucf = resident, classifier_head, ucf
        self.rank, self.world, self.group, self.exchange = rank, world, group, exchange
        self.pool_sequences = pool_sequences
        self.items, self.total = [], 0             # (offset, count, finish) in list order
        self.names = []                            # the videos of ``items`` (error messages of AucWeights)
        self.pool, self.pooled = [], 0             # own LTN work waiting for a launch: (offset, sequences)
        self.parts = []                            # (offset, device tensor) scored segments of this rank

    def owns(self, i):
        return i % self.world == self.rank

    def _register(self, count, finish, name=None):
        off = self.total
        self.items.append((off, int(count), finish))
        self.names.append(name if name is not None else f"#{len(self.names)}")
        self.total += int(count)
        return off

    def add_ltn(self, i, count, make_sequences, finish, name=None):
        off = self._register(count, finish, name)
        if self.owns(i):
            seqs = make_sequences()
            if len(seqs) != count:
                raise RuntimeError(f"video {i}: {len(seqs)} sequences, {count} announced")
            self.pool.append((off, seqs))
            self.pooled += len(seqs)
            if self.pooled >= self.pool_sequences:
                self.flush()

    def add_spans(self, i, count, make_spans, finish, name=None):
        """A video of a resident set: ``make_spans() -> [(first_row, n_tokens)]`` of the bank, one per score."""
        off = self._register(count, finish, name)
        if self.owns(i):
            spans = make_spans()
            if len(spans) != count:
                raise RuntimeError(f"video {i}: {len(spans)} spans, {count} announced")
            self.pool.append((off, spans))
            self.pooled += count
            if self.pooled >= self.pool_sequences:
                self.flush()

    def add_bins(self, i, count, make_table, finish, name=None):
        """A UCF video of a resident set: ``make_table() -> (first [32], count [32])``, its bins as runs of bank clips."""
        off = self._register(count, finish, name)
        if self.owns(i):
            self.pool.append((off, make_table()))
            self.pooled += count
            if self.pooled >= self.pool_sequences:
                self.flush()

    def _flush_resident(self):
        bank = self.resident.bank
        if self.ucf is not None:
            # the bins of every pooled video in one launch -> a bins bank [32 * videos, P, d], then spans of that bank
            from . import functional as Fn
            first = [v for _, (f, _c) in self.pool for v in f]
            count = [v for _, (_f, c) in self.pool for v in c]
            n_bins = len(self.pool[0][1][0])
            bank = Fn.segment_mean(bank, first, count, l2=self.ucf["l2"])
            per = [scoring.ucf_bin_spans(self.ucf["part_len"], self.ucf["rewindow"], bank.shape[1], v * n_bins, n_bins)
                   for v in range(len(self.pool))]
        else:
            per = [spans for _, spans in self.pool]
        sc = scoring.resident_sequence_scores(self.enc, self.head, bank, [q for spans in per for q in spans], ragged=self.ragged,
                                              classifier_head=self.classifier_head)
        o = 0
        for (off, _), spans in zip(self.pool, per):
            self.parts.append((off, sc[o:o + len(spans)]))
            o += len(spans)
        self.pool, self.pooled = [], 0

    def add_clips(self, i, count, score, finish, name=None):
        off = self._register(count, finish, name)
        if self.owns(i):
            sc = score().reshape(-1).float()
            if sc.numel() != count:
                raise RuntimeError(f"video {i}: {sc.numel()} clip scores, {count} announced")
            self.parts.append((off, sc))

    def flush(self):
        if not self.pool:
            return
        if self.resident is not None:
            return self._flush_resident()
        sc = scoring.ltn_sequence_scores(self.enc, self.head, [q for _, seqs in self.pool for q in seqs],
                                         **({"ragged": self.ragged} if self.ragged else {}))
        o = 0
        for off, seqs in self.pool:
            self.parts.append((off, sc[o:o + len(seqs)]))
            o += len(seqs)
        self.pool, self.pooled = [], 0

    def flat_scores(self):
        """The complete flat score vector of the pass on the device: own scores, then the sum over the ranks."""
        self.flush()
        flat = torch.zeros((self.total,), device=self.device, dtype=torch.float32)
        for off, sc in self.parts:
            flat[off:off + sc.numel()] = sc
        if self.world > 1:
            if self.exchange is not None:
                self.exchange(flat)                 # tests: several ranks emulated in one process
            else:
                import torch.distributed as dist
                from .dist import all_reduce_sum
                all_reduce_sum(flat, self.group)
        return flat

    def results(self):
        host = self.flat_scores().cpu().numpy()
        return [finish(host[off:off + n]) for off, n, finish in self.items]


def _threshold(scores_np, threshold):
    s = torch.from_numpy(np.ascontiguousarray(scores_np, dtype=np.float32)).reshape(-1, 1)
    return torch.where(s > threshold, s, torch.zeros_like(s)).numpy()


@torch.no_grad()
def generate_pseudo_labels(enc, head, mode, dataset, dataset_path, training_txt, threshold, part_len=1, n_patch=16,
                           d_model=None, segment_len=16, classifier_head=False, out_path=None, pool_sequences=2048,
                           rank=None, world=None, group=None, exchange=None, ragged=False, resident=None):
    """mode 'STN' | 'LTN'; dataset 'SHT' | 'UCF' | 'UBnormal'.  Returns the dict (and writes it when ``out_path`` - on rank 0
    only under several ranks; every rank returns the complete dict).  ``ragged``: the pooled LTN parts of all lengths (the short
    tail parts of ``tail='short'``) share padded batches (scoring.ltn_sequence_scores); ``"unpadded"``: they share batches without
    padding (parts of at most 127 patch tokens).  ``resident``: a ``ResidentSet`` of the list's videos (STN: every stored patch,
    ``n_patch=None``; UCF: ``view=True``) - the archive is not opened and nothing is uploaded."""
    device = next(enc.parameters()).device
    d_model = d_model or enc.layer_norm.normalized_shape[0]
    rank, world = _ranks(rank, world, group)
    if resident is not None:
        return _generate_resident(enc, head, mode, dataset, training_txt, threshold, part_len, n_patch, segment_len, classifier_head,
                                  out_path, _ScoreBoard(enc, head, device, rank, world, group, pool_sequences, exchange, ragged, resident,
                                                        classifier_head=(mode != "STN" or classifier_head),
                                                        ucf=dict(part_len=part_len, rewindow=False, l2=False)
                                                        if (mode != "STN" and dataset == "UCF") else None))
    board = _ScoreBoard(enc, head, device, rank, world, group, pool_sequences, exchange, ragged)
    keys = []

    with FeatureArchive(dataset_path) as arc:
        for i, (line, key) in enumerate(_train_keys(dataset, training_txt)):
            keys.append(key + ".npy")
            if mode == "STN":
                board.add_clips(i, arc.shape(key + ".npy")[0],
                                lambda key=key: scoring.stn_clip_scores(enc, head, _dev(arc[key + ".npy"], device), classifier_head),
                                lambda v: _threshold(v, threshold))
                continue
            if dataset == "UCF":
                ranges = scoring.ucf_bin_ranges(part_len, rewindow=False)

                def make(line=line):
                    feats, n_frames = UCF_train(line, dataset_path, segment_len)
                    f = _dev(feats, device).view(-1, n_patch, d_model)
                    return scoring.ltn_ucf_bin_sequences(f, n_frames, part_len, segment_len, normalize=False, rewindow=False)[0]
            else:
                ranges = scoring.part_ranges(arc.shape(key + ".npy")[0], part_len)

                def make(key=key):
                    return scoring.ltn_part_sequences(_dev(arc[key + ".npy"], device), part_len, tail="short")[0]
            board.add_ltn(i, len(ranges), make,
                          lambda v, ranges=ranges: _threshold(np.concatenate([np.repeat(x, e - b) for x, (b, e) in zip(v, ranges)]),
                                                              threshold))
        rows = board.results()
    out = dict(zip(keys, rows))                   # the list-file key order of the saved dict
    if out_path and rank == 0:
        np.save(out_path, out)
    return out


def _label_rows(ranges, threshold):
    return lambda v: _threshold(np.concatenate([np.repeat(x, e - b) for x, (b, e) in zip(v, ranges)]), threshold)


def _generate_resident(enc, head, mode, dataset, training_txt, threshold, part_len, n_patch, segment_len, classifier_head, out_path,
                       board):
    """``generate_pseudo_labels`` over a ResidentSet: the same list walk, every video registered as spans of the bank."""
    rs, keys = board.resident, []
    # the host-fed generators score every stored patch (no cut to n_patch); only the UCF route views the rows as [-1, n_patch, d]
    P = rs.patches(n_patch, "generate_pseudo_labels") if (mode != "STN" and dataset == "UCF") else rs.bank.shape[1]
    for i, (line, key) in enumerate(_train_keys(dataset, training_txt)):
        keys.append(key + ".npy")
        n = rs.n_clips(key)
        if mode == "STN":
            board.add_spans(i, n, lambda key=key, n=n: scoring.part_spans(n, 1, P, first_clip=rs.first_clip(key))[0],
                            lambda v: _threshold(v, threshold))
        elif dataset == "UCF":
            ranges = scoring.ucf_bin_ranges(part_len, rewindow=False)
            n_frames = _ucf_line(line)[1]
            board.add_bins(i, len(ranges), lambda key=key, n=n, n_frames=n_frames: scoring.ucf_bin_table(
                n_frames, segment_len, first_clip=rs.first_clip(key), n_clips=n), _label_rows(ranges, threshold))
        else:
            ranges = scoring.part_ranges(n, part_len)
            board.add_spans(i, len(ranges), lambda key=key, n=n: scoring.part_spans(n, part_len, P, "short", rs.first_clip(key))[0],
                            _label_rows(ranges, threshold))
    out = dict(zip(keys, board.results()))
    if out_path and board.rank == 0:
        np.save(out_path, out)
    return out


class AucWeights:
    """The per-row frame counts of ONE pass - one (list, masks, mode, part_len, segment_len): ``pos[i]`` / ``neg[i]`` frames labelled
    1 / 0 repeat the score of flat row i (int32 device tensors once filled; ``pos_host`` / ``neg_host`` the same counts as int64
    numpy arrays), ``total`` rows, ``frames`` frames.  Created empty, filled by the first ``evaluate_auc`` / ``evaluate_train_auc``
    call that gets it as ``device_auc=`` and reused by the later ones: the labels of a list do not change between evaluations.

    ``fill`` derives the counts from the ``finish`` closures the pass registered, so the tail rules (re-windowed tail, negative
    slice, UCF bin edges, ``anno[:n]``) exist once: every closure runs on its own flat row numbers instead of scores, what comes back
    as frame "scores" are the frames' row ids (exact through float32 below 2^24 - hence the row limit) beside their labels."""
    MAX_ROWS, MAX_FRAMES = 1 << 24, 1 << 26          # the limits of lstc_auc_weighted (include/lstc_hip.h)

    def __init__(self):
        self.pos = self.neg = self.pos_host = self.neg_host = None
        self.total, self.frames = None, 0

    @property
    def filled(self):
        return self.total is not None

    def fill(self, board):
        """From the registered videos of ``board`` (a ``_ScoreBoard`` after its list walk), onto the board's device.  Every refusal
        is a ValueError raised before anything is launched."""
        total = int(board.total)
        if total > self.MAX_ROWS:
            raise ValueError(f"AucWeights: {total} score rows, lstc_auc_weighted takes at most 2^24")
        if total <= 0:
            raise ValueError("AucWeights: the pass registered no scores")
        ids, labels, frames = [], [], 0
        for (off, n, finish), name in zip(board.items, board.names):
            s, l = finish(np.arange(off, off + n, dtype=np.float32))
            s, l = np.asarray(s), np.asarray(l)
            if s.size != l.size:
                raise ValueError(f"AucWeights: video {name!r} has {s.size} frame scores and {l.size} frame labels")
            frames += s.size
            if frames > self.MAX_FRAMES:
                raise ValueError(f"AucWeights: more than 2^26 frames (at video {name!r})")
            if not np.all((l == 0) | (l == 1)):
                raise ValueError(f"AucWeights: video {name!r} has a frame label other than 0 / 1")
            ids.append(s.ravel().astype(np.int64))
            labels.append(l.ravel().astype(np.float64))
        ids, labels = np.concatenate(ids), np.concatenate(labels)
        if ids.size and (ids.min() < 0 or ids.max() >= total):
            raise ValueError("AucWeights: a finish closure returned something other than its own scores")
        pos = np.bincount(ids, weights=labels, minlength=total).astype(np.int64)
        neg = np.bincount(ids, minlength=total).astype(np.int64) - pos
        self.pos_host, self.neg_host = pos, neg
        self.pos = torch.from_numpy(pos.astype(np.int32)).to(board.device)
        self.neg = torch.from_numpy(neg.astype(np.int32)).to(board.device)
        self.total, self.frames = total, int(frames)
        return self

    def auc(self, flat):
        """AUC of the flat device score vector of the pass: two launches, then the pass's only device-to-host copy (40 bytes)."""
        from . import functional as Fn
        if flat.numel() != self.total:
            raise ValueError(f"AucWeights: built for {self.total} score rows, got {flat.numel()}")
        return float(Fn.read_auc(Fn.weighted_auc(flat.contiguous(), self.pos, self.neg)).auc)


def ucf_class(name):
    """The class of a UCF-Crime video: the alphabetic prefix of its name (``Abuse028_x264`` -> ``Abuse``,
    ``Normal_Videos_003_x264`` -> ``Normal``, ``RoadAccidents001_x264`` -> ``RoadAccidents``); a directory and an extension are
    dropped first."""
    base = str(name).replace("\\", "/").split("/")[-1].split(".")[0]
    k = 0
    while k < len(base) and base[k].isalpha():
        k += 1
    return base[:k]


class ReportWeights(AucWeights):
    """``AucWeights`` whose evaluation is the whole detection report (``lstc_det_report``): handed to ``evaluate_auc`` /
    ``evaluate_train_auc`` as ``device_auc=``, the pass returns the overall AUC as before and leaves a ``metrics.DetectionReport``
    in ``self.report`` - AUC, AP, PR-AUC, the confusion counts at ``thresholds`` and the score sums of all frames, and, with
    ``group_of`` (video name -> class name, e.g. ``ucf_class``), the same per class: ``fill`` maps every flat row to the class of
    its video, classes numbered in first-seen order (``group_names``).  Two reports per evaluation (all rows; the rows by class),
    and 208 bytes per record come to the host.  At most 2^20 rows and 64 classes (ValueError before any launch)."""
    MAX_ROWS, MAX_GROUPS = 1 << 20, 64               # the limits of lstc_det_report (include/lstc_hip.h)

    def __init__(self, group_of=None, thresholds=(0.5,)):
        super().__init__()
        self.group_of, self.thresholds = group_of, tuple(float(t) for t in thresholds)
        if not 1 <= len(self.thresholds) <= 8:
            raise ValueError(f"ReportWeights: 1 .. 8 thresholds, got {len(self.thresholds)}")
        self.group_names, self.gid, self.gid_host, self.report = [], None, None, None
        self._thresholds_dev = None

    def fill(self, board):
        if int(board.total) > self.MAX_ROWS:
            raise ValueError(f"ReportWeights: {int(board.total)} score rows, lstc_det_report takes at most 2^20")
        names, gid = [], None
        if self.group_of is not None:
            gid = np.zeros(max(int(board.total), 0), np.int64)
            for (off, n, _), name in zip(board.items, board.names):
                cls = self.group_of(name)
                if cls not in names:
                    names.append(cls)
                gid[off:off + n] = names.index(cls)
            if len(names) > self.MAX_GROUPS:
                raise ValueError(f"ReportWeights: {len(names)} classes, lstc_det_report takes at most 64")
        super().fill(board)
        self.group_names, self.gid_host = names, gid
        self.gid = None if gid is None else torch.from_numpy(gid.astype(np.int32)).to(board.device)
        self._thresholds_dev = torch.tensor(self.thresholds, dtype=torch.float32).to(board.device)
        return self

    def auc(self, flat):
        """The report of the flat device score vector of the pass (``self.report``); returns its overall AUC."""
        from . import functional as Fn
        from .metrics import DetectionReport
        if flat.numel() != self.total:
            raise ValueError(f"ReportWeights: built for {self.total} score rows, got {flat.numel()}")
        flat = flat.contiguous()
        whole = Fn.detection_report(flat, self.pos, self.neg, thresholds=self._thresholds_dev)
        parts = None
        if self.gid is not None and self.group_names:
            parts = Fn.detection_report(flat, self.pos, self.neg, self.gid, len(self.group_names), self._thresholds_dev)
        overall = Fn.read_detection_report(whole)[0]
        groups = Fn.read_detection_report(parts) if parts is not None else []
        self.report = DetectionReport(overall, groups, self.group_names, self.thresholds)
        return float(overall.auc)


def _device_auc_arg(device_auc, return_frames, what):
    """None (the host AUC), or the AucWeights of the pass: a fresh one for ``True``."""
    if device_auc is None or device_auc is False:
        return None
    if return_frames:
        raise ValueError(f"{what}: device_auc returns the AUC alone; return_frames=True stays on the host route")
    if device_auc is True:
        return AucWeights()
    if not isinstance(device_auc, AucWeights):
        raise TypeError(f"{what}: device_auc takes True or a pipeline.AucWeights, got {type(device_auc).__name__}")
    return device_auc


def _finish_pass(board, weights, return_frames, what):
    """The AUC of a walked list: on the host from every video's frames, or (``weights``) on the device from the flat vector."""
    if weights is None:
        return _auc_of(board.results(), return_frames)
    if not weights.filled:
        weights.fill(board)
    elif weights.total != board.total:
        raise ValueError(f"{what}: the AucWeights hold {weights.total} score rows, this pass has {board.total} - one AucWeights per "
                         "(list, masks, mode, part_len, segment_len)")
    return weights.auc(board.flat_scores())


def _auc_of(rows, return_frames):
    s, l = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
    auc = roc_auc(s, l)
    return (auc, s, l) if return_frames else auc


@torch.no_grad()
def evaluate_auc(enc, head, mode, dataset, dataset_path, testing_txt, masks, part_len, n_patch, segment_len=16,
                 return_frames=False, pool_sequences=2048, rank=None, world=None, group=None, exchange=None, ragged=False,
                 resident=None, device_auc=None):
    """``masks``: directory of ``<video>.npy`` frame masks (SHT / UBnormal, ``--test_mask_dir``) or the ground-truth
    archive (UCF, ``--test_mask_path``).  LTN only scores parts; STN scores clips (in-loop evaluation of the spatio
    scripts, Train/spatio_transformer_shanghaitech.py:118-150: every clip's score x segment_len).  ``ragged``: pooled LTN
    parts of all lengths share padded batches (scoring.ltn_sequence_scores); ``"unpadded"``: batches without padding.
    ``resident``: a ``ResidentSet`` of the list's videos, cut to ``n_patch`` (UCF: ``view=True``) - ``dataset_path`` is not opened,
    nothing is uploaded, STN clips are pooled like LTN parts and the UCF bins of a pool are one ``lstc_segment_mean`` launch.
    ``device_auc``: ``True`` or an ``AucWeights`` (filled by the first call, reused by the later ones; ValueError when it was built
    for another row count) - the AUC is computed on the device from the flat score vector (``lstc_auc_weighted``) and the float read
    from its record is returned: no score comes to the host.  With ``resident`` and filled weights no mask file and no ground-truth
    archive is opened either.  Not with ``return_frames`` (ValueError)."""
    weights = _device_auc_arg(device_auc, return_frames, "evaluate_auc")
    device = next(enc.parameters()).device
    rank, world = _ranks(rank, world, group)
    labels_known = weights is not None and weights.filled      # the finish closures will not run: their labels are not read
    board = _ScoreBoard(enc, head, device, rank, world, group, pool_sequences, exchange, ragged, resident,
                        classifier_head=(mode == "LTN"),
                        ucf=dict(part_len=part_len, rewindow=True, l2=True) if (dataset == "UCF" and mode == "LTN") else None)
    rs = resident
    P = rs.patches(n_patch, "evaluate_auc") if rs is not None else n_patch

    def stn_finish(anno):
        def fin(v):
            s = np.repeat(v, segment_len)
            return s, np.asarray(anno[:s.shape[0]])
        return fin

    if dataset == "UCF":
        for i, line in enumerate(open(testing_txt, "r").readlines()):
            name = _ucf_line(line)[0]
            if rs is None and board.owns(i):
                feats, anno, n_frames, _ = UCF_test(line, dataset_path, masks, segment_len, return_name=True)
            else:                                    # not ours: the list line and the ground truth say everything but the scores
                key, n_frames, fields = _ucf_line(line)
                feats = None
                if labels_known and rs is not None:
                    anno = None
                elif fields[2] == "Normal":
                    anno = np.zeros(n_frames)
                else:
                    with FeatureArchive(masks) as gt:
                        anno = np.asarray(gt[key + ".npy"])
            if rs is not None:
                n = rs.n_clips(key)
                if mode != "LTN":
                    board.add_spans(i, n, lambda key=key, n=n: scoring.part_spans(n, 1, P, first_clip=rs.first_clip(key))[0],
                                    stn_finish(anno), name)
                    continue
                ranges = scoring.ucf_bin_ranges(part_len, rewindow=True)
                r = scoring.ucf_bin_edges(n_frames, segment_len)
                board.add_bins(i, len(ranges), lambda key=key, n=n, n_frames=n_frames: scoring.ucf_bin_table(
                    n_frames, segment_len, first_clip=rs.first_clip(key), n_clips=n),
                    lambda v, ranges=ranges, r=r, anno=anno: scoring.frame_scores_ucf(v, ranges, r, anno, segment_len), name)
                continue
            if mode != "LTN":
                if feats is None:
                    with FeatureArchive(dataset_path) as arc:
                        shp = arc.shape(_ucf_line(line)[0] + ".npy")
                        n_clips = int(np.prod(shp)) // (n_patch * shp[-1])
                else:
                    n_clips = int(np.prod(feats.shape)) // (n_patch * feats.shape[-1])

                def score(feats=feats):
                    f = _dev(feats, device)
                    return scoring.stn_clip_scores(enc, head, f.view(-1, n_patch, f.shape[-1]))
                board.add_clips(i, n_clips, score, stn_finish(anno), name)
                continue
            ranges = scoring.ucf_bin_ranges(part_len, rewindow=True)
            r = scoring.ucf_bin_edges(n_frames, segment_len)

            def make(feats=feats, n_frames=n_frames):
                f = _dev(feats, device)
                return scoring.ltn_ucf_bin_sequences(f.view(-1, n_patch, f.shape[-1]), n_frames, part_len, segment_len,
                                                     normalize=True, rewindow=True)[0]
            board.add_ltn(i, len(ranges), make,
                          lambda v, ranges=ranges, r=r, anno=anno: scoring.frame_scores_ucf(v, ranges, r, anno, segment_len), name)
    elif rs is not None:
        if labels_known:
            keys = [line.strip().split(",")[0] for line in open(testing_txt, "r").readlines()]
            annos = [None] * len(keys)
        else:
            keys, annos = test_list("sht" if dataset in ("SHT", "MT_SHT") else "ubnormal", testing_txt, masks)
        for i, (key, anno) in enumerate(zip(keys, annos)):
            n = rs.n_clips(key)
            if mode != "LTN":
                board.add_spans(i, n, lambda key=key, n=n: scoring.part_spans(n, 1, P, first_clip=rs.first_clip(key))[0], stn_finish(anno),
                                key)
                continue
            ranges = scoring.part_ranges(n, part_len)
            board.add_spans(i, len(ranges), lambda key=key, n=n: scoring.part_spans(n, part_len, P, "rewindow", rs.first_clip(key))[0],
                            lambda v, ranges=ranges, anno=anno: scoring.frame_scores_sht(v, ranges, anno, segment_len), key)
    else:
        loader = shanghaitech_test if dataset in ("SHT", "MT_SHT") else UBnormal_test
        feats_l, _, annos = loader(testing_txt, masks, dataset_path)
        names = [line.strip().split(",")[0] for line in open(testing_txt, "r").readlines()] if weights is not None else None
        for i, (feats, anno) in enumerate(zip(feats_l, annos)):
            name = names[i] if names else None
            n = feats.shape[0]
            if mode != "LTN":
                board.add_clips(i, n, lambda feats=feats: scoring.stn_clip_scores(enc, head, _dev(feats, device, n_patch)),
                                stn_finish(anno), name)
                continue
            ranges = scoring.part_ranges(n, part_len)
            board.add_ltn(i, len(ranges),
                          lambda feats=feats: scoring.ltn_part_sequences(_dev(feats, device, n_patch), part_len, tail="rewindow")[0],
                          lambda v, ranges=ranges, anno=anno: scoring.frame_scores_sht(v, ranges, anno, segment_len), name)
    return _finish_pass(board, weights, return_frames, "evaluate_auc")


@torch.no_grad()
def evaluate_train_auc(enc, head, mode, dataset, train_archive, training_txt, mask_dir, part_len, n_patch, segment_len=16,
                       return_frames=False, pool_sequences=2048, rank=None, world=None, group=None, exchange=None, resident=None,
                       device_auc=None):
    """Frame-level AUC over the TRAINING videos, the quantity the SHT / UBnormal train scripts select checkpoints on
    (Train/temporal_transformer_shanghaitech.py:186-229, Train/spatio_transformer_shanghaitech.py:145-172,
    Train/temporal_transformer_UBnormal.py:193-232): every training video is scored like a test video; a normal video's
    frames are labelled 0, an abnormal video's labels are the first frames of ``mask_dir + key + ".npy"`` (the upstream
    string concatenation - ``--test_mask_dir`` holds the masks of the training videos too).  Video class: second list
    field (SHT ``name,label``) or the ``abnormal`` / ``normal`` name prefix (UBnormal).  ``resident``: a ``ResidentSet`` of the
    training videos - ``ResidentSet.from_pairs(feed)`` wraps the training bank already in HBM - instead of ``train_archive``.
    ``device_auc``: as in ``evaluate_auc`` (the masks are read when the weights are filled, and never after)."""
    weights = _device_auc_arg(device_auc, return_frames, "evaluate_train_auc")
    device = next(enc.parameters()).device
    rank, world = _ranks(rank, world, group)
    rs = resident
    board = _ScoreBoard(enc, head, device, rank, world, group, pool_sequences, exchange, False, rs, classifier_head=(mode == "LTN"))
    P = rs.patches(n_patch, "evaluate_train_auc") if rs is not None else n_patch

    def frame_labels(abnormal, key, n):
        if not abnormal:
            return np.zeros(n)
        return np.asarray(np.load(mask_dir + key + ".npy", allow_pickle=True))[:n]

    import contextlib
    with (FeatureArchive(train_archive) if rs is None else contextlib.nullcontext()) as arc:
        for i, line in enumerate(open(training_txt, "r").readlines()):
            fields = line.strip().split(",")
            key = fields[0]
            if dataset in ("SHT", "MT_SHT"):
                abnormal = int(fields[1]) == 1
            elif len(fields) > 1 and fields[1].strip() in ("0", "1"):
                # the upstream pass reads the second column as the 0/1 class (Train/temporal_transformer_UBnormal.py:198)
                abnormal = int(fields[1]) == 1
            else:
                # the published UBnormal list holds a FRAME COUNT there (train_video_names_frames.txt; upstream then looks for
                # a mask of every video and stops) - the class of such a line comes from the file name
                abnormal = not key.startswith("normal")
            n = arc.shape(key + ".npy")[0] if rs is None else rs.n_clips(key)
            if mode != "LTN":
                def fin(v, abnormal=abnormal, key=key):
                    s = np.repeat(v, segment_len)
                    return s, frame_labels(abnormal, key, s.shape[0])
                if rs is not None:
                    board.add_spans(i, n, lambda key=key, n=n: scoring.part_spans(n, 1, P, first_clip=rs.first_clip(key))[0], fin, key)
                    continue
                board.add_clips(i, n, lambda key=key: scoring.stn_clip_scores(enc, head, _dev(arc[key + ".npy"], device, n_patch)), fin,
                                key)
                continue
            ranges = scoring.part_ranges(n, part_len)

            def expand(v, ranges=ranges, abnormal=abnormal, key=key):
                sfr = np.concatenate([np.full((e - b) * segment_len, float(x), np.float32) for x, (b, e) in zip(v, ranges)])
                return sfr, frame_labels(abnormal, key, sfr.shape[0])
            if rs is not None:
                board.add_spans(i, len(ranges), lambda key=key, n=n: scoring.part_spans(n, part_len, P, "rewindow", rs.first_clip(key))[0],
                                expand, key)
                continue
            board.add_ltn(i, len(ranges),
                          lambda key=key: scoring.ltn_part_sequences(_dev(arc[key + ".npy"], device, n_patch), part_len, tail="rewindow")[0],
                          expand, key)
        return _finish_pass(board, weights, return_frames, "evaluate_train_auc")
