"""Frame-level ROC-AUC with the semantics of the reference's ``utils.eval_utils.eval`` (:139-143 -> cal_auc :21-24 =
sklearn ``roc_curve`` + ``auc``, pos_label=1): tie-aware trapezoid.  Host-side numpy; pinned against the reference's own function
in tests/golden/misc.npz.  A pooled pass hands ``roc_auc`` every frame of a whole list (several hundred thousand scores for
ShanghaiTech and UCF-Crime), although each frame's score only repeats one of a few thousand to a few ten thousand ROW scores
(parts, clips, bins): ``roc_auc_weighted`` computes the same AUC from the rows and their frame counts, exactly, and is the host
statement of what ``lstc_auc_weighted`` (csrc/metrics.hip) computes on the device.  The second half of the module is the rest of the
reference's ``utils/eval_utils.py`` - PR-AUC, average precision, the thresholded confusion family, the score statistics and the
per-class table - as ``detection_report_weighted`` (the host statement of ``lstc_det_report``), the frame-level functions under the
reference's names derived from it, and ``DetectionReport``, pinned against the reference's functions in tests/golden/detection.npz."""
import numpy as np


def roc_auc(scores, labels) -> float:
    s = np.asarray(scores, dtype=np.float64).ravel()
    y = np.asarray(labels, dtype=np.float64).ravel()
    order = np.argsort(-s, kind="mergesort")
    s, y = s[order], y[order]
    last_of_tie = np.r_[np.nonzero(np.diff(s))[0], y.size - 1]
    tp = np.r_[0.0, np.cumsum(y)[last_of_tie]]
    fp = np.r_[0.0, 1.0 + last_of_tie - np.cumsum(y)[last_of_tie]]
    if tp[-1] == 0 or fp[-1] == 0:
        return float("nan")
    tpr, fpr = tp / tp[-1], fp / fp[-1]
    return float(np.sum((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) * 0.5))


def roc_auc_weighted(scores, pos, neg):
    """AUC of frames that repeat row scores: row i has score ``scores[i]`` and covers ``pos[i]`` frames labelled 1 and ``neg[i]``
    labelled 0.  -> (auc, u2, P, N) with the exact integers
        u2 = sum_i sum_j pos_i neg_j (2 [s_i > s_j] + [s_i == s_j]),   P = sum pos,   N = sum neg,
    and auc = u2 / (2 P N), rounded once (NaN when P or N is 0, as ``roc_auc``).  Sort-based: a stable argsort, groups of equal
    scores g, u2 = sum_g pos_g (2 neg_below_g + neg_g).  Scores are compared as float32 values (+0.0 == -0.0); rows without weight
    are dropped before anything looks at their score."""
    s = np.asarray(scores, dtype=np.float32).ravel()
    p = np.asarray(pos).ravel().astype(np.int64)
    q = np.asarray(neg).ravel().astype(np.int64)
    if not (s.shape == p.shape == q.shape):
        raise ValueError(f"roc_auc_weighted: {s.shape[0]} scores, {p.shape[0]} pos and {q.shape[0]} neg counts")
    if (p < 0).any() or (q < 0).any():
        raise ValueError("roc_auc_weighted: negative frame count")
    keep = (p | q) != 0
    s, p, q = s[keep], p[keep], q[keep]
    P, N = int(p.sum()), int(q.sum())
    if np.isnan(s).any():
        return float("nan"), 0, P, N
    order = np.argsort(s, kind="mergesort")
    s, p, q = s[order], p[order], q[order]
    u2 = 0
    if s.size:
        first = np.r_[0, np.nonzero(s[1:] != s[:-1])[0] + 1]          # first row of every group of equal scores
        pg, qg = np.add.reduceat(p, first), np.add.reduceat(q, first)
        below = np.cumsum(qg) - qg
        u2 = sum(int(a) * (2 * int(b) + int(c)) for a, b, c in zip(pg, below, qg))      # Python integers: no 64-bit overflow
    if P == 0 or N == 0:
        return float("nan"), u2, P, N
    return u2 / (2 * P * N), u2, P, N


def eval(total_scores, total_labels, logger=None) -> float:   # noqa: A001  (reference name)
    return roc_auc(np.array(total_scores), np.array(total_labels))


# ---------------------------------------------------------------------------------------------------- the detection report
# The rest of the reference's utils/eval_utils.py (cal_pr_auc :16-19, the thresholded family :26-88, cal_score_gap, cal_pAUC,
# cal_rmse, cal_AP :145-148, eval_each_part :97-122) without sklearn.  Every one of them is a function of per-row counts over rows
# that carry weights - ``detection_report_weighted``, the host statement of ``lstc_det_report`` (csrc/metrics.hip) - and a frame is
# a row of weight 1, so each formula exists once.
DET_MAX_THRESHOLDS = 8
DET_NAN_SCORE, DET_TOO_MANY_FRAMES = 1, 2
_DET_MAX_FRAMES = 1 << 26
_NAN = float("nan")


class DetRecord:
    """One group's record, the fields of ``LstcDetOut``: Python ints ``pos`` (P), ``neg`` (N), ``u2``, ``tp_at[8]``, ``fp_at[8]``,
    floats ``auc``, ``ap``, ``pr_auc``, ``sum_s_pos``, ``sum_s_neg``, ``sum_sq_err``, and ``flags``."""
    __slots__ = ("pos", "neg", "u2", "tp_at", "fp_at", "auc", "ap", "pr_auc", "sum_s_pos", "sum_s_neg", "sum_sq_err", "flags",
                 "reserved")

    def __repr__(self):
        return "DetRecord(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"


def _pair_counts(s, p, q, g):
    """Per row i, over the rows j with g[j] == g[i]: tp_ge = sum p_j [s_j >= s_i], fp_ge = sum q_j [s_j >= s_i], tp_eq, fp_eq the
    same under s_j == s_i (int64 arrays).  Sort-based: a stable sort by (group, score), runs of equal (group, score), cumulative
    counts.  No NaN in ``s``."""
    n = s.shape[0]
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z, z, z
    order = np.lexsort((s, g))                                           # by group, then by score (both stable)
    s, p, q, g = s[order], p[order], q[order], g[order]
    new_g = np.r_[True, g[1:] != g[:-1]]
    first = np.nonzero(new_g | np.r_[True, s[1:] != s[:-1]])[0]          # first row of every run of equal (group, score)
    size = np.diff(np.r_[first, n])
    run_g = np.cumsum(new_g)[first] - 1                                  # the group run a (group, score) run lies in
    out = []
    for w in (p, q):
        eq = np.add.reduceat(w, first)
        upto = np.cumsum(eq)                                             # runs up to and including this one
        end_of_g = np.zeros(run_g[-1] + 1, np.int64)
        end_of_g[run_g] = upto                                           # the last run of a group writes last
        ge = end_of_g[run_g] - (upto - eq)
        out += [ge, eq]
    back = np.empty(n, np.int64)
    back[order] = np.arange(n)
    tp_ge, tp_eq, fp_ge, fp_eq = (np.repeat(v, size)[back] for v in out)
    return tp_ge, fp_ge, tp_eq, fp_eq


def _precisions(tp_ge, fp_ge, tp_eq, fp_eq):
    """(prec, prev) of rows that cover a positive frame: the precision at the row's own score and at the scores strictly above it;
    prev is 1.0 where nothing lies above - sklearn's closing point (recall 0, precision 1).  One IEEE division each."""
    prec = tp_ge.astype(np.float64) / (tp_ge + fp_ge).astype(np.float64)
    tg, fg = tp_ge - tp_eq, fp_ge - fp_eq
    den = tg + fg
    prev = np.ones(prec.shape, np.float64)
    np.divide(tg.astype(np.float64), den.astype(np.float64), out=prev, where=den != 0)
    return prec, prev


def _report(s, p, q, g, n_groups, thresholds):
    """The records of float64 scores ``s`` (the compares are made on these values), int64 counts and group ids, float64 thresholds."""
    import math
    if not (s.shape == p.shape == q.shape == g.shape) or s.ndim != 1:
        raise ValueError(f"detection report: {s.shape} scores, {p.shape} pos, {q.shape} neg and {g.shape} group ids")
    if (p < 0).any() or (q < 0).any():
        raise ValueError("detection report: negative frame count")
    if not 1 <= len(thresholds) <= DET_MAX_THRESHOLDS:
        raise ValueError(f"detection report: 1 .. {DET_MAX_THRESHOLDS} thresholds, got {len(thresholds)}")
    if n_groups < 1:
        raise ValueError("detection report: n_groups must be at least 1")
    keep = ((p | q) != 0) & (g >= 0) & (g < n_groups)                    # the other rows do not exist
    s, p, q, g = s[keep], p[keep], q[keep], g[keep]
    real = ~np.isnan(s)
    sv, pv, qv, gv = s[real], p[real], q[real], g[real]
    tp_ge, fp_ge, tp_eq, fp_eq = _pair_counts(sv, pv, qv, gv)
    has = pv > 0
    prec, prev = _precisions(tp_ge[has], fp_ge[has], tp_eq[has], fp_eq[has])
    ap_t = np.zeros(sv.shape, np.float64)
    pr_t = np.zeros(sv.shape, np.float64)
    dp, dn = pv.astype(np.float64), qv.astype(np.float64)
    ap_t[has] = dp[has] * prec
    pr_t[has] = dp[has] * ((prec + prev) * 0.5)
    d1 = 1.0 - sv
    sp_t, sn_t, se_t = dp * sv, dn * sv, dp * (d1 * d1) + dn * (sv * sv)
    records = []
    for k in range(n_groups):
        r = DetRecord()
        r.pos, r.neg = int(p[g == k].sum()), int(q[g == k].sum())
        m = gv == k
        Pv, Nv = int(pv[m].sum()), int(qv[m].sum())
        if Pv + Nv <= _DET_MAX_FRAMES:                                       # every product and the sum stay below 2^54
            r.u2 = int((pv[m & has] * (2 * (Nv - fp_ge[m & has]) + fp_eq[m & has])).sum())
        else:                                                                # Python integers: no 64-bit overflow
            r.u2 = sum(int(a) * (2 * (Nv - int(b)) + int(c)) for a, b, c in zip(pv[m & has], fp_ge[m & has], fp_eq[m & has]))
        r.tp_at = [int(pv[m & (sv > t)].sum()) for t in thresholds] + [0] * (DET_MAX_THRESHOLDS - len(thresholds))
        r.fp_at = [int(qv[m & (sv > t)].sum()) for t in thresholds] + [0] * (DET_MAX_THRESHOLDS - len(thresholds))
        r.flags = (DET_NAN_SCORE if bool((g[~real] == k).any()) else 0) | (DET_TOO_MANY_FRAMES if r.pos + r.neg > _DET_MAX_FRAMES else 0)
        r.reserved = 0
        if r.flags:
            r.auc = r.ap = r.pr_auc = r.sum_s_pos = r.sum_s_neg = r.sum_sq_err = _NAN
        else:
            r.auc = r.u2 / (2 * r.pos * r.neg) if r.pos and r.neg else _NAN
            r.ap = math.fsum(ap_t[m]) / r.pos if r.pos else _NAN
            r.pr_auc = math.fsum(pr_t[m]) / r.pos if r.pos else _NAN
            r.sum_s_pos, r.sum_s_neg, r.sum_sq_err = math.fsum(sp_t[m]), math.fsum(sn_t[m]), math.fsum(se_t[m])
        records.append(r)
    return records


def detection_report_weighted(scores, pos, neg, groups=None, n_groups=1, thresholds=(0.5,)):
    """The host statement of ``lstc_det_report``: row i has the float32 score ``scores[i]``, covers ``pos[i]`` / ``neg[i]`` frames
    labelled 1 / 0 and belongs to group ``groups[i]`` (None: all in group 0; a row outside 0 .. n_groups - 1, or without weight,
    does not exist).  -> one ``DetRecord`` per group.  Over the rows of its group every row i has
        tp_ge = sum pos_j [s_j >= s_i],  fp_ge = sum neg_j [s_j >= s_i],  tp_eq, fp_eq the same under s_j == s_i;
    with P, N the group's frame counts,
        u2 = sum pos_i (2 (N - fp_ge) + fp_eq),  auc = u2 / (2 P N)          (``roc_auc_weighted``'s, the ROC trapezoid)
        ap = (sum pos_i prec_i) / P,  prec_i = tp_ge / (tp_ge + fp_ge)          (sklearn's average_precision_score of the frames)
        pr_auc = (sum pos_i (prec_i + prev_i) / 2) / P                            (the trapezoid under precision_recall_curve)
    where prev_i is the precision at the scores strictly above s_i, 1.0 when there is none; ``tp_at[t]`` / ``fp_at[t]`` count the
    label-1 / label-0 frames with a score > thresholds[t] (float32 compare, strict); ``sum_s_pos`` = sum pos_i s_i, ``sum_s_neg``,
    ``sum_sq_err`` = sum pos_i (1 - s_i)^2 + neg_i s_i^2.  Integers are Python ints; every float sum is ``math.fsum`` of the per-row
    float64 terms the kernel forms, divided once.  A NaN score on a row with weight sets ``DET_NAN_SCORE`` and every float to NaN;
    the integers are then those of the rows with a real score (``pos`` / ``neg`` count every row)."""
    s = np.asarray(scores, dtype=np.float32).ravel().astype(np.float64)
    p, q = np.asarray(pos).ravel().astype(np.int64), np.asarray(neg).ravel().astype(np.int64)
    g = np.zeros(s.shape, np.int64) if groups is None else np.asarray(groups).ravel().astype(np.int64)
    if groups is None and n_groups != 1:
        raise ValueError("detection_report_weighted: without groups there is one group")
    th = [float(np.float32(t)) for t in thresholds]
    return _report(s, p, q, g, int(n_groups), th)


def _ratio(a, b):
    """a / b as numpy divides float64 scalars: 0 / 0 is NaN, x / 0 is +-inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def _frames(scores, labels, threshold=0.5):
    """The record of frames (rows of weight 1); the scores are compared as the float64 values the reference compares."""
    s = np.asarray(scores, dtype=np.float64).ravel()
    y = np.asarray(labels, dtype=np.float64).ravel()
    if s.shape != y.shape:
        raise ValueError(f"{s.shape[0]} frame scores and {y.shape[0]} frame labels")
    if not np.all((y == 0) | (y == 1)):
        raise ValueError("a frame label other than 0 / 1")
    p = y.astype(np.int64)
    return _report(s, p, 1 - p, np.zeros(s.shape, np.int64), 1, [float(threshold)])[0]


def _confusion(scores, labels, threshold):
    """(tp, fp, tn, fn) as float64, the reference's sums."""
    r = _frames(scores, labels, threshold)
    tp, fp = r.tp_at[0], r.fp_at[0]
    return tuple(np.float64(v) for v in (tp, fp, r.neg - fp, r.pos - tp))


def cal_pr_auc(scores, labels):
    return _frames(scores, labels).pr_auc


def cal_AP(scores, labels):
    return _frames(scores, labels).ap


def cal_false_alarm(scores, labels, threshold=0.5):
    tp, fp, tn, fn = _confusion(scores, labels, threshold)
    return _ratio(fp, fp + tn)


def cal_false_neg(scores, labels, threshold=0.5):
    tp, fp, tn, fn = _confusion(scores, labels, threshold)
    return _ratio(fn, tp + fn)


def cal_precision(scores, labels, threshold=0.5):
    tp, fp, tn, fn = _confusion(scores, labels, threshold)
    return _ratio(tp, tp + fp)


def cal_accuracy(scores, labels, threshold=0.5):
    tp, fp, tn, fn = _confusion(scores, labels, threshold)
    return _ratio(tp + tn, tp + fp + tn + fn)


def cal_recall(scores, labels, threshold=0.5):
    tp, fp, tn, fn = _confusion(scores, labels, threshold)
    return _ratio(tp, tp + fn)


def cal_specific(scores, labels, threshold=0.5):
    tp, fp, tn, fn = _confusion(scores, labels, threshold)
    return _ratio(tn, fp + tn)


def cal_sensitivity(scores, labels, threshold=0.50):
    tp, fp, tn, fn = _confusion(scores, labels, threshold)
    return _ratio(tp, tp + fn)


def cal_geometric_mean(scores, labels, threshold=0.5):
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(np.float64(cal_sensitivity(scores, labels, threshold)) * np.float64(cal_specific(scores, labels, threshold))))


def cal_f_measure(scores, labels, threshold=0.5):
    p, r = np.float64(cal_precision(scores, labels, threshold)), np.float64(cal_recall(scores, labels, threshold))
    return _ratio(2 * p * r, p + r)


def _mcc(tp, fp, tn, fn):
    """The reference's expression (:82-88), (fp + fn) in the second factor included."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float((tp * tn - fp * fn) / np.sqrt((tp + fp) * (fp + fn) * (tn + fp) * (tn + fn)))


def cal_MCC(scores, labels, threshold=0.5):
    return _mcc(*_confusion(scores, labels, threshold))


def cal_score_gap(scores, labels):
    r = _frames(scores, labels)
    return float(np.float64(_ratio(r.sum_s_pos, r.pos)) - np.float64(_ratio(r.sum_s_neg, r.neg)))


def cal_pAUC(scores, labels):
    r = _frames(scores, labels)
    return float(0.5 * (np.float64(_ratio(r.sum_s_pos, r.pos)) - np.float64(_ratio(r.sum_s_neg, r.neg)) + 1))


def cal_rmse(scores, labels):
    r = _frames(scores, labels)
    return float(np.float64(_ratio(r.sum_sq_err, r.pos + r.neg)) ** 0.5)


_PART_LINE = "{}: \tAUC \t{:.4f}, PR-AUC \t{:.4f}, FAR \t{}\tGAP\t{:.4f}"
_NORMAL_LINE = "{}: \tAUC \t{}, PR-AUC \t{}, FAR \t{}\tGAP\t{}"


class DetectionReport:
    """The records of one evaluation: ``overall`` (every row) and ``groups`` (one record per name in ``names``; empty without a
    grouping), with ``thresholds`` the values behind ``tp_at`` / ``fp_at``.  A record is anything with the fields of ``LstcDetOut``
    (``DetRecord``, ``_lib.DetOut``).  The derived numbers come from the record's integers and sums; ``t`` picks the threshold."""

    def __init__(self, overall, groups=(), names=(), thresholds=(0.5,)):
        self.overall, self.groups, self.names = overall, list(groups), list(names)
        self.thresholds = tuple(float(t) for t in thresholds)
        if len(self.groups) != len(self.names):
            raise ValueError(f"DetectionReport: {len(self.groups)} records for {len(self.names)} names")

    def record(self, name=None):
        return self.overall if name is None else self.groups[self.names.index(name)]

    @staticmethod
    def _confusion(r, t):
        tp, fp = int(r.tp_at[t]), int(r.fp_at[t])
        return tuple(np.float64(v) for v in (tp, fp, int(r.neg) - fp, int(r.pos) - tp))

    def far(self, name=None, t=0):
        tp, fp, tn, fn = self._confusion(self.record(name), t)
        return _ratio(fp, fp + tn)

    def false_neg(self, name=None, t=0):
        tp, fp, tn, fn = self._confusion(self.record(name), t)
        return _ratio(fn, tp + fn)

    def precision(self, name=None, t=0):
        tp, fp, tn, fn = self._confusion(self.record(name), t)
        return _ratio(tp, tp + fp)

    def recall(self, name=None, t=0):
        tp, fp, tn, fn = self._confusion(self.record(name), t)
        return _ratio(tp, tp + fn)

    def accuracy(self, name=None, t=0):
        tp, fp, tn, fn = self._confusion(self.record(name), t)
        return _ratio(tp + tn, tp + fp + tn + fn)

    def f_measure(self, name=None, t=0):
        p, r = np.float64(self.precision(name, t)), np.float64(self.recall(name, t))
        return _ratio(2 * p * r, p + r)

    def mcc(self, name=None, t=0):
        return _mcc(*self._confusion(self.record(name), t))

    def gap(self, name=None):
        r = self.record(name)
        return float(np.float64(_ratio(r.sum_s_pos, int(r.pos))) - np.float64(_ratio(r.sum_s_neg, int(r.neg))))

    def rmse(self, name=None):
        r = self.record(name)
        return float(np.float64(_ratio(r.sum_sq_err, int(r.pos) + int(r.neg))) ** 0.5)

    def mean_ap(self, n_classes=13):
        """``eval_each_part``'s second value: the PR-AUCs of the groups other than 'Normal', summed in their order, over
        ``n_classes`` (upstream divides by the 13 UCF-Crime anomaly classes whatever the dict holds)."""
        total = 0
        for name, r in zip(self.names, self.groups):
            if name != "Normal":
                total += r.pr_auc
        return total / n_classes

    def normal_far(self, t=0):
        return self.far("Normal", t) if "Normal" in self.names else _NAN

    def each_part_lines(self, t=0):
        """One line per group in ``eval_each_part``'s format (:108, :119)."""
        lines = []
        for name, r in zip(self.names, self.groups):
            if name == "Normal":
                lines.append(_NORMAL_LINE.format(name, "None", "None", self.far(name, t), "None"))
            else:
                lines.append(_PART_LINE.format(name, r.auc, r.pr_auc, self.far(name, t), self.gap(name)))
        return lines

    def overall_line(self, t=0):
        r = self.overall
        return "report: AUC {:.6f}, AP {:.6f}, PR-AUC {:.6f}, FAR@{:g} {:.6f}, GAP {:.6f}".format(
            r.auc, r.ap, r.pr_auc, self.thresholds[t], self.far(None, t), self.gap())


def eval_each_part(labels_dict, scores_dict, logger=None):
    """The reference's per-class table (:97-122): for every key of ``labels_dict`` one printed (or ``logger.info``) line - AUC,
    PR-AUC, FAR at 0.5 and score gap of the class's frames, FAR alone for 'Normal' - and ``(normal_far, sum of the PR-AUCs / 13)``.
    One deviation: without a 'Normal' key ``normal_far`` is NaN, where upstream raises UnboundLocalError."""
    names = list(labels_dict.keys())
    groups = [_frames(np.array(scores_dict[k], dtype=float), np.array(labels_dict[k], dtype=float)) for k in names]
    rep = DetectionReport(None, groups, names)
    for line in rep.each_part_lines():
        if logger is None:
            print(line)
        else:
            logger.info(line)
    return rep.normal_far(), rep.mean_ap(13)
