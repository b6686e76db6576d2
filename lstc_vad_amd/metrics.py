"""Frame-level ROC-AUC with the semantics of the reference's ``utils.eval_utils.eval`` (:139-143 -> cal_auc :21-24 =
sklearn ``roc_curve`` + ``auc``, pos_label=1): tie-aware trapezoid.  Host-side numpy; pinned against the reference's own function
in tests/golden/misc.npz.  A pooled pass hands ``roc_auc`` every frame of a whole list (several hundred thousand scores for
ShanghaiTech and UCF-Crime), although each frame's score only repeats one of a few thousand to a few ten thousand ROW scores
(parts, clips, bins): ``roc_auc_weighted`` computes the same AUC from the rows and their frame counts, exactly, and is the host
statement of what ``lstc_auc_weighted`` (csrc/metrics.hip) computes on the device."""
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
