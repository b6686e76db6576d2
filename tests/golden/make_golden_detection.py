#!/usr/bin/env python3
"""Golden values for the detection report (lstc_vad_amd.metrics: ``detection_report_weighted``, the ``cal_*`` functions and
``eval_each_part``), produced by the REAL reference's ``utils/eval_utils.py`` (sklearn behind it).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_detection.py [--out DIR]      # build container only

Every case is a small list of weighted rows - float32 score, ``pos`` / ``neg`` frames labelled 1 / 0, a group id - drawn here from
a seeded generator.  The rows are expanded to frames (a row's score repeated pos + neg times) and the reference's own functions
run on the frames: all rows together (``<case>.overall``, one value per name in ``functions``) and the rows of every group
(``<case>.groups`` [n_groups, len(GROUP_FUNCTIONS)], NaN where the group lacks the frames the function needs).  The 14-class case
also runs ``eval_each_part`` and records its printed lines and both return values.  Output: ``tests/golden/detection.npz``."""
import argparse
import contextlib
import io
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from _refimport import assert_reference, bind_reference              # noqa: E402

FUNCTIONS = ["cal_auc", "cal_pr_auc", "cal_AP", "cal_false_alarm", "cal_false_neg", "cal_precision", "cal_recall", "cal_accuracy",
             "cal_specific", "cal_sensitivity", "cal_geometric_mean", "cal_f_measure", "cal_MCC", "cal_score_gap", "cal_pAUC",
             "cal_rmse"]
GROUP_FUNCTIONS = ["cal_auc", "cal_pr_auc", "cal_AP", "cal_false_alarm", "cal_score_gap"]
UCF_CLASSES = ["Abuse", "Arrest", "Arson", "Assault", "Burglary", "Explosion", "Fighting", "RoadAccidents", "Robbery", "Shooting",
               "Shoplifting", "Stealing", "Vandalism", "Normal"]


def cases():
    """name -> (scores float32 [n], pos int64 [n], neg int64 [n], gid int64 [n], n_groups)."""
    rs = np.random.RandomState(20261021)
    out = {}

    def weights(n, wmax=20):
        return rs.randint(0, wmax + 1, n).astype(np.int64), rs.randint(0, wmax + 1, n).astype(np.int64)

    def put(name, s, pos, neg, gid, n_groups):
        out[name] = (np.asarray(s, np.float32), pos, neg, np.asarray(gid, np.int64), n_groups)

    n = 200                                                              # every score distinct
    put("no_ties", rs.permutation(n).astype(np.float32) / np.float32(n), *weights(n), rs.randint(0, 3, n), 3)
    n = 300                                                              # 5 distinct scores
    put("ties_5", rs.choice([0.1, 0.3, 0.5, 0.7, 0.9], n), *weights(n), rs.randint(0, 4, n), 4)
    n = 150                                                              # 3 distinct scores
    put("ties_3", rs.choice([0.2, 0.5, 0.8], n), *weights(n), rs.randint(0, 2, n), 2)
    n = 50
    put("all_equal", np.full(n, 0.25), *weights(n), rs.randint(0, 2, n), 2)
    put("single_row", [0.625], np.array([3]), np.array([5]), [0], 1)
    n = 120                                                              # group 2 holds label-0 frames only (normal videos)
    s, (pos, neg), gid = rs.choice(np.linspace(0, 1, 41), n), weights(n), rs.randint(0, 3, n)
    pos[gid == 2] = 0
    neg[gid == 2] += 1
    put("normal_group", s, pos, neg, gid, 3)
    n = 100                                                              # both sides of 0.5, the threshold itself, and both zeros
    put("around_half", rs.choice([-0.0, 0.0, 0.25, 0.5, 0.5000001, 0.75, 1.0], n), *weights(n), rs.randint(0, 2, n), 2)
    n = 90                                                               # the rows with the highest score cover no label-1 frame
    s, (pos, neg), gid = rs.choice([0.1, 0.4, 0.6, 0.95], n), weights(n), rs.randint(0, 2, n)
    pos[s == 0.95] = 0
    neg[s == 0.95] += 1
    put("top_tie_without_positive", s, pos, neg, gid, 2)
    n = 160                                                              # rows without weight and rows outside every group
    s, (pos, neg), gid = np.round(rs.rand(n), 1), weights(n, 6), rs.randint(0, 5, n)      # ids 3 and 4 lie outside the 3 groups
    dead = rs.rand(n) < 0.2
    pos[dead], neg[dead] = 0, 0
    put("holes", s, pos, neg, gid, 3)
    n = 280                                                              # the 13 UCF-Crime anomaly classes and Normal
    s, (pos, neg), gid = np.round(rs.rand(n), 2), weights(n, 12), np.arange(n) % 14
    s[gid == 13] = np.round(s[gid == 13] * 0.7, 2)
    pos[gid == 13] = 0
    neg[gid == 13] += 1
    put("fourteen_classes", s, pos, neg, gid, 14)
    return out


def expand(s, pos, neg):
    """Frames of the rows: (float64 scores, float64 labels), a row's label-1 frames first."""
    fs = np.repeat(s.astype(np.float64), pos + neg)
    fl = np.concatenate([np.r_[np.ones(int(a)), np.zeros(int(b))] for a, b in zip(pos, neg)]) if len(s) else np.zeros(0)
    return fs, fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    bind_reference()
    import utils.eval_utils as ref                                   # the reference's, sklearn behind it
    assert_reference(ref)
    warnings.simplefilter("ignore")
    np.seterr(all="ignore")
    data = {"functions": np.array(FUNCTIONS), "group_functions": np.array(GROUP_FUNCTIONS), "classes": np.array(UCF_CLASSES)}
    names = []
    for name, (s, pos, neg, gid, n_groups) in cases().items():
        names.append(name)
        fs, fl = expand(s, pos, neg)
        data[name + ".scores"], data[name + ".pos"], data[name + ".neg"], data[name + ".gid"] = s, pos, neg, gid
        data[name + ".n_groups"] = np.int64(n_groups)
        data[name + ".overall"] = np.array([float(getattr(ref, f)(fs, fl)) for f in FUNCTIONS], np.float64)
        per = np.full((n_groups, len(GROUP_FUNCTIONS)), np.nan)
        for g in range(n_groups):
            m = gid == g
            gs, gl = expand(s[m], pos[m], neg[m])
            P, N = int(gl.sum()), int((1 - gl).sum())
            for k, f in enumerate(GROUP_FUNCTIONS):
                if (N > 0) if f == "cal_false_alarm" else (P > 0 and N > 0):
                    per[g, k] = float(getattr(ref, f)(gs, gl))
        data[name + ".groups"] = per
    s, pos, neg, gid, _ = cases()["fourteen_classes"]
    labels_dict, scores_dict = {}, {}
    for g, cls in enumerate(UCF_CLASSES):
        m = gid == g
        gs, gl = expand(s[m], pos[m], neg[m])
        labels_dict[cls], scores_dict[cls] = list(gl), list(gs)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        normal_far, mean_ap = ref.eval_each_part(labels_dict, scores_dict)
    data["each_part.lines"] = np.array(buf.getvalue().splitlines())
    data["each_part.returns"] = np.array([float(normal_far), float(mean_ap)], np.float64)
    data["cases"] = np.array(names)
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "detection.npz")
    np.savez_compressed(path, **data)
    print(f"wrote {path}: {len(names)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
