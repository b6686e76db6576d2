"""The detection report, the part that needs no GPU: ``metrics.detection_report_weighted`` (the host statement of what
``lstc_det_report`` computes), the frame-level ``cal_*`` functions and ``eval_each_part`` against the reference's own functions
(tests/golden/detection.npz, written by tests/golden/make_golden_detection.py), the twin's integers against the all-pairs
formula, ``pipeline.ucf_class``, the C ABI (record layout, refusals by return code), ``pipeline.ReportWeights`` on CPU boards, the
``--report`` flag, and four seeded mistakes that the fixture's cases must be able to see.

The bound on a double.  Scores lie in [0, 1], so every metric here lies in [-1, 1] and the bound is absolute, like the AUC's
``(K + 4) 2^-52``.  With K distinct scores, the reference side (sklearn) forms K precision / recall pairs (one rounding each) and
sums K trapezoid or step terms of at most three roundings each in float64: its error stays below (K + 8) 2^-53.  Our side forms
one term per row that covers a positive frame, n of them, each with at most four roundings, sums them with ``math.fsum`` (exact)
and divides once; counting a half unit per term for the terms' own roundings seen relative to the sum gives at most
(n + 8) 2^-53.  Together: ``(K + n + 16) 2^-53``.  The thresholded family is a single division of exact integers on both sides
(and a square root or a few products for G-mean, F-measure and MCC); it sits far inside the same bound."""
import contextlib
import ctypes as C
import io
import math
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF = "/root/reference"
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "detection.npz"), allow_pickle=False)


def case(z, name):
    return (z[name + ".scores"], z[name + ".pos"], z[name + ".neg"], z[name + ".gid"], int(z[name + ".n_groups"]))


def expand(s, pos, neg):
    fs = np.repeat(np.asarray(s, np.float32).astype(np.float64), np.asarray(pos) + np.asarray(neg))
    fl = np.concatenate([np.r_[np.ones(int(a)), np.zeros(int(b))] for a, b in zip(pos, neg)]) if len(s) else np.zeros(0)
    return fs, fl


def bound(s, pos, neg):
    """(K + n + 16) 2^-53: K distinct scores, n rows that cover a positive frame (module docstring)."""
    live = (np.asarray(pos) + np.asarray(neg)) > 0
    return (np.unique(np.asarray(s, np.float32)[live]).size + int((np.asarray(pos) > 0).sum()) + 16) * U53


def off(got, want, tol):
    """|got - want| / tol; both NaN is agreement, one NaN is not (inf)."""
    if math.isnan(want) or math.isnan(got):
        return 0.0 if math.isnan(want) and math.isnan(got) else math.inf
    if math.isinf(want) or math.isinf(got):
        return 0.0 if got == want else math.inf
    return abs(got - want) / tol


def report_values(rep, name=None):
    """The reference's function names -> the values a DetectionReport derives for one record."""
    from lstc_vad_amd import metrics as M
    r = rep.record(name)
    sens, spec = rep.recall(name), 1.0 - rep.far(name) if int(r.neg) else float("nan")
    return {"cal_auc": r.auc, "cal_pr_auc": r.pr_auc, "cal_AP": r.ap, "cal_false_alarm": rep.far(name), "cal_false_neg": rep.false_neg(name),
            "cal_precision": rep.precision(name), "cal_recall": rep.recall(name), "cal_accuracy": rep.accuracy(name),
            "cal_sensitivity": sens, "cal_f_measure": rep.f_measure(name), "cal_MCC": rep.mcc(name), "cal_score_gap": rep.gap(name),
            "cal_pAUC": 0.5 * (rep.gap(name) + 1), "cal_rmse": rep.rmse(name), "cal_specific": M._ratio(int(r.neg) - int(r.fp_at[0]), int(r.neg)),
            "cal_geometric_mean": math.sqrt(sens * M._ratio(int(r.neg) - int(r.fp_at[0]), int(r.neg))) if sens == sens else float("nan")}


def twin_worst(z, name):
    """Worst |twin - reference| / bound of a case: every function on all rows, and the group functions on every group."""
    from lstc_vad_amd import metrics as M
    s, pos, neg, gid, n_groups = case(z, name)
    tol = bound(s, pos, neg)
    whole = M.DetectionReport(M.detection_report_weighted(s, pos, neg)[0])
    got = report_values(whole)
    worst = max(off(got[f], float(w), tol) for f, w in zip(z["functions"], z[name + ".overall"]))
    groups = M.detection_report_weighted(s, pos, neg, gid, n_groups)
    rep = M.DetectionReport(None, groups, [str(k) for k in range(n_groups)])
    for k in range(n_groups):
        got = report_values(rep, str(k))
        for f, w in zip(z["group_functions"], z[name + ".groups"][k]):
            if not math.isnan(float(w)):                      # NaN: the reference was not asked (a group without the frames it needs)
                worst = max(worst, off(got[str(f)], float(w), tol))
    return worst


# ---------------------------------------------------------------------------------------------------- 1. against the reference
def test_fixture_holds_the_cases_the_issue_names(gold):
    names = list(gold["cases"])
    assert 8 <= len(names) <= 12 and os.path.getsize(os.path.join(GOLD, "detection.npz")) < 64 << 10
    uniq = {n: np.unique(gold[n + ".scores"]).size for n in names}
    assert all(gold[n + ".scores"].size <= 300 for n in names)
    assert uniq["no_ties"] == gold["no_ties.scores"].size and uniq["ties_3"] == 3 and uniq["ties_5"] == 5 and uniq["all_equal"] == 1
    assert gold["single_row.scores"].size == 1
    s, pos, neg, gid, _ = case(gold, "normal_group")
    assert pos[gid == 2].sum() == 0 and neg[gid == 2].sum() > 0
    s = gold["around_half.scores"]
    assert (s > 0.5).any() and (s < 0.5).any() and (s == 0.5).any() and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
    s, pos, neg, gid, _ = case(gold, "top_tie_without_positive")
    assert pos[s == s.max()].sum() == 0 and neg[s == s.max()].sum() > 0
    assert int(gold["fourteen_classes.n_groups"]) == 14 and list(gold["classes"])[-1] == "Normal"


def test_twin_against_the_reference(gold):
    worst = {n: twin_worst(gold, n) for n in gold["cases"]}
    print("detection_report_weighted against the reference, worst |error| / bound per case:", {str(k): "%.3f" % v for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst                    # above half the bound: look for a defect first


def test_frame_functions_against_the_reference(gold):
    from lstc_vad_amd import metrics as M
    import utils.eval_utils as shim
    worst = 0.0
    for name in gold["cases"]:
        s, pos, neg, _, _ = case(gold, name)
        fs, fl = expand(s, pos, neg)
        tol = bound(s, pos, neg)
        for f, want in zip(gold["functions"], gold[name + ".overall"]):
            fn = getattr(shim, str(f))
            assert str(f) == "cal_auc" or fn is getattr(M, str(f))
            with np.errstate(all="ignore"):
                got = fn(fs, fl)
            assert isinstance(got, float)
            r = off(got, float(want), tol)
            worst = max(worst, r)
            assert r <= 1.0, (name, f, got, float(want), r)
    print("frame-level functions against the reference: worst |error| / bound %.3f" % worst)
    assert worst <= 0.5
    # the reference's threshold argument, strict >
    fs, fl = np.array([0.2, 0.5, 0.5, 0.7, 0.9]), np.array([0.0, 0.0, 1.0, 0.0, 1.0])
    assert M.cal_false_alarm(fs, fl) == 1 / 3 and M.cal_false_alarm(fs, fl, 0.4) == 2 / 3 and M.cal_false_alarm(fs, fl, threshold=0.9) == 0.0
    assert M.cal_recall(fs, fl) == 0.5 and M.cal_sensitivity(fs, fl, 0.4) == 1.0
    assert math.isnan(M.cal_precision(fs, fl, 0.95)) and math.isnan(M.cal_false_alarm(fs[[2, 4]], fl[[2, 4]]))      # 0 / 0
    assert not hasattr(shim, "cal_f1") and not hasattr(shim, "eval_classification") and not hasattr(shim, "plt")


def test_twin_integers_are_the_all_pairs_formula(gold):
    from lstc_vad_amd import metrics as M
    th = (0.5, 0.25, np.float32(0.1), 1.0)
    for name in gold["cases"]:
        s, pos, neg, gid, n_groups = case(gold, name)
        for groups, ng in ((None, 1), (gid, n_groups)):
            recs = M.detection_report_weighted(s, pos, neg, groups, ng, th)
            g = np.zeros(s.size, np.int64) if groups is None else gid
            for k, r in enumerate(recs):
                m = (g == k) & ((pos + neg) > 0)
                sk, pk, qk = s[m], pos[m], neg[m]
                ge, eq = sk[None, :] >= sk[:, None], sk[None, :] == sk[:, None]
                fp_ge, fp_eq = (ge * qk[None, :]).sum(1), (eq * qk[None, :]).sum(1)
                P, N = int(pk.sum()), int(qk.sum())
                assert (r.pos, r.neg) == (P, N) and r.flags == 0 and r.reserved == 0
                assert r.u2 == int((pk * (2 * (N - fp_ge) + fp_eq)).sum()) == M.roc_auc_weighted(sk, pk, qk)[1], (name, k)
                for t, v in enumerate(th):
                    assert r.tp_at[t] == int(pk[sk > np.float32(v)].sum()) and r.fp_at[t] == int(qk[sk > np.float32(v)].sum())
                assert r.tp_at[4:] == [0] * 4 and r.fp_at[4:] == [0] * 4 and all(isinstance(v, int) for v in r.tp_at + r.fp_at + [r.u2, r.pos])
                if P and N:
                    assert r.auc == M.roc_auc_weighted(sk, pk, qk)[0]
                else:
                    assert math.isnan(r.auc) and (P > 0 or (math.isnan(r.ap) and math.isnan(r.pr_auc)))


def test_twin_nan_rows_and_refusals():
    from lstc_vad_amd import metrics as M
    s = np.array([0.1, np.nan, 0.7, np.nan, 0.4], np.float32)
    pos, neg = np.array([1, 0, 2, 3, 0]), np.array([2, 0, 1, 1, 4])
    clean = M.detection_report_weighted(s, np.array([1, 0, 2, 0, 0]), np.array([2, 0, 1, 0, 4]))[0]       # the NaN rows without weight
    assert clean.flags == 0 and clean.auc == M.roc_auc_weighted(s[[0, 2, 4]], [1, 2, 0], [2, 1, 4])[0]
    r = M.detection_report_weighted(s, pos, neg)[0]
    assert r.flags == M.DET_NAN_SCORE and (r.pos, r.neg) == (6, 8) and r.u2 == clean.u2 and r.tp_at == clean.tp_at
    assert all(math.isnan(v) for v in (r.auc, r.ap, r.pr_auc, r.sum_s_pos, r.sum_s_neg, r.sum_sq_err))
    two = M.detection_report_weighted(s, pos, neg, [0, 0, 0, 1, 7], 2)                                    # the NaN row sits in group 1
    assert two[0].flags == 0 and two[1].flags == M.DET_NAN_SCORE and (two[0].pos, two[0].neg) == (3, 3)
    with pytest.raises(ValueError):
        M.detection_report_weighted(s, pos, neg[:4])
    with pytest.raises(ValueError):
        M.detection_report_weighted(s, -pos, neg)
    with pytest.raises(ValueError):
        M.detection_report_weighted(s, pos, neg, thresholds=())
    with pytest.raises(ValueError):
        M.detection_report_weighted(s, pos, neg, thresholds=[0.5] * 9)
    with pytest.raises(ValueError):
        M.detection_report_weighted(s, pos, neg, n_groups=2)


def test_eval_each_part_prints_the_reference_lines(gold):
    from lstc_vad_amd import metrics as M
    s, pos, neg, gid, _ = case(gold, "fourteen_classes")
    labels, scores = {}, {}
    for k, cls in enumerate(gold["classes"]):
        fs, fl = expand(s[gid == k], pos[gid == k], neg[gid == k])
        labels[str(cls)], scores[str(cls)] = list(fl), list(fs)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        far, mean_ap = M.eval_each_part(labels, scores)
    assert buf.getvalue().splitlines() == [str(l) for l in gold["each_part.lines"]]
    tol = bound(s, pos, neg)
    assert off(far, float(gold["each_part.returns"][0]), tol) <= 0.5 and off(mean_ap, float(gold["each_part.returns"][1]), tol) <= 0.5
    seen = []
    logger = Namespace(info=seen.append)
    assert M.eval_each_part(labels, scores, logger) == (far, mean_ap) and seen == buf.getvalue().splitlines()
    # the same table from the weighted rows
    rep = M.DetectionReport(None, M.detection_report_weighted(s, pos, neg, gid, 14), [str(c) for c in gold["classes"]])
    assert rep.each_part_lines() == seen and rep.normal_far() == far and off(rep.mean_ap(), mean_ap, tol) <= 0.5
    # the stated deviation: no 'Normal' key
    del labels["Normal"]
    with contextlib.redirect_stdout(io.StringIO()):
        far2, map2 = M.eval_each_part(labels, scores)
    assert math.isnan(far2) and map2 == mean_ap


@pytest.mark.skipif(not os.path.isdir(REF), reason="reference tree absent (fixtures are generated in the build container)")
def test_make_golden_detection_reproduces_the_committed_fixture(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("PYTHONPATH", None)
    r = subprocess.run([sys.executable, os.path.join(GOLD, "make_golden_detection.py"), "--out", str(tmp_path)], env=env, cwd="/",
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    a, b = np.load(os.path.join(tmp_path, "detection.npz")), np.load(os.path.join(GOLD, "detection.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------- 2. the cases can see mistakes
def test_the_cases_see_four_seeded_mistakes(gold, monkeypatch):
    """The twin with one mistake at a time: each must leave the bound on at least one case (NaN counts as outside)."""
    from lstc_vad_amd import metrics as M
    counts, precisions = M._pair_counts, M._precisions

    def strictly_greater(s, p, q, g):                          # > for >=
        tp_ge, fp_ge, tp_eq, fp_eq = counts(s, p, q, g)
        return tp_ge - tp_eq, fp_ge - fp_eq, tp_eq, fp_eq

    def prev_from_ge(*c):                                       # the previous precision read from the >= counts
        prec, _ = precisions(*c)
        return prec, prec

    def closing_point_zero(tp_ge, fp_ge, tp_eq, fp_eq):        # the curve closed at precision 0
        prec, prev = precisions(tp_ge, fp_ge, tp_eq, fp_eq)
        return prec, np.where((tp_ge - tp_eq) + (fp_ge - fp_eq) == 0, 0.0, prev)

    def no_group_compare(s, p, q, g):                           # the pair loop ignores the group
        return counts(s, p, q, np.zeros_like(g))

    assert max(twin_worst(gold, n) for n in gold["cases"]) <= 0.5
    for what, attr, fn in (("> for >=", "_pair_counts", strictly_greater), ("prev from >=", "_precisions", prev_from_ge),
                           ("closing point 0", "_precisions", closing_point_zero), ("group compare dropped", "_pair_counts", no_group_compare)):
        with monkeypatch.context() as m:
            m.setattr(M, attr, fn)
            with np.errstate(all="ignore"):
                worst = {str(n): twin_worst(gold, n) for n in gold["cases"]}
        caught = [n for n, v in worst.items() if v > 1.0]
        print(f"{what}: outside the bound on {len(caught)} of {len(worst)} cases")
        assert caught, (what, worst)


# ---------------------------------------------------------------------------------------------------- 3. names, C ABI, refusals
def test_ucf_class_on_ucf_crime_names():
    from lstc_vad_amd.pipeline import ucf_class
    for name, cls in (("Abuse028_x264", "Abuse"), ("Normal_Videos_003_x264", "Normal"), ("RoadAccidents127_x264", "RoadAccidents"),
                      ("Shoplifting001_x264.npy", "Shoplifting"), ("Anomaly-Videos/Arson011_x264.mp4", "Arson"),
                      ("Normal_Videos_event", "Normal"), ("Testing_Normal_Videos_Anomaly/Normal_Videos_935_x264.mp4", "Normal"),
                      ("01_0014", "")):
        assert ucf_class(name) == cls, name


def test_det_record_layout_matches_header(lib, tmp_path):
    from lstc_vad_amd._lib import DetOut
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lstc_hip.h"', 'int main(void) {',
             'printf("LstcDetOut %zu\\n", sizeof(LstcDetOut));', 'printf("version %d\\n", LSTC_VERSION);',
             'printf("flags %u %u\\n", LSTC_DET_NAN_SCORE, LSTC_DET_TOO_MANY_FRAMES);']
    for fname, _ in DetOut._fields_:
        lines.append(f'printf("LstcDetOut.{fname} %zu %zu\\n", offsetof(LstcDetOut, {fname}), sizeof(((LstcDetOut*)0)->{fname}));')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert int(got["LstcDetOut"][0]) == C.sizeof(DetOut) == 208
    assert int(got["version"][0]) == 112 == lib.lstc_version()
    from lstc_vad_amd import _lib, metrics
    assert [int(v) for v in got["flags"]] == [_lib.DET_NAN_SCORE, _lib.DET_TOO_MANY_FRAMES] == [metrics.DET_NAN_SCORE, metrics.DET_TOO_MANY_FRAMES]
    for fname, ctype in DetOut._fields_:
        o, size = (int(x) for x in got[f"LstcDetOut.{fname}"])
        assert o == getattr(DetOut, fname).offset and size == C.sizeof(ctype), fname
    hdr = open(os.path.join(ROOT, "include", "lstc_hip.h")).read()
    assert "utils/eval_utils.py:16-19, 26-95, 97-122, 145-148" in hdr


def test_det_entry_points_refuse_by_return_code(lib):
    from lstc_vad_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("lstc_det_report", "lstc_det_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.EXPORTS
    det, need = lib.lstc_det_report, lib.lstc_det_workspace_bytes
    # (scores, pos, neg, gid, n, n_groups, thresholds, n_thresholds, workspace, workspace_bytes, out, stream): never dereferenced
    ok = [16, 16, 16, 16, 1000, 3, 16, 1, 16, need(1000, 3), 16, None]
    for i in (0, 1, 2, 6, 8, 10):
        a = list(ok)
        a[i] = None
        assert det(*a) == -1, i                                              # LSTC_E_NULL
    for n in (0, -1, -(1 << 40)):
        a = list(ok)
        a[4] = n
        assert det(*a) == -2, n                                              # LSTC_E_SHAPE
    for g in (0, -3):
        a = list(ok)
        a[5] = g
        assert det(*a) == -2, g
    for t in (0, -1, 9, 1 << 20):
        a = list(ok)
        a[7] = t
        assert det(*a) == -2, t
    a = list(ok)
    a[3] = None                                                              # no gid: one group only
    assert det(*a) == -2
    for short in (0, 16, need(1000, 3) - 1, need(999, 3)):
        a = list(ok)
        a[9] = short
        assert det(*a) == -2, short                                          # workspace too small
    for n, g in (((1 << 20) + 1, 3), (1 << 40, 3), (1000, 65), (1000, 1 << 40)):
        a = list(ok)
        a[4], a[5], a[9] = n, g, 1 << 40
        assert det(*a) == -5, (n, g)                                         # LSTC_E_RANGE
    a = list(ok)
    a[10] = 20                                                               # the records are 8-byte aligned
    assert det(*a) == -3
    sizes = [need(n, 1) for n in (1, 2, 255, 256, 257, 1023, 1024, 1025, 4099, 40000, 1 << 20)]
    assert sizes == [16 * n + 16 for n in (1, 2, 255, 256, 257, 1023, 1024, 1025, 4099, 40000, 1 << 20)]      # the stated function
    assert need(0, 1) == 32 and need(-5, 1) == 32 and need(1 << 30, 64) == sizes[-1] and need(1000, 64) == need(1000, 1)
    assert lib.lstc_version() == 112


def test_detection_report_refuses_before_the_device_matters():
    from lstc_vad_amd import functional as Fn
    s, c = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError):
        Fn.detection_report(s.double(), c, c)
    with pytest.raises(TypeError):
        Fn.detection_report(s, c.long(), c)
    with pytest.raises(TypeError):
        Fn.detection_report(s, c, c, c[:3], 2)
    with pytest.raises(ValueError):
        Fn.detection_report(s, c, c, None, 2)
    with pytest.raises(ValueError):
        Fn.detection_report(s, c, c, c, 65)
    with pytest.raises(ValueError):
        Fn.detection_report(s, c, c, thresholds=[0.1] * 9)
    with pytest.raises(ValueError, match="2\\^20"):
        big = torch.zeros(1, dtype=torch.int32).expand((1 << 20) + 1)            # views of one element
        Fn.detection_report(torch.zeros(1).expand((1 << 20) + 1), big, big)
    with pytest.raises(RuntimeError, match="not on a HIP device.*no CPU fallback"):
        Fn.detection_report(s, c, c)


def _board():
    from lstc_vad_amd import pipeline
    return pipeline._ScoreBoard(None, None, "cpu", 0, 1, None, 100)


def test_report_weights_refusals_come_before_any_launch():
    from lstc_vad_amd import pipeline
    b = _board()
    b._register(1, lambda v: pytest.fail("closure run"), "x")
    b.total = (1 << 20) + 1
    with pytest.raises(ValueError, match="2\\^20"):
        pipeline.ReportWeights().fill(b)
    with pytest.raises(ValueError, match="thresholds"):
        pipeline.ReportWeights(thresholds=[0.1] * 9)
    b = _board()
    for k in range(65):
        b._register(1, lambda v: pytest.fail("closure run"), f"{chr(65 + k % 26)}{chr(97 + k // 26)}_{k}")
    with pytest.raises(ValueError, match="65 classes"):
        pipeline.ReportWeights(group_of=lambda name: name.split("_")[0]).fill(b)
    # a good board: rows -> classes in first-seen order, on top of the inherited counts
    b = _board()
    b._register(2, lambda v: (np.repeat(v, 3), np.array([0, 1, 1, 0, 0, 0.0])), "Arson011_x264")
    b._register(1, lambda v: (np.repeat(v, 2), np.zeros(2)), "Normal_Videos_003_x264")
    b._register(3, lambda v: (np.repeat(v, 1), np.ones(3)), "Arson002_x264")
    w = pipeline.ReportWeights(group_of=pipeline.ucf_class).fill(b)
    assert isinstance(w, pipeline.AucWeights) and w.total == 6 and w.frames == 11 and w.report is None
    assert w.group_names == ["Arson", "Normal"] and w.gid_host.tolist() == [0, 0, 1, 0, 0, 0] and w.gid.dtype == torch.int32
    assert w.pos_host.tolist() == [2, 0, 0, 1, 1, 1] and w.neg_host.tolist() == [1, 3, 2, 0, 0, 0]
    with pytest.raises(ValueError, match="score rows"):
        w.auc(torch.zeros(7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.auc(torch.zeros(6))
    assert pipeline._device_auc_arg(w, False, "x") is w
    with pytest.raises(ValueError, match="return_frames"):
        pipeline._device_auc_arg(w, True, "x")
    plain = pipeline.ReportWeights().fill(b)
    assert plain.gid is None and plain.group_names == []


def test_report_flag_parses_on_every_script():
    from lstc_vad_amd import cli
    for script in cli._FLAGS:
        p = cli.build_parser(script)
        assert p.parse_args([]).report is False and p.parse_args([]).device_auc is False, script
        assert p.parse_args(["--report"]).report is True, script
        assert cli.complete_args(script, Namespace(batch_size=2)).report is False, script
        argv = cli.namespace_to_argv(script, p.parse_args(["--report", "--resident_eval"]))
        assert "--report" in argv and cli.complete_args(script, argv=argv).report is True, script
    from lstc_vad_amd.pipeline import ReportWeights, ucf_class
    w = cli._report_weights(Namespace(report=True), "UCF")
    assert isinstance(w, ReportWeights) and w.group_of is ucf_class and cli._report_weights(Namespace(report=True), "SHT").group_of is None
    assert cli._report_weights(Namespace(report=False), "UCF") is None and cli.report_lines(None) == [] and cli.report_lines(w) == []
