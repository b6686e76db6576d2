"""The detection report on the GPU: ``lstc_det_report`` through the C ABI against its host twin
``metrics.detection_report_weighted`` (integers equal, the AUC bit-equal, the other doubles within a derived bound), the bits'
independence of the launch plan, ``pipeline.ReportWeights`` on the passes of the synthetic world of tests/golden/pipeline_world.py
(through the helpers of tests/test_resident_gpu.py) and ``--report`` on Test/evaluation_UCF.py.

The bound on a double: a group's ``ap``, ``pr_auc`` and the three score sums are sums of m non-negative per-row terms (m rows of the
group carry weight), each formed with at most 3 roundings beyond the ones the twin makes too, added in some fixed order (at most
(m - 1) 2^-53 relative for non-negative terms, whatever the order) and divided once; the twin adds the same terms exactly
(``math.fsum``).  Relative error at most ``(m + 8) 2^-53``."""
import ctypes as C
import math
import os
import struct

import numpy as np
import pytest
import torch

from test_resident_gpu import DEV, _cli, _keys, _models, _no_uploads, _owns, _two, world        # noqa: F401  (world: a fixture)

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53
GUARD = 64
DOUBLES = ("ap", "pr_auc", "sum_s_pos", "sum_s_neg", "sum_sq_err")
WORST = {"ratio": 0.0}                                   # worst |device - twin| / bound seen by this module's kernel tests
# csrc/metrics.hip: 256 rows i per workgroup, chunks of 256 rows j, slices of whole chunks.  Up to 256 rows there is one slice, from
# 257 on the rows j are split (first boundary at row 256); lists of about 12 k rows run slices of two chunks (boundary at row 512)
SIZES = [1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
TH8 = (0.5, 0.25, 0.75, 0.0, 1.0, -1.0, 0.1, 0.999)


def same_bits(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def rows(n, seed, family, wmax=48):
    """Scores of a family, a +0.0 / -0.0 pair, weights 0..wmax, rows of zero weight that carry NaN."""
    rs = np.random.RandomState(seed)
    if family == "continuous":
        s = rs.rand(n).astype(np.float32)
    elif family == "four":
        s = rs.choice(np.array([0.25, 0.5, 0.75, 1.0], np.float32), n)
    else:
        s = np.full(n, 0.25, np.float32)
    pos, neg = rs.randint(0, wmax + 1, n).astype(np.int32), rs.randint(0, wmax + 1, n).astype(np.int32)
    if n >= 2 and family != "equal":
        s[0], s[1] = 0.0, -0.0
        pos[0], neg[0], pos[1], neg[1] = 3, 1, 2, 5
    if n >= 8:
        s[5::7] = np.nan
        pos[5::7] = 0
        neg[5::7] = 0
    return s, pos, neg


def group_ids(n, n_groups, seed, pos):
    """Group ids with an empty group (the last but one), a group without positives (group 1: ``pos`` is edited), rows outside
    every group (id n_groups + 5 and id 0xFFFFFFFF)."""
    rs = np.random.RandomState(seed)
    gid = rs.randint(0, n_groups, n).astype(np.int32)
    if n_groups > 2:
        gid[gid == n_groups - 2] = 0
    pos[gid == 1] = 0
    gid[3::11] = n_groups + 5
    gid[4::13] = -1
    return gid


def run_abi(s, pos, neg, gid, n_groups, th, slices=None):
    """lstc_det_report through the C ABI: records between guard bytes, the workspace (0xFF before the call) too."""
    from lstc_vad_amd import _lib as L
    lib = L.load()
    n = s.size
    ds, dp, dn = (torch.from_numpy(a).to(DEV) for a in (s, pos, neg))
    dg = None if gid is None else torch.from_numpy(gid).to(DEV)
    dt = torch.tensor(th, dtype=torch.float32).to(DEV)
    need, size = int(lib.lstc_det_workspace_bytes(n, n_groups)), C.sizeof(L.DetOut) * n_groups
    ws = torch.full((need + 2 * GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    out = torch.full((size + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    assert out.data_ptr() % 8 == 0
    old = os.environ.pop("LSTC_DET_SLICES", None)
    if slices is not None:
        os.environ["LSTC_DET_SLICES"] = str(slices)
    try:
        L.check(lib.lstc_det_report(L.dev_ptr(ds), L.dev_ptr(dp), L.dev_ptr(dn), None if dg is None else L.dev_ptr(dg), n, n_groups,
                                    L.dev_ptr(dt), len(th), ws.data_ptr() + GUARD, need, out.data_ptr() + GUARD, L.stream_ptr()),
                "lstc_det_report")
        torch.cuda.synchronize()
    finally:
        os.environ.pop("LSTC_DET_SLICES", None)
        if old is not None:
            os.environ["LSTC_DET_SLICES"] = old
    host, wh = out.cpu().numpy(), ws.cpu().numpy()
    assert (host[:GUARD] == 0xAB).all() and (host[GUARD + size:] == 0xAB).all(), "written outside the records"
    assert (wh[:GUARD] == 0xFF).all() and (wh[GUARD + need:] == 0xFF).all(), "written outside the workspace"
    raw = host[GUARD:GUARD + size].tobytes()
    return [L.DetOut.from_buffer_copy(raw[k:k + C.sizeof(L.DetOut)]) for k in range(0, size, C.sizeof(L.DetOut))], raw


def check_against_twin(s, pos, neg, gid, n_groups, th, what, slices=None):
    from lstc_vad_amd.metrics import detection_report_weighted
    want = detection_report_weighted(s, pos, neg, gid, n_groups, th)
    got, raw = run_abi(s, pos, neg, gid, n_groups, th, slices)
    g = np.zeros(s.size, np.int64) if gid is None else gid.astype(np.int64)
    for k, (a, b) in enumerate(zip(got, want)):
        ints = (a.pos, a.neg, a.u2, list(a.tp_at), list(a.fp_at), a.flags, a.reserved)
        assert ints == (b.pos, b.neg, b.u2, b.tp_at, b.fp_at, b.flags, 0), (what, k, ints, b)
        if b.flags or not (b.pos and b.neg):
            assert math.isnan(a.auc) and math.isnan(b.auc), (what, k)
        else:
            assert same_bits(a.auc, b.u2 / (2 * b.pos * b.neg)) and same_bits(a.auc, b.auc), (what, k, a.auc, b.auc)
        tol = (int(((g == k) & ((pos.astype(np.int64) + neg) > 0)).sum()) + 8) * U53
        for f in DOUBLES:
            x, y = getattr(a, f), getattr(b, f)
            if math.isnan(y):
                assert math.isnan(x), (what, k, f, x)
                continue
            ratio = abs(x - y) / (abs(y) * tol) if y else (0.0 if x == 0.0 else math.inf)
            WORST["ratio"] = max(WORST["ratio"], ratio)
            assert ratio <= 1.0, (what, k, f, x, y, ratio)
    return got, raw


def check_against_auc_kernel(s, pos, neg, rec, what):
    """Group 0 of an ungrouped call carries lstc_auc_weighted's integers and its AUC bits."""
    from lstc_vad_amd import functional as Fn
    ref = Fn.read_auc(Fn.weighted_auc(*(torch.from_numpy(a).to(DEV) for a in (s, pos, neg))))
    assert (rec.u2, rec.pos, rec.neg) == (ref.u2, ref.pos, ref.neg), (what, rec.u2, ref.u2)
    assert same_bits(rec.auc, ref.auc) or (math.isnan(rec.auc) and math.isnan(ref.auc)), (what, rec.auc, ref.auc)


@pytest.mark.parametrize("n", SIZES)
def test_kernel_is_the_twin(n):
    for f, family in enumerate(("continuous", "four", "equal")):
        for n_groups in (None, 2, 14, 64):
            s, pos, neg = rows(n, 100 * n + f, family)
            gid = None if n_groups is None else group_ids(n, n_groups, n + f, pos)
            th = TH8 if (f + (n_groups or 0)) % 2 else (0.5,)
            got, _ = check_against_twin(s, pos, neg, gid, n_groups or 1, th, (n, family, n_groups))
            if gid is None:
                check_against_auc_kernel(s, pos, neg, got[0], (n, family))
    print("worst |device - twin| / ((m + 8) 2^-53 |twin|) so far: %.4f" % WORST["ratio"])


def test_one_realistic_size():
    """n = 40 000 (an STN pass over ShanghaiTech has 37 k rows): real-shaped weights - most rows cover 16 label-0 frames; ungrouped
    and in 14 classes."""
    rs = np.random.RandomState(11)
    n = 40000
    s = rs.rand(n).astype(np.float32)
    s[::50] = np.round(s[::50], 1)
    neg = np.full(n, 16, np.int32)
    pos = np.zeros(n, np.int32)
    hot = rs.rand(n) < 0.04
    pos[hot] = rs.randint(1, 17, int(hot.sum()))
    neg[hot] = 16 - pos[hot]
    got, _ = check_against_twin(s, pos, neg, None, 1, (0.5, 0.1), "40 000")
    check_against_auc_kernel(s, pos, neg, got[0], "40 000")
    gid = (np.arange(n) // 97 % 14).astype(np.int32)                       # videos of 97 rows, 14 classes
    check_against_twin(s, pos, neg, gid, 14, TH8, "40 000 in 14 classes")
    print("worst |device - twin| / ((m + 8) 2^-53 |twin|) so far: %.4f" % WORST["ratio"])


def test_flags_and_nan_rows():
    from lstc_vad_amd import _lib as L
    s, pos, neg = rows(1025, 5, "continuous")
    gid = group_ids(1025, 2, 5, pos)
    clean, _ = check_against_twin(s, pos, neg, gid, 2, (0.5,), "NaN on weightless rows only")
    assert clean[0].flags == 0 and clean[1].flags == 0 and np.isnan(s).any()
    bad = int(np.nonzero((gid == 0) & (pos > 0))[0][7])
    s[bad] = np.nan                                                       # a weighted row of group 0 with a NaN score
    got, _ = check_against_twin(s, pos, neg, gid, 2, (0.5,), "NaN on a weighted row")
    assert got[0].flags == L.DET_NAN_SCORE and got[1].flags == 0
    assert all(math.isnan(getattr(got[0], f)) for f in DOUBLES + ("auc",)) and not math.isnan(got[1].sum_s_neg)
    assert (got[0].pos, got[0].neg) == (clean[0].pos, clean[0].neg) and got[0].tp_at[0] <= clean[0].tp_at[0]
    whole, _ = check_against_twin(s, pos, neg, None, 1, TH8, "NaN on a weighted row, ungrouped")
    assert whole[0].flags == L.DET_NAN_SCORE
    check_against_auc_kernel(s, pos, neg, whole[0], "NaN on a weighted row")
    s, pos, neg = rows(4099, 6, "four")
    s[np.isnan(s)] = 0.5
    pos[:], neg[:] = 1 << 13, 1 << 13                                     # 4099 * 2^14 frames > 2^26
    got, _ = run_abi(s, pos, neg, None, 1, (0.5,))
    assert got[0].flags == L.DET_TOO_MANY_FRAMES and (got[0].pos, got[0].neg) == (4099 << 13, 4099 << 13)
    assert all(math.isnan(getattr(got[0], f)) for f in DOUBLES + ("auc",))
    pos[:], neg[:] = 8186, 8186                                           # 4099 * 16372 <= 2^26: not flagged, and exact
    got, _ = check_against_twin(s, pos, neg, None, 1, (0.5,), "at the frame limit")
    check_against_auc_kernel(s, pos, neg, got[0], "at the frame limit")


@pytest.mark.parametrize("n,n_groups", [(257, None), (4099, 14), (12461, None)])
def test_bits_do_not_depend_on_the_launch_plan(n, n_groups):
    """One slice, seven slices, as many as there are chunks, and the launcher's own plan: the same record bytes."""
    s, pos, neg = rows(n, 9, "continuous" if n_groups else "four", 400)
    gid = None if n_groups is None else group_ids(n, n_groups, 9, pos)
    plans = [run_abi(s, pos, neg, gid, n_groups or 1, TH8, slices)[1] for slices in (None, 1, 7, 64)]
    assert all(p == plans[0] for p in plans[1:])
    check_against_twin(s, pos, neg, gid, n_groups or 1, TH8, (n, "one slice"), slices=1)


def test_functional_wrapper():
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.metrics import detection_report_weighted
    s, pos, neg = rows(1000, 3, "four")
    gid = group_ids(1000, 3, 3, pos)
    ds, dp, dn, dg = (torch.from_numpy(a).to(DEV) for a in (s, pos, neg, gid))
    rec = Fn.detection_report(ds, dp, dn, dg, 3, (0.5, 0.25))
    assert rec.is_cuda and rec.dtype == torch.int64 and tuple(rec.shape) == (3, 26)
    out = torch.empty_like(rec)
    assert Fn.detection_report(ds, dp, dn, dg, 3, torch.tensor([0.5, 0.25], device=DEV), out=out) is out and torch.equal(out, rec)
    got, want = Fn.read_detection_report(rec), detection_report_weighted(s, pos, neg, gid, 3, (0.5, 0.25))
    assert [(a.pos, a.neg, a.u2, list(a.tp_at)) for a in got] == [(b.pos, b.neg, b.u2, b.tp_at) for b in want]
    if hasattr(torch, "uint32"):
        again = Fn.detection_report(ds, dp.view(torch.uint32), dn.view(torch.uint32), dg.view(torch.uint32), 3, (0.5, 0.25))
        assert torch.equal(again, rec)
    one = Fn.read_detection_report(Fn.detection_report(ds, dp, dn))
    assert len(one) == 1 and one[0].pos == int(pos.sum())


# ---------------------------------------------------------------------------------------------------- the passes
def _passes(world, dialect):
    from lstc_vad_amd import pipeline
    if dialect == "UCF":
        feats, txt, masks, keys = world["ucf_feats"], world["ucf_test"], world["ucf_gt"], _keys(world["ucf_test"], True)
        make = lambda r, w: pipeline.ResidentSet.from_archive(feats, keys, DEV, n_patch=9, view=True, owns=_owns(r, w))
        return "ucf", (feats, txt, masks, 2, 9), dict(pool_sequences=20), make, pipeline.ucf_class
    feats, txt, masks, keys = world["sht_feats"], world["sht_test"], world["sht_masks"], _keys(world["sht_test"])
    make = lambda r, w: pipeline.ResidentSet.from_archive(feats, keys, DEV, n_patch=16, owns=_owns(r, w))
    return "ltn", (feats, txt, masks, 3, 16), dict(pool_sequences=5), make, (lambda name: name.split("_")[0])      # SHT: the scene


def _report_is_the_twin_on_the_frames(w, fs, fl, what):
    """``w.report`` against ``metrics.detection_report_weighted`` on the frames of the host route (every frame a row of weight 1)."""
    from lstc_vad_amd.metrics import detection_report_weighted
    fl = fl.astype(np.int64)
    weight = w.pos_host + w.neg_host
    tol = (int((weight > 0).sum()) + 8) * U53
    pairs = [(w.report.overall, detection_report_weighted(fs, fl, 1 - fl, thresholds=w.thresholds)[0])]
    if w.group_names:
        frame_gid = np.repeat(w.gid_host, weight)             # a video's frames are contiguous and its rows share a class
        pairs += list(zip(w.report.groups, detection_report_weighted(fs, fl, 1 - fl, frame_gid, len(w.group_names), w.thresholds)))
    assert len(pairs) == 1 + len(w.group_names)
    for a, b in pairs:
        assert (a.pos, a.neg, a.u2, list(a.tp_at), list(a.fp_at), a.flags) == (b.pos, b.neg, b.u2, b.tp_at, b.fp_at, 0), (what, b)
        for f in DOUBLES + ("auc",):
            x, y = getattr(a, f), getattr(b, f)
            assert (math.isnan(x) and math.isnan(y)) or abs(x - y) <= tol * abs(y), (what, f, x, y)


@pytest.mark.parametrize("dialect", ["SHT", "UCF"])
def test_report_weights_on_the_passes(world, dialect, monkeypatch):
    from lstc_vad_amd import pipeline
    which, (feats, txt, masks, part_len, n_patch), kw, make, group_of = _passes(world, dialect)
    enc, head = _models(world, which)

    def ev(rs=None, masks=masks, **more):
        return pipeline.evaluate_auc(enc, head, "LTN", dialect, feats, txt, masks, part_len, n_patch, resident=rs, **kw, **more)
    whole = make(None, None)
    for route, rs_of in (("host-fed", lambda r, w: None), ("resident", lambda r, w: whole if w is None else make(r, w))):
        _, fs, fl = ev(rs_of(None, None), return_frames=True)
        plain = ev(rs_of(None, None), device_auc=True)
        w = pipeline.ReportWeights(group_of=group_of, thresholds=(0.5, 0.3))
        got = ev(rs_of(None, None), device_auc=w)
        assert isinstance(got, float) and same_bits(got, plain) and same_bits(got, w.report.overall.auc), (dialect, route, got, plain)
        assert len(w.group_names) >= 2 and w.report.names == w.group_names and w.frames == fs.size
        _report_is_the_twin_on_the_frames(w, fs, fl, (dialect, route))
        first = w.report
        two = _two(lambda r, n, ex: ev(rs_of(r, n), rank=r, world=n, exchange=ex, device_auc=w))
        assert same_bits(two, plain) and w.report is not first
        _report_is_the_twin_on_the_frames(w, fs, fl, (dialect, route, "two ranks"))
        if dialect == "UCF":
            assert w.group_names == ["Arson", "Normal", "RoadAccidents"] and not math.isnan(w.report.normal_far())
            assert len(w.report.each_part_lines()) == 3 and w.report.each_part_lines()[1].startswith("Normal: \tAUC \tNone")
        if route == "resident":
            # filled weights over a resident set: no mask file or ground-truth archive is opened, nothing is uploaded
            with monkeypatch.context() as m:
                _no_uploads(m)
                again = ev(whole, masks=os.path.join(world["root"], "no_such_masks") + os.sep, device_auc=w)
            assert same_bits(again, plain)
            _report_is_the_twin_on_the_frames(w, fs, fl, (dialect, route, "second evaluation"))
    ungrouped = pipeline.ReportWeights()
    assert same_bits(ev(device_auc=ungrouped), plain) and ungrouped.report.groups == [] and ungrouped.report.overall.pos == int(fl.sum())
    with pytest.raises(ValueError, match="return_frames"):
        ev(device_auc=pipeline.ReportWeights(), return_frames=True)


# ---------------------------------------------------------------------------------------------------- the command line
def test_report_flag_on_the_ucf_evaluation_script(world):
    """Test/evaluation_UCF.py with and without --report: the same ``auc = `` line up to the bar of the device AUC (K <= 48 score
    rows) - the very number of the device route - followed by the report lines of the same pass run here."""
    from lstc_vad_amd import cli, pipeline
    ev = ["--d_model", "32", "--temporal_n_head", "2", "--temporal_d_k", "16", "--temporal_d_v", "16", "--temporal_n_hidden", "64",
          "--temporal_MHA_layerNorm", "--temporal_FFN_layerNorm", "--relative_position_encoding", "--n_patch", "9",
          "--dataset_path", world["ucf_feats"], "--testing_txt", world["ucf_test"], "--test_mask_path", world["ucf_gt"],
          "--temporal_model_path", world["ltn_ucf_enc.ckpt"], "--classifier_model_path", world["ltn_ucf_cls.ckpt"]]
    runs = []
    for flag in ([], ["--report"]):
        e = _cli("Test", "evaluation_UCF.py", ev + flag)
        assert e.returncode == 0, e.stderr[-2000:]
        runs.append(e.stdout.splitlines())
    (plain,), with_report = [l for l in runs[0] if l.startswith("auc = ")], runs[1]
    at = [i for i, l in enumerate(with_report) if l.startswith("auc = ")]
    assert len(at) == 1 and not any(l.startswith("report:") for l in runs[0])
    assert runs[0][:runs[0].index(plain)] == with_report[:at[0]]                      # nothing printed before it changes
    assert abs(float(plain.split("auc = ")[-1]) - float(with_report[at[0]].split("auc = ")[-1])) <= (48 + 4) * 2.0 ** -52
    enc, head = _models(world, "ucf")
    w = pipeline.ReportWeights(group_of=pipeline.ucf_class)
    auc = pipeline.evaluate_auc(enc, head, "LTN", "UCF", world["ucf_feats"], world["ucf_test"], world["ucf_gt"], 2, 9, device_auc=w)
    assert with_report[at[0]] == "auc =  " + str(auc)
    lines = with_report[at[0] + 1:]
    assert lines == cli.report_lines(w) and len(lines) == 1 + 3 + 1
    assert lines[0].startswith("report: AUC ") and " AP " in lines[0] and " PR-AUC " in lines[0] and " FAR@0.5 " in lines[0] and " GAP " in lines[0]
    assert float(lines[0].split("AUC ")[1].split(",")[0]) == float("%.6f" % w.report.overall.auc)
    assert lines[1:4] == w.report.each_part_lines() and lines[4] == "report: normal FAR {}, mAP {:.6f}".format(w.report.normal_far(), w.report.mean_ap())


def test_report_flag_in_the_training_loop(world, tmp_path):
    """Train/temporal_transformer_shanghaitech.py with --resident_eval --report: the in-loop evaluation logs its AUC lines as before
    and, after them, the overall report line of the test list, whose AUC is the logged test AUC."""
    model = ["--d_model", "32", "--n_head", "2", "--d_k", "16", "--d_v", "16", "--n_hidden", "64", "--MHA_layerNorm", "--FFN_layerNorm",
             "--relative_position_encoding", "--part_len", "3"]
    save = str(tmp_path / "ck") + os.sep
    os.makedirs(save)
    train = model + ["--dataset_path", world["sht_feats"], "--training_txt", world["sht_train"], "--testing_txt", world["sht_test"],
                     "--test_mask_dir", world["sht_masks"], "--batch_size", "2", "--part_num", "3", "--n_patch", "16", "--load_model",
                     "--lr_encoder", "0", "--lr_classifier", "0", "--epochs", "1", "--inter_epoch", "1", "--seed", "3",
                     "--save_threshold", "0", "--load_temporal_model_path", world["ltn_sht_enc.ckpt"], "--load_classifier_model_path",
                     world["ltn_sht_cls.ckpt"], "--saved_prefix", "pre_", "--model_save_dir", save, "--log_dir", str(tmp_path / "log"),
                     "--resident_eval", "--report"]
    r = _cli("Train", "temporal_transformer_shanghaitech.py", train)
    assert r.returncode == 0, r.stderr[-2500:]
    log = [l.split(": ", 1)[-1] for l in r.stderr.splitlines()]
    auc_at = [i for i, l in enumerate(log) if "now test_AUC is" in l]
    rep_at = [i for i, l in enumerate(log) if l.startswith("report: AUC ")]
    assert len(auc_at) == 1 and len(rep_at) == 1 and rep_at[0] > auc_at[0], log[-12:]
    test_auc = float(log[auc_at[0]].split("now test_AUC is")[1].split()[0])
    assert float(log[rep_at[0]].split("AUC ")[1].split(",")[0]) == float("%.6f" % test_auc)
    assert " AP " in log[rep_at[0]] and " FAR@0.5 " in log[rep_at[0]] and not any(l.startswith("report: normal FAR") for l in log)
