"""Evaluation and label passes fed from the host (the default arguments of pipeline.evaluate_auc / generate_pseudo_labels: every
video read from the archive, uploaded and cut into sequences per pass) against the same passes on a pipeline.ResidentSet
(``resident=``: the set uploaded once, every part a span of the HBM bank), and lstc_segment_mean alone.  A measurement tool, not on
the product path.

Workloads (synthetic features, the reference's sizes):
  SHT-shaped   ``--sht_videos`` (199) videos of ``--sht_clips`` (190 on average, 60 % .. 140 %) clips, P = 16, d = 2048, LTN part_len 3:
               evaluate_auc (rewindowed tail) and generate_pseudo_labels (short tail)
  UCF-shaped   ``--ucf_videos`` (290) videos of ``--ucf_clips`` (100 on average) clips, P = 9, d = 2048, 32 bins, part_len 2
each in fp32 and in bf16 mode; the label passes run with threshold 0, so that their rows are the scores themselves and ``max |diff|``
is a score difference in every row of the report.  The archives are directories of .npy files (memory-mapped reads: the host-fed arm runs from the page
cache after the warm-up round, its best case).  The arms run interleaved, ``--repeats`` (5) rounds after ``--warmup`` (1); each time is
a host clock around the pass and a device synchronise.  The upload of the resident set is timed once and reported apart.
Run on an MI355X:  python tools/resident_eval_time.py --work /tmp/resident_eval [--out profiles/resident_eval.txt]

``--device_auc`` measures the device AUC instead (profiles/device_auc.txt): evaluate_auc over the same resident sets with and
without ``device_auc=`` (one filled pipeline.AucWeights per pass), interleaved; the host tail the flag replaces (the ``.cpu()`` copy
of the flat score vector, every ``finish`` closure and metrics.roc_auc - the code of ``_ScoreBoard.results`` and ``_auc_of``), timed
on the same flat vector in the same process; and the event-timed kernel pair of lstc_auc_weighted on the passes' own weights.

``--report`` measures the detection report (profiles/detection_report.txt): evaluate_auc over the same resident sets with a filled
pipeline.ReportWeights (13 / 14 classes) against the route that gives the same numbers without it - ``return_frames=True``, then
the frame-level functions of lstc_vad_amd.metrics on the frames, overall and by class - interleaved; and the event-timed launches
of lstc_det_report, ungrouped and grouped, beside lstc_auc_weighted on the same rows."""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstc_vad_amd import functional as Fn                            # noqa: E402
from lstc_vad_amd import pipeline, scoring                           # noqa: E402
from lstc_vad_amd.models import Classifier, Encoder                  # noqa: E402

SEG, D = 16, 2048


def _write(root, name, n_videos, mean_clips, P, ucf, seed):
    """A directory archive, a test list, a train list and the masks of the abnormal half -> dict of paths, clip counts."""
    rs, gen = np.random.RandomState(seed), np.random.default_rng(seed)
    feats = os.path.join(root, name + "_feats")
    masks = os.path.join(root, name + "_masks") + os.sep
    os.makedirs(feats, exist_ok=True)
    os.makedirs(masks, exist_ok=True)
    counts = [max(4, int(mean_clips * (0.6 + 0.8 * rs.rand()))) for _ in range(n_videos)]
    test, train = [], []
    for i, n in enumerate(counts):
        abnormal = i % 2 == 1
        key = (("Abuse%03d_x264" if abnormal else "Normal_Videos%03d_x264") % i) if ucf else "%02d_%04d" % (1 + i % 13, i)
        np.save(os.path.join(feats, key + ".npy"), 0.5 * np.maximum(gen.standard_normal((n, P, D), dtype=np.float32), 0))
        n_frames = n * SEG + 7
        if abnormal:
            m = np.zeros(n_frames)
            m[n_frames // 3: n_frames // 2] = 1.0
            np.save(os.path.join(masks, key + ".npy"), m)
        if ucf:
            test.append(f"Dir/{key}.mp4 {n_frames} {'Abuse' if abnormal else 'Normal'} -1 -1 -1 -1 \n")
            train.append(f"Dir/{key}.mp4 {n_frames} \n")
        else:
            test.append(f"{key},{int(abnormal)},{-1 if abnormal else n_frames}\n")
            train.append(f"{key},{int(abnormal)}\n")
    paths = {"feats": feats, "masks": masks.rstrip(os.sep) if ucf else masks, "test": os.path.join(root, name + "_test.txt"),
             "train": os.path.join(root, name + "_train.txt")}
    open(paths["test"], "w").write("".join(test))
    open(paths["train"], "w").write("".join(train))
    return paths, counts


def _time_arms(arms, warmup, repeats):
    times, last = {k: [] for k in arms}, {}
    for r in range(warmup + repeats):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(time.perf_counter() - t0)
    return times, last


def _resident_world(a, dev, lines):
    """The two lists, their models and their resident sets, as the --device_auc and --report arms use them."""
    from lstc_vad_amd.models import Regressor
    sht, sht_counts = _write(a.work, "sht", a.sht_videos, a.sht_clips, 16, False, 1)
    ucf, ucf_counts = _write(a.work, "ucf", a.ucf_videos, a.ucf_clips, 9, True, 2)
    wide = dict(n_layers=3, n_head=8, d_k=256, d_v=256, d_model=D, d_inner=4096, FFN_layerNorm=True, weight_init=False)
    ltn = lambda depth: Encoder(MHA_layerNorm=True, relative_pe=True, window_size=4, window_depth=depth, **wide).to(dev).eval()
    models = {("sht", "LTN"): (ltn(3), Classifier(D).to(dev).eval()), ("ucf", "LTN"): (ltn(2), Classifier(D).to(dev).eval()),
              ("sht", "STN"): (Encoder(**wide).to(dev).eval(), Regressor(D).to(dev).eval())}
    keys = lambda txt, is_ucf: [(l.split(" ")[0].split("/")[-1].split(".")[0] if is_ucf else l.split(",")[0])
                                for l in open(txt).read().splitlines()]
    sets = {"sht": pipeline.ResidentSet.from_archive(sht["feats"], keys(sht["test"], False), dev, n_patch=16),
            "ucf": pipeline.ResidentSet.from_archive(ucf["feats"], keys(ucf["test"], True), dev, n_patch=9, view=True)}
    lines.append(f"SHT-shaped: {a.sht_videos} videos, {sum(sht_counts)} clips, P = 16, d = {D}, part_len 3; UCF-shaped: {a.ucf_videos} "
                 f"videos, {sum(ucf_counts)} clips, P = 9, 32 bins, part_len 2; both resident (pipeline.ResidentSet)")
    return sht, ucf, models, sets


def _event_time(fn, warm=3, runs=9):
    """Median seconds of ``fn()`` between two events on the current stream."""
    ts = []
    for _ in range(warm + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(ts[warm:])


UCF_CLASSES = ["Abuse", "Arrest", "Arson", "Assault", "Burglary", "Explosion", "Fighting", "RoadAccidents", "Robbery", "Shooting",
               "Shoplifting", "Stealing", "Vandalism"]


def _class_of(name):
    """The timing lists name their abnormal videos Abuse<i> / <scene>_<i>: spread them over 13 classes (plus Normal for UCF), the
    class count of UCF-Crime and of ShanghaiTech's scenes."""
    cls = pipeline.ucf_class(name)
    if not cls:                                   # "<scene>_<i>": the scene
        return name.split("_")[0]
    if cls == "Normal":
        return cls
    return UCF_CLASSES[int(name[len(cls):len(cls) + 3]) % 13]


def _report_arm(a, dev, lines, res):
    """The --report arm (see the module docstring)."""
    from lstc_vad_amd import metrics
    sht, ucf, models, sets = _resident_world(a, dev, lines)
    lines.append(f"evaluate_auc, medians of {a.repeats} interleaved runs after {a.warmup} warm-up round(s) (min .. max): report = "
                 "evaluate_auc(resident=, device_auc=ReportWeights(group_of=)) with filled weights - AUC, AP, PR-AUC, FAR, GAP overall and "
                 "per class on the device; host = what gives the same numbers today: evaluate_auc(resident=, return_frames=True), then "
                 "cal_AP, cal_pr_auc, cal_false_alarm and cal_score_gap on all frames and eval_each_part on the frames by class "
                 "(lstc_vad_amd.metrics, numpy)")
    weights = {}
    for mode, tag, kind in (("fp32", "sht", "LTN"), ("fp32", "ucf", "LTN"), ("bf16", "sht", "LTN"), ("bf16", "ucf", "LTN"),
                            ("fp32", "sht", "STN")):
        W, P, part_len, dataset = (sht, 16, 3, "SHT") if tag == "sht" else (ucf, 9, 2, "UCF")
        enc, head = models[tag, kind]
        w = weights.setdefault((tag, kind), pipeline.ReportWeights(group_of=_class_of))
        Fn.set_compute_dtype(mode)
        try:
            ev = lambda **kw: pipeline.evaluate_auc(enc, head, kind, dataset, W["feats"], W["test"], W["masks"], part_len, P,
                                                    resident=sets[tag], **kw)
            ev(device_auc=w)                                        # fills the weights: built once, outside the timed runs
            frame_gid = np.repeat(w.gid_host, w.pos_host + w.neg_host)

            def host():
                auc, fs, fl = ev(return_frames=True)
                out = [auc, metrics.cal_AP(fs, fl), metrics.cal_pr_auc(fs, fl), metrics.cal_false_alarm(fs, fl), metrics.cal_score_gap(fs, fl)]
                labels = {c: fl[frame_gid == k] for k, c in enumerate(w.group_names)}
                scores = {c: fs[frame_gid == k] for k, c in enumerate(w.group_names)}
                return out + list(metrics.eval_each_part(labels, scores, logger=_Quiet))

            def report():
                auc = ev(device_auc=w)
                r = w.report
                return [auc, r.overall.ap, r.overall.pr_auc, r.far(), r.gap(), r.normal_far(), r.mean_ap()]
            times, last = _time_arms({"host": host, "report": report}, a.warmup, a.repeats)
        finally:
            Fn.set_compute_dtype("fp32")
        diff = max(abs(x - y) for x, y in zip(last["host"], last["report"]) if x == x or y == y)
        row = {"mode": mode, "set": tag, "net": kind, "rows": w.total, "frames": w.frames, "classes": len(w.group_names), "max_diff": diff}
        for arm in ("host", "report"):
            row[arm] = {"median_s": statistics.median(times[arm]), "min_s": min(times[arm]), "max_s": max(times[arm])}
        row["host_over_report"] = row["host"]["median_s"] / row["report"]["median_s"]
        res["rows"].append(row)
        ms = lambda r: f"{r['median_s'] * 1e3:8.2f} ms ({r['min_s'] * 1e3:.2f} .. {r['max_s'] * 1e3:.2f})"
        lines.append(f"  {mode:5s} {tag} {kind} {w.total:6d} rows {w.frames:7d} frames {len(w.group_names):2d} classes | host {ms(row['host'])} | "
                     f"report {ms(row['report'])} | host / report {row['host_over_report']:.3f} | max |diff| of the 7 numbers {diff:.1e}")
    # the launches alone, event-timed, on the passes' own weights and classes, next to lstc_auc_weighted on the same rows
    gen = torch.Generator().manual_seed(5)
    for what, w in (("UCF parts", weights["ucf", "LTN"]), ("SHT parts", weights["sht", "LTN"]), ("SHT clips", weights["sht", "STN"])):
        n = w.total
        sc = torch.rand(n, generator=gen).to(dev)
        th = torch.tensor([0.5], dtype=torch.float32).to(dev)
        one = Fn.detection_report(sc, w.pos, w.neg, thresholds=th)
        many = Fn.detection_report(sc, w.pos, w.neg, w.gid, len(w.group_names), th)
        auc = Fn.weighted_auc(sc, w.pos, w.neg)
        t_one = _event_time(lambda: Fn.detection_report(sc, w.pos, w.neg, thresholds=th, out=one))
        t_many = _event_time(lambda: Fn.detection_report(sc, w.pos, w.neg, w.gid, len(w.group_names), th, out=many))
        t_auc = _event_time(lambda: Fn.weighted_auc(sc, w.pos, w.neg, out=auc))
        busy = int((np.add.reduceat(w.pos_host, np.arange(0, n, 256)) > 0).sum())
        pairs = busy * 256 * n
        res["rows"].append({"kernel": "lstc_det_report", "shape": what, "n": n, "ungrouped_us": t_one * 1e6, "grouped_us": t_many * 1e6,
                            "classes": len(w.group_names), "lstc_auc_weighted_us": t_auc * 1e6, "row_blocks_with_positives": busy})
        lines.append(f"  lstc_det_report, {what:9s}: n = {n:6d}, {busy} of {(n + 255) // 256} blocks of 256 rows hold a positive frame: "
                     f"{t_one * 1e6:.1f} us ungrouped ({pairs / t_one * 1e-12:.2f} T pairs/s), {t_many * 1e6:.1f} us in {len(w.group_names)} "
                     f"classes; lstc_auc_weighted on the same rows {t_auc * 1e6:.1f} us (memset + two launches / two launches, event-timed, "
                     "medians of 9)")


class _Quiet:
    info = staticmethod(lambda line: None)


def _device_auc_report(a, dev, lines, res):
    """The --device_auc report (see the module docstring)."""
    sht, ucf, models, sets = _resident_world(a, dev, lines)
    lines.append(f"evaluate_auc, medians of {a.repeats} interleaved runs after {a.warmup} warm-up round(s) (min .. max): resident = "
                 "evaluate_auc(resident=) as it stands, + device_auc = the same call with a filled AucWeights; host tail = .cpu() of the "
                 "flat vector + every finish closure + metrics.roc_auc, on the pass's own flat vector, same process")
    weights = {}
    for mode, tag, kind in (("fp32", "sht", "LTN"), ("fp32", "ucf", "LTN"), ("bf16", "sht", "LTN"), ("bf16", "ucf", "LTN"),
                            ("fp32", "sht", "STN")):
        W, P, part_len, dataset = (sht, 16, 3, "SHT") if tag == "sht" else (ucf, 9, 2, "UCF")
        enc, head = models[tag, kind]
        w = weights.setdefault((tag, kind), pipeline.AucWeights())
        Fn.set_compute_dtype(mode)
        try:
            ev = lambda **kw: pipeline.evaluate_auc(enc, head, kind, dataset, W["feats"], W["test"], W["masks"], part_len, P,
                                                    resident=sets[tag], **kw)
            ev(device_auc=w)                                        # fills the weights: built once, outside the timed runs
            arms = {"resident": lambda: ev(), "+ device_auc": lambda: ev(device_auc=w)}
            times, last = _time_arms(arms, a.warmup, a.repeats)
            # the host tail on this pass's flat vector: what _ScoreBoard.results and _auc_of do behind the all-reduce
            seen = {}
            orig = pipeline._ScoreBoard.flat_scores

            def spy(board):
                seen["board"], seen["flat"] = board, orig(board)
                return seen["flat"]
            pipeline._ScoreBoard.flat_scores = spy
            try:
                ev()
            finally:
                pipeline._ScoreBoard.flat_scores = orig
            board, flat = seen["board"], seen["flat"]

            def tail():
                host = flat.cpu().numpy()
                return pipeline._auc_of([finish(host[off:off + n]) for off, n, finish in board.items], False)
            t_tail, _ = _time_arms({"tail": tail}, a.warmup, a.repeats)
        finally:
            Fn.set_compute_dtype("fp32")
        row = {"mode": mode, "set": tag, "net": kind, "rows": w.total, "frames": w.frames,
               "auc_diff": abs(last["resident"] - last["+ device_auc"])}
        for arm, t in (("resident", times["resident"]), ("device_auc", times["+ device_auc"]), ("host_tail", t_tail["tail"])):
            row[arm] = {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t)}
        row["resident_over_device_auc"] = row["resident"]["median_s"] / row["device_auc"]["median_s"]
        res["rows"].append(row)
        ms = lambda r: f"{r['median_s'] * 1e3:8.2f} ms ({r['min_s'] * 1e3:.2f} .. {r['max_s'] * 1e3:.2f})"
        lines.append(f"  {mode:5s} {tag} {kind} evaluate_auc  {w.total:6d} rows {w.frames:7d} frames | resident {ms(row['resident'])} | "
                     f"+ device_auc {ms(row['device_auc'])} | resident / device_auc {row['resident_over_device_auc']:.3f} | host tail "
                     f"{ms(row['host_tail'])} | |AUC diff| {row['auc_diff']:.1e}")
    # the kernel pair alone, event-timed, on the passes' own weights; 9 280 rows: the UCF pass's rows split into their two bins
    wu, wl, ws = weights["ucf", "LTN"], weights["sht", "LTN"], weights["sht", "STN"]
    half = lambda v: np.stack([v // 2, v - v // 2], 1).reshape(-1)
    shaped = [("UCF bins", half(wu.pos_host), half(wu.neg_host)), ("SHT parts", wl.pos_host, wl.neg_host),
              ("SHT clips", ws.pos_host, ws.neg_host)]
    gen = torch.Generator().manual_seed(5)
    for what, pos, neg in shaped:
        n = int(pos.shape[0])
        sc = torch.rand(n, generator=gen).to(dev)
        dp, dn = torch.from_numpy(pos.astype(np.int32)).to(dev), torch.from_numpy(neg.astype(np.int32)).to(dev)
        out = Fn.weighted_auc(sc, dp, dn)
        ts = []
        for _ in range(3 + 9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            Fn.weighted_auc(sc, dp, dn, out=out)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        t = statistics.median(ts[3:])
        rec = Fn.read_auc(out)
        busy = int((np.add.reduceat(pos, np.arange(0, n, 256)) > 0).sum())
        res["rows"].append({"kernel": "lstc_auc_weighted", "shape": what, "n": n, "median_us": t * 1e6, "pos": rec.pos, "neg": rec.neg,
                            "row_blocks_with_positives": busy})
        lines.append(f"  lstc_auc_weighted, {what:9s}: n = {n:6d}, P = {rec.pos}, N = {rec.neg}, {busy} of {(n + 255) // 256} blocks of 256 rows "
                     f"hold a positive frame: {t * 1e6:.1f} us for the two launches (event-timed, median of 9)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--work", required=True, help="scratch directory for the synthetic archives (removed afterwards)")
    ap.add_argument("--sht_videos", type=int, default=199)
    ap.add_argument("--sht_clips", type=int, default=190)
    ap.add_argument("--ucf_videos", type=int, default=290)
    ap.add_argument("--ucf_clips", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device_auc", action="store_true", help="the device-AUC report instead (profiles/device_auc.txt)")
    ap.add_argument("--report", action="store_true", help="the detection-report arm instead (profiles/detection_report.txt)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("resident_eval_time.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    os.makedirs(a.work, exist_ok=True)
    lines, res = [], {"repeats": a.repeats, "rows": []}
    try:
        if a.device_auc:
            _device_auc_report(a, dev, lines, res)
            return _finish(a, lines, res)
        if a.report:
            _report_arm(a, dev, lines, res)
            return _finish(a, lines, res)
        sht, sht_counts = _write(a.work, "sht", a.sht_videos, a.sht_clips, 16, False, 1)
        ucf, ucf_counts = _write(a.work, "ucf", a.ucf_videos, a.ucf_clips, 9, True, 2)
        head = Classifier(D).to(dev).eval()
        encs = {"sht": Encoder(n_layers=3, n_head=8, d_k=256, d_v=256, d_model=D, d_inner=4096, MHA_layerNorm=True, FFN_layerNorm=True,
                               relative_pe=True, window_size=4, window_depth=3, weight_init=False).to(dev).eval(),
                "ucf": Encoder(n_layers=3, n_head=8, d_k=256, d_v=256, d_model=D, d_inner=4096, MHA_layerNorm=True, FFN_layerNorm=True,
                               relative_pe=True, window_size=4, window_depth=2, weight_init=False).to(dev).eval()}
        keys = lambda txt, is_ucf: [(l.split(" ")[0].split("/")[-1].split(".")[0] if is_ucf else l.split(",")[0])
                                    for l in open(txt).read().splitlines()]
        sets, upload = {}, {}
        for tag, W, P, is_ucf, gen_patch in (("sht", sht, 16, False, None), ("ucf", ucf, 9, True, 9)):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            sets[tag, "ev"] = pipeline.ResidentSet.from_archive(W["feats"], keys(W["test"], is_ucf), dev, n_patch=P, view=is_ucf)
            torch.cuda.synchronize(); upload[tag] = time.perf_counter() - t0
            # the label pass walks the same videos: it shares the bank (SHT generators score every stored patch: the same P here)
            sets[tag, "gen"] = sets[tag, "ev"]
        lines.append(f"SHT-shaped: {a.sht_videos} videos, {sum(sht_counts)} clips, P = 16, d = {D}, LTN part_len 3 "
                     f"({sets['sht', 'ev'].bank.numel() * 4 / 2**30:.2f} GiB, uploaded once in {upload['sht']:.2f} s); "
                     f"UCF-shaped: {a.ucf_videos} videos, {sum(ucf_counts)} clips, P = 9, 32 bins, part_len 2 "
                     f"({sets['ucf', 'ev'].bank.numel() * 4 / 2**30:.2f} GiB, uploaded once in {upload['ucf']:.2f} s)")
        lines.append(f"medians of {a.repeats} interleaved runs after {a.warmup} warm-up round(s) (min .. max = the spread); clips/s = clips of "
                     "the list / median")
        for mode in ("fp32", "bf16"):
            Fn.set_compute_dtype(mode)
            try:
                for tag, W, P, part_len, dataset, counts in (("sht", sht, 16, 3, "SHT", sht_counts), ("ucf", ucf, 9, 2, "UCF", ucf_counts)):
                    enc = encs[tag]
                    ev = lambda rs, ragged=False: pipeline.evaluate_auc(enc, head, "LTN", dataset, W["feats"], W["test"], W["masks"], part_len,
                                                                        P, return_frames=True, resident=rs, ragged=ragged)
                    gen = lambda rs, ragged=False: pipeline.generate_pseudo_labels(enc, head, "LTN", dataset, W["feats"], W["train"], 0.0,
                                                                                   part_len=part_len, n_patch=P, d_model=D, resident=rs,
                                                                                   ragged=ragged)
                    passes = [("evaluate_auc", ev, sets[tag, "ev"], False)]
                    passes.append(("generate_pseudo_labels", gen, sets[tag, "gen"], False))
                    if tag == "sht":            # the short tail parts of the label pass: all lengths in shared chunks
                        passes.append(("generate_pseudo_labels ragged='unpadded'", gen, sets[tag, "gen"], "unpadded"))
                    for what, fn, rs, ragged in passes:
                        arms = {"host-fed": lambda fn=fn, ragged=ragged: fn(None, ragged), "resident": lambda fn=fn, rs=rs, ragged=ragged: fn(rs, ragged)}
                        times, last = _time_arms(arms, a.warmup, a.repeats)
                        if what == "evaluate_auc":
                            diff = float(np.abs(last["host-fed"][1] - last["resident"][1]).max())
                        else:
                            diff = max(float(np.abs(last["host-fed"][k] - last["resident"][k]).max()) for k in last["host-fed"])
                        row = {"mode": mode, "set": tag, "pass": what, "clips": int(sum(counts)), "max_abs_diff": diff}
                        for arm in arms:
                            t = times[arm]
                            row[arm] = {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t),
                                        "clips_per_s": sum(counts) / statistics.median(t)}
                        row["host_over_resident"] = row["host-fed"]["median_s"] / row["resident"]["median_s"]
                        res["rows"].append(row)
                        lines.append(f"  {mode:5s} {tag} {what:42s} host-fed {row['host-fed']['median_s'] * 1e3:9.1f} ms "
                                     f"({row['host-fed']['min_s'] * 1e3:.1f} .. {row['host-fed']['max_s'] * 1e3:.1f}) = "
                                     f"{row['host-fed']['clips_per_s'] / 1e3:7.1f} k clips/s | resident {row['resident']['median_s'] * 1e3:9.1f} ms "
                                     f"({row['resident']['min_s'] * 1e3:.1f} .. {row['resident']['max_s'] * 1e3:.1f}) = "
                                     f"{row['resident']['clips_per_s'] / 1e3:7.1f} k clips/s | host / resident {row['host_over_resident']:.2f} | "
                                     f"max |diff| {diff:.1e}")
            finally:
                Fn.set_compute_dtype("fp32")
        # lstc_segment_mean alone: the bins of every UCF-shaped video in one launch
        rs = sets["ucf", "ev"]
        first, count = [], []
        for k, n in zip(rs.keys, ucf_counts):
            f, c = scoring.ucf_bin_table(n * SEG + 7, first_clip=rs.first_clip(k), n_clips=n)
            first += f
            count += c
        fd, cd = torch.tensor(first, dtype=torch.int64, device=dev), torch.tensor(count, dtype=torch.int32, device=dev)
        moved = (sum(count) + len(count)) * 9 * D * 4
        for l2 in (False, True):
            out = Fn.segment_mean(rs.bank, fd, cd, l2=l2)
            ts = []
            for _ in range(3 + 9):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                Fn.segment_mean(rs.bank, fd, cd, l2=l2, out=out)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e-3)
            t = statistics.median(ts[3:])
            res["rows"].append({"kernel": "lstc_segment_mean", "l2": l2, "segments": len(count), "bytes": moved, "median_us": t * 1e6,
                                "GB_per_s": moved / t / 1e9})
            lines.append(f"  lstc_segment_mean{' + l2' if l2 else '     '}: {len(count)} bins x 9 patches, {moved / 1e6:.0f} MB read + written, "
                         f"{t * 1e6:.1f} us = {moved / t / 1e9:.0f} GB/s (event-timed, median of 9; a launch this short is partly launch "
                         f"latency; gather_rows: ~6000 GB/s on an 805 MB batch)")
    finally:
        shutil.rmtree(a.work, ignore_errors=True)
    _finish(a, lines, res)


def _finish(a, lines, res):
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
