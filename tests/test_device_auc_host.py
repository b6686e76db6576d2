"""Frame-level AUC on the device, the part that needs no GPU: ``metrics.roc_auc_weighted`` (the host statement of what
``lstc_auc_weighted`` computes) against ``metrics.roc_auc`` on the expanded frames and against the O(n^2) integer formula,
``pipeline.AucWeights`` built from the ``finish`` closures of every pass over the synthetic world of tests/golden/pipeline_world.py,
the C ABI (record size, refusals by return code, workspace size), the ``--device_auc`` flag, and the host side of the launcher under
AddressSanitizer and UBSan as a stand-alone program (argument errors only: nothing is launched)."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import pipeline_world as pw                                   # noqa: E402

U52 = 2.0 ** -52


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def bar(scores):
    """(K + 4) 2^-52, K the number of distinct scores: the accumulated rounding of the host trapezoid's K float64 terms in [0, 1];
    the weighted value is rounded once."""
    return (np.unique(np.asarray(scores, dtype=np.float32)).size + 4) * U52


def rows(n, seed, wmax=48):
    """n row scores rounded to 2 decimals (heavy ties) with a +0.0 / -0.0 pair, weights 0..wmax and some rows of no weight."""
    rs = np.random.RandomState(seed)
    s = np.round(rs.rand(n), 2).astype(np.float32)
    pos, neg = rs.randint(0, wmax + 1, n), rs.randint(0, wmax + 1, n)
    if n >= 2:
        s[0], s[1] = 0.0, -0.0
        pos[0], neg[0], pos[1], neg[1] = 3, 1, 2, 5
    if n >= 8:
        pos[5::7] = 0
        neg[5::7] = 0
    return s, pos, neg


def expand(s, pos, neg):
    fs = np.repeat(s, np.asarray(pos) + np.asarray(neg))
    fl = np.concatenate([np.r_[np.ones(int(a)), np.zeros(int(b))] for a, b in zip(pos, neg)]) if len(s) else np.zeros(0)
    return fs, fl


def u2_all_pairs(s, pos, neg):
    """The contract's formula, all pairs, Python integers."""
    s = np.asarray(s, dtype=np.float32)
    keep = [i for i in range(len(s)) if pos[i] or neg[i]]
    u2 = 0
    for i in keep:
        for j in keep:
            u2 += int(pos[i]) * int(neg[j]) * (2 * int(s[i] > s[j]) + int(s[i] == s[j]))
    return u2, int(sum(int(pos[i]) for i in keep)), int(sum(int(neg[i]) for i in keep))


# ---------------------------------------------------------------------------------------------------- 1. the twin
@pytest.mark.parametrize("n", [1, 2, 257, 3000])
def test_weighted_twin_against_roc_auc_on_the_expanded_frames(n):
    from lstc_vad_amd.metrics import roc_auc, roc_auc_weighted
    cases = [rows(n, 10 + n)]
    s, pos, neg = rows(n, 20 + n)
    cases.append((np.full(n, 0.25, np.float32), pos, neg))                   # all equal: AUC 0.5 exactly
    if n == 1:
        cases.append((np.float32([0.5]), np.array([3]), np.array([4])))
    for s, pos, neg in cases:
        auc, u2, P, N = roc_auc_weighted(s, pos, neg)
        want = roc_auc(*expand(s, pos, neg))
        if P == 0 or N == 0:
            assert math.isnan(auc) and math.isnan(want)
            continue
        assert abs(auc - want) <= bar(s), (n, auc, want)
        assert auc == u2 / (2 * P * N)
    assert roc_auc_weighted(np.full(n, 0.25, np.float32), np.full(n, 2), np.full(n, 3))[0] == 0.5


@pytest.mark.parametrize("n", [1, 2, 63, 257])
def test_weighted_twin_integers_are_the_all_pairs_formula(n):
    from lstc_vad_amd.metrics import roc_auc_weighted
    s, pos, neg = rows(n, 30 + n)
    s[n // 2] = np.float32(1e-45)                                            # a denormal orders as a float
    for sc in (s, np.zeros(n, np.float32)):
        auc, u2, P, N = roc_auc_weighted(sc, pos, neg)
        assert (u2, P, N) == u2_all_pairs(sc, pos, neg)
    # rows of zero weight do not exist, NaN included
    s2, p2, n2 = s.copy(), pos.copy(), neg.copy()
    s2[-1], p2[-1], n2[-1] = np.nan, 0, 0
    want = u2_all_pairs(s2[:-1], p2[:-1], n2[:-1])
    assert roc_auc_weighted(s2, p2, n2)[1:] == want


def test_weighted_twin_nan_cases_and_refusals():
    from lstc_vad_amd.metrics import roc_auc_weighted
    s, pos, neg = rows(50, 3)
    assert math.isnan(roc_auc_weighted(s, np.zeros(50, int), neg)[0])        # P = 0
    assert math.isnan(roc_auc_weighted(s, pos, np.zeros(50, int))[0])        # N = 0
    assert math.isnan(roc_auc_weighted(np.zeros(0, np.float32), [], [])[0])
    s[7] = np.nan
    pos[7] = 1
    assert math.isnan(roc_auc_weighted(s, pos, neg)[0])                      # a weighted NaN row
    with pytest.raises(ValueError):
        roc_auc_weighted(s, pos[:-1], neg)
    with pytest.raises(ValueError):
        roc_auc_weighted(s, -pos - 1, neg)


# ---------------------------------------------------------------------------------------------------- 2. AucWeights from the closures
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from lstc_vad_amd.models import Classifier, Encoder, Regressor
    return pw.build(str(tmp_path_factory.mktemp("world")), Encoder, Regressor, Classifier)


def _keys(txt, ucf=False):
    lines = open(txt).read().splitlines()
    return [l.split(" ")[0].split("/")[-1].split(".")[0] for l in lines] if ucf else [l.split(",")[0] for l in lines]


class _Cpu(torch.nn.Module):
    """Stands in for the encoder of a pass whose scoring is faked: a parameter on the CPU names the pass's device."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def _fake_scoring(monkeypatch):
    """Scores without a device: a span's score is a function of the span alone, on a grid of 23 values (ties)."""
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd import pipeline

    def scores(enc, head, bank, spans, **kw):
        return torch.tensor([((7 * int(f) + 13 * int(t)) % 23) / 22.0 for f, t in spans], dtype=torch.float32)
    monkeypatch.setattr(pipeline.scoring, "resident_sequence_scores", scores)
    monkeypatch.setattr(Fn, "segment_mean", lambda bank, first, count, l2=False: torch.zeros(len(first), bank.shape[1], bank.shape[2]))


def _capture_launch(monkeypatch, seen):
    """``Fn.weighted_auc`` replaced by the host twin: records its operands and returns the record the kernel would write."""
    from lstc_vad_amd import _lib
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.metrics import roc_auc_weighted

    def fake(scores, pos, neg, out=None):
        auc, u2, P, N = roc_auc_weighted(scores.numpy(), pos.numpy(), neg.numpy())
        seen.append((scores.numpy().copy(), pos.numpy().copy(), neg.numpy().copy()))
        rec = _lib.AucOut(u2, P, N, auc, 0, 0)
        return torch.from_numpy(np.frombuffer(bytes(rec), dtype=np.int64).copy())
    monkeypatch.setattr(Fn, "weighted_auc", fake)


PASSES = [("SHT", "LTN", 3), ("SHT", "STN", 3), ("SHT", "LTN", 4), ("UBnormal", "LTN", 3), ("UBnormal", "STN", 3),
          ("UCF", "LTN", 2), ("UCF", "LTN", 5), ("UCF", "STN", 2)]


@pytest.mark.parametrize("dataset,mode,part_len", PASSES)
def test_auc_weights_from_the_closures_of_evaluate_auc(world, monkeypatch, dataset, mode, part_len):
    """The pass runs on the CPU with faked scores over a resident set.  First call: the weights are filled from the closures, then
    the launch refuses the CPU tensors (no fallback).  Second call, same weights, the launch replaced by the host twin and the masks
    moved away: nothing is read, and the AUC stays within the bar of the host pass (``_auc_of`` on the same scores)."""
    from lstc_vad_amd import pipeline
    ucf = dataset == "UCF"
    tag = {"SHT": "sht", "UBnormal": "ubn", "UCF": "ucf"}[dataset]
    feats, txt = world[tag + "_feats"], world[tag + "_test"]
    masks = world["ucf_gt"] if ucf else world[tag + "_masks"]
    n_patch = 9 if ucf else 16
    rs = pipeline.ResidentSet.from_archive(feats, _keys(txt, ucf), "cpu", n_patch=n_patch, view=ucf)
    _fake_scoring(monkeypatch)

    def ev(masks=masks, **kw):
        return pipeline.evaluate_auc(_Cpu(), None, mode, dataset, feats, txt, masks, part_len, n_patch, pool_sequences=7, resident=rs, **kw)
    want, fs, fl = ev(return_frames=True)
    w = pipeline.AucWeights()
    assert not w.filled
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev(device_auc=w)
    assert w.filled and w.frames == fs.size and int(w.pos_host.sum()) == int(fl.sum()) and int(w.neg_host.sum()) == int((fl == 0).sum())
    assert w.pos.dtype == torch.int32 and w.pos.shape == w.neg.shape == (w.total,)
    assert np.array_equal(w.pos.numpy(), w.pos_host) and np.array_equal(w.neg.numpy(), w.neg_host)
    seen = []
    _capture_launch(monkeypatch, seen)
    got = ev(masks=os.path.join(world["root"], "no_such_masks") + os.sep, device_auc=w)
    (scores, pos, neg), = seen
    assert isinstance(got, float) and scores.shape == (w.total,)
    assert abs(got - want) <= bar(scores), (dataset, mode, part_len, got, want)
    # the frames the host pass saw are the rows repeated
    order = np.argsort(fs, kind="mergesort")
    rep = np.repeat(scores, pos + neg)
    assert np.array_equal(np.sort(rep), fs[order])
    # weights of another pass are refused before anything is scored
    if mode == "LTN":
        with pytest.raises(ValueError, match="score rows"):
            pipeline.evaluate_auc(_Cpu(), None, mode, dataset, feats, txt, masks, part_len + 1, n_patch, resident=rs, device_auc=w)
    with pytest.raises(ValueError, match="score rows"):
        w.auc(torch.zeros(w.total + 1))
    with pytest.raises(ValueError, match="return_frames"):
        ev(device_auc=w, return_frames=True)
    with pytest.raises(TypeError):
        ev(device_auc="yes")


@pytest.mark.parametrize("mode", ["LTN", "STN"])
def test_auc_weights_from_the_closures_of_evaluate_train_auc(world, monkeypatch, mode):
    from lstc_vad_amd import pipeline
    feats, txt, masks = world["sht_feats"], world["sht_train"], world["sht_masks"]
    rs = pipeline.ResidentSet.from_archive(feats, _keys(txt), "cpu", n_patch=16)
    _fake_scoring(monkeypatch)

    def tr(masks=masks, **kw):
        return pipeline.evaluate_train_auc(_Cpu(), None, mode, "SHT", feats, txt, masks, 3, 16, pool_sequences=6, resident=rs, **kw)
    want, fs, fl = tr(return_frames=True)
    w = pipeline.AucWeights()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr(device_auc=w)
    assert w.filled and w.frames == fs.size and int(w.pos_host.sum()) == int(fl.sum())
    seen = []
    _capture_launch(monkeypatch, seen)
    got = tr(masks=os.path.join(world["root"], "no_such_masks") + os.sep, device_auc=w)
    assert abs(got - want) <= bar(seen[0][0]), (mode, got, want)
    assert abs(tr(device_auc=True) - want) <= bar(seen[0][0])                # weights built and dropped
    with pytest.raises(ValueError, match="return_frames"):
        tr(device_auc=True, return_frames=True)


def _board():
    from lstc_vad_amd import pipeline
    return pipeline._ScoreBoard(None, None, "cpu", 0, 1, None, 100)


def test_auc_weights_refusals_come_before_any_launch():
    from lstc_vad_amd import pipeline
    b = _board()
    b._register(2, lambda v: (np.repeat(v, 2), np.array([0.0, 1.0, 0.0, 1.0])), "fine")
    b._register(2, lambda v: (np.repeat(v, 2), np.array([0.0, 2.0, 0.0, 1.0])), "vid_7")
    with pytest.raises(ValueError, match="vid_7.*other than 0 / 1"):
        pipeline.AucWeights().fill(b)
    b = _board()
    b._register(3, lambda v: (np.repeat(v, 16), np.zeros(40)), "01_0042")
    with pytest.raises(ValueError, match="01_0042.*48 frame scores and 40 frame labels"):
        pipeline.AucWeights().fill(b)
    b = _board()
    b._register(1, lambda v: pytest.fail("closure run"), "x")
    b.total = (1 << 24) + 1
    with pytest.raises(ValueError, match="2\\^24"):
        pipeline.AucWeights().fill(b)
    b = _board()                                                             # 2^26 + 1 frames, as views that hold one element
    b._register(1, lambda v: (np.broadcast_to(v, ((1 << 26) + 1,)), np.broadcast_to(np.zeros(1), ((1 << 26) + 1,))), "long")
    with pytest.raises(ValueError, match="2\\^26"):
        pipeline.AucWeights().fill(b)
    # a good board: the counts are the closure's frames per row
    b = _board()
    b._register(2, lambda v: (np.repeat(v, 3), np.array([0, 1, 1, 0, 0, 0.0])), "a")
    b._register(1, lambda v: (np.repeat(v, 0), np.zeros(0)), "empty")
    b._register(1, lambda v: (np.repeat(v, 2), np.ones(2)), "c")
    w = pipeline.AucWeights().fill(b)
    assert w.total == 4 and w.frames == 8 and w.pos_host.tolist() == [2, 0, 0, 2] and w.neg_host.tolist() == [1, 3, 0, 0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.auc(torch.zeros(4))


def test_weighted_auc_refuses_before_the_device_matters():
    from lstc_vad_amd import functional as Fn
    s, c = torch.zeros(4), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(TypeError):
        Fn.weighted_auc(s.double(), c, c)
    with pytest.raises(TypeError):
        Fn.weighted_auc(s, c.long(), c)
    with pytest.raises(TypeError):
        Fn.weighted_auc(s, c[:3], c)
    with pytest.raises(TypeError):
        Fn.weighted_auc(torch.zeros(0), c[:0], c[:0])
    with pytest.raises(RuntimeError, match="not on a HIP device.*no CPU fallback"):
        Fn.weighted_auc(s, c, c)


# ---------------------------------------------------------------------------------------------------- 3. the C ABI
def test_auc_record_layout_matches_header(lib, tmp_path):
    from lstc_vad_amd._lib import AucOut
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lstc_hip.h"', 'int main(void) {',
             'printf("LstcAucOut %zu\\n", sizeof(LstcAucOut));', 'printf("version %d\\n", LSTC_VERSION);']
    for fname, _ in AucOut._fields_:
        lines.append(f'printf("LstcAucOut.{fname} %zu %zu\\n", offsetof(LstcAucOut, {fname}), sizeof(((LstcAucOut*)0)->{fname}));')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert int(got["LstcAucOut"][0]) == C.sizeof(AucOut) == 40
    assert int(got["version"][0]) == 112 == lib.lstc_version()
    for fname, ctype in AucOut._fields_:
        off, size = (int(x) for x in got[f"LstcAucOut.{fname}"])
        assert off == getattr(AucOut, fname).offset and size == C.sizeof(ctype), fname
    hdr = open(os.path.join(ROOT, "include", "lstc_hip.h")).read()
    assert "utils/eval_utils.py:21-24,139-143" in hdr


def test_auc_entry_points_refuse_by_return_code(lib):
    from lstc_vad_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("lstc_auc_weighted", "lstc_auc_workspace_bytes"):
        assert hasattr(raw, name) and name in _lib.EXPORTS
    auc, need = lib.lstc_auc_weighted, lib.lstc_auc_workspace_bytes
    # (scores, pos, neg, n, workspace, workspace_bytes, out, stream): never dereferenced, every call fails a host check
    ok = [16, 16, 16, 1000, 16, need(1000), 16, None]
    for i in (0, 1, 2, 4, 6):
        a = list(ok)
        a[i] = None
        assert auc(*a) == -1, i                                              # LSTC_E_NULL
    for n in (0, -1, -(1 << 40)):
        a = list(ok)
        a[3] = n
        assert auc(*a) == -2, n                                              # LSTC_E_SHAPE
    for short in (0, 8, need(1000) - 1, need(999) - 1):
        a = list(ok)
        a[5] = short
        assert auc(*a) == -2, short                                          # workspace too small
    for n in ((1 << 24) + 1, 1 << 40):
        a = list(ok)
        a[3], a[5] = n, 1 << 40
        assert auc(*a) == -5, n                                              # LSTC_E_RANGE
    a = list(ok)
    a[6] = 20                                                                # the record is 8-byte aligned
    assert auc(*a) == -3
    sizes = [need(n) for n in (1, 2, 255, 256, 257, 1023, 1024, 1025, 4099, 40000, 65537, 1 << 20, 1 << 24)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] < 64 << 20
    assert need(0) > 0 and need(-5) > 0 and need(1 << 30) == sizes[-1]
    assert lib.lstc_version() == 112


# ---------------------------------------------------------------------------------------------------- 4. the command line
def test_device_auc_flag_parses_on_every_script():
    from lstc_vad_amd import cli
    scripts = list(cli._FLAGS)
    assert any(s.startswith("evaluation") for s in scripts) and set(cli.SCRIPTS) <= set(scripts)
    for script in scripts:
        p = cli.build_parser(script)
        assert p.parse_args([]).device_auc is False, script
        assert p.parse_args(["--device_auc"]).device_auc is True, script
        assert p.parse_args(["--device_auc", "--resident_eval"]).resident_eval is True, script
        assert cli.complete_args(script, Namespace(batch_size=2)).device_auc is False, script
        assert cli.complete_args(script, Namespace(device_auc=True)).device_auc is True, script
        argv = cli.namespace_to_argv(script, p.parse_args(["--device_auc"]))
        assert "--device_auc" in argv and cli.complete_args(script, argv=argv).device_auc is True, script
        assert "--device_auc" not in cli.namespace_to_argv(script, p.parse_args([])), script


# ---------------------------------------------------------------------------------------------------- 5. the launcher under sanitizers
SAN_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include <stdint.h>
#include "lstc_hip.h"
/* what the launcher's translation unit expects from the rest of the library in a host-only build */
extern "C" const char FATBIN_SYMBOL[1024] = {0};
const uint64_t* lstc_seed_dev_current() { return nullptr; }
int main(void) {
    int bad = 0;
    static float s[16];                            /* never dereferenced: every call below fails a host check */
    static uint32_t w[16];
    static uint64_t ws[4];
    LstcAucOut out; memset(&out, 0, sizeof out);
    const int64_t need = lstc_auc_workspace_bytes(1000);
    bad += sizeof(LstcAucOut) != 40;
    bad += lstc_auc_weighted(NULL, w, w, 1000, ws, need, &out, NULL) != LSTC_E_NULL;
    bad += lstc_auc_weighted(s, NULL, w, 1000, ws, need, &out, NULL) != LSTC_E_NULL;
    bad += lstc_auc_weighted(s, w, NULL, 1000, ws, need, &out, NULL) != LSTC_E_NULL;
    bad += lstc_auc_weighted(s, w, w, 1000, NULL, need, &out, NULL) != LSTC_E_NULL;
    bad += lstc_auc_weighted(s, w, w, 1000, ws, need, NULL, NULL) != LSTC_E_NULL;
    bad += lstc_auc_weighted(s, w, w, 0, ws, need, &out, NULL) != LSTC_E_SHAPE;
    bad += lstc_auc_weighted(s, w, w, INT64_MIN, ws, need, &out, NULL) != LSTC_E_SHAPE;
    bad += lstc_auc_weighted(s, w, w, 1000, ws, need - 1, &out, NULL) != LSTC_E_SHAPE;
    bad += lstc_auc_weighted(s, w, w, 1000, ws, INT64_MIN, &out, NULL) != LSTC_E_SHAPE;
    bad += lstc_auc_weighted(s, w, w, ((int64_t)1 << 24) + 1, ws, INT64_MAX, &out, NULL) != LSTC_E_RANGE;
    bad += lstc_auc_weighted(s, w, w, INT64_MAX, ws, INT64_MAX, &out, NULL) != LSTC_E_RANGE;
    bad += lstc_auc_weighted(s, w, w, 1000, ws, need, (LstcAucOut*)((char*)&out + 4), NULL) != LSTC_E_ALIGN;
    int64_t last = 0;
    const int64_t ns[] = {INT64_MIN, -1, 0, 1, 256, 257, 1024, 1025, 40000, (int64_t)1 << 24, ((int64_t)1 << 24) + 1, INT64_MAX};
    for (unsigned k = 0; k < sizeof ns / sizeof ns[0]; ++k) {
        const int64_t b = lstc_auc_workspace_bytes(ns[k]);
        bad += !(b > 0 && b >= last);
        last = b;
    }
    printf("workspace(1000) %lld bad %d\n", (long long)need, bad);
    return bad;
}
"""


def test_auc_launcher_host_side_is_clean_under_asan_and_ubsan(tmp_path):
    """The host half of csrc/metrics.hip (the launch plan and the argument checks) compiled host-only with
    -fsanitize=address,undefined and linked with a small ``main`` that calls the entry points with bad arguments.  A stand-alone
    program: no GPU, nothing launched, nothing loaded into python."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc absent")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libsan"]
    obj = tmp_path / "metrics_host.o"
    subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-ffp-contract=off",
                    *[a for f in san for a in ("-Xarch_host", f)], "-I", os.path.join(ROOT, "include"), "-c",
                    os.path.join(ROOT, "lstc_vad_amd", "csrc", "metrics.hip"), "-o", str(obj)], check=True, timeout=600)
    syms = subprocess.run(["nm", str(obj)], capture_output=True, text=True, check=True).stdout
    fatbin = re.search(r"\bU (__hip_fatbin_\w+)", syms).group(1)
    src = tmp_path / "main.cpp"
    src.write_text(SAN_MAIN.replace("FATBIN_SYMBOL", fatbin))
    exe = tmp_path / "auc_args"
    main_obj = tmp_path / "main.o"
    subprocess.run([hipcc, *san, "-x", "c++", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(main_obj)], check=True,
                   timeout=600)
    subprocess.run([hipcc, *san, str(main_obj), str(obj), "-o", str(exe)], check=True, timeout=600)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)      # the environment is left as it is
    assert r.returncode == 0 and "bad 0" in r.stderr + r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout, r.stderr[-3000:])
