"""Frame-level AUC on the GPU: ``lstc_auc_weighted`` against its host twin ``metrics.roc_auc_weighted`` (integers equal, the AUC
bit-equal), the bits' independence of the launch, and the two AUC passes with ``device_auc=`` against the same pass without it on
the synthetic world of tests/golden/pipeline_world.py (through the helpers of tests/test_resident_gpu.py)."""
import math
import os
import re
import struct

import numpy as np
import pytest
import torch

from test_resident_gpu import DEV, _cli, _keys, _models, _no_uploads, _owns, _two, world        # noqa: F401  (world: a fixture)

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
# the kernel's own sizes (csrc/metrics.hip): 256 rows i per workgroup, chunks of 1024 rows j through LDS, slices of whole chunks -
# one chunk per slice up to 64 * 1024 rows, two from 65 537 rows on
NT, CHUNK, ONE_CHUNK_SLICES = 256, 1024, 64 * 1024
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 4099]
SLICE_SIZES = [ONE_CHUNK_SLICES - 1, ONE_CHUNK_SLICES, ONE_CHUNK_SLICES + 1]


def _Fn():
    from lstc_vad_amd import functional as Fn
    return Fn


def bar(scores):
    """(K + 4) 2^-52, K distinct scores: the rounding of the host trapezoid's K float64 terms; the device value is rounded once."""
    return (np.unique(np.asarray(scores, dtype=np.float32)).size + 4) * U52


def rows(n, seed, wmax=48):
    """Scores rounded to 2 decimals, a +0.0 / -0.0 pair, a denormal, weights 0..wmax, rows of zero weight that carry NaN."""
    rs = np.random.RandomState(seed)
    s = np.round(rs.rand(n), 2).astype(np.float32)
    pos, neg = rs.randint(0, wmax + 1, n).astype(np.int32), rs.randint(0, wmax + 1, n).astype(np.int32)
    if n >= 2:
        s[0], s[1] = 0.0, -0.0
        pos[0], neg[0], pos[1], neg[1] = 3, 1, 2, 5
    if n >= 8:
        s[3] = np.float32(1e-45)
        pos[3], neg[3] = 1, 1
        s[5::7] = np.nan
        pos[5::7] = 0
        neg[5::7] = 0
    return s, pos, neg


def device_auc(s, pos, neg, dtype=torch.int32):
    Fn = _Fn()
    rec = Fn.weighted_auc(torch.from_numpy(s).to(DEV), torch.from_numpy(pos).to(DEV).view(dtype), torch.from_numpy(neg).to(DEV).view(dtype))
    assert rec.is_cuda and rec.dtype == torch.int64 and rec.numel() == 5
    return Fn.read_auc(rec)


def same_bits(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def check_against_twin(s, pos, neg, what, dtype=torch.int32):
    from lstc_vad_amd.metrics import roc_auc_weighted
    auc, u2, P, N = roc_auc_weighted(s, pos, neg)
    got = device_auc(s, pos, neg, dtype)
    assert (got.u2, got.pos, got.neg, got.flags, got.reserved) == (u2, P, N, 0, 0), (what, got.u2, u2, got.pos, P, got.neg, N, got.flags)
    if P == 0 or N == 0:
        assert math.isnan(got.auc) and math.isnan(auc), what
    else:
        assert same_bits(got.auc, u2 / (2 * P * N)) and same_bits(got.auc, auc), (what, got.auc, auc)
    return got


@pytest.mark.parametrize("n", SIZES)
def test_kernel_is_the_twin_exactly(n):
    s, pos, neg = rows(n, 100 + n, 4000 if n == 4099 else 48)
    got = check_against_twin(s, pos, neg, (n, "rounded"))
    if n == 4099:
        assert got.u2 > 1 << 32 and got.pos + got.neg < 1 << 26          # the count leaves 32 bits, the frames stay under the limit
    check_against_twin(np.full(n, 0.25, np.float32), pos, neg, (n, "all equal"))
    check_against_twin(s, np.zeros_like(pos), neg, (n, "pos all zero"))
    check_against_twin(s, pos, np.zeros_like(neg), (n, "neg all zero"))
    if hasattr(torch, "uint32"):
        check_against_twin(s, pos, neg, (n, "uint32"), torch.uint32)
    # one positive row in the last workgroup only: every other block of rows leaves at once
    p1 = np.zeros_like(pos)
    p1[n - 1] = 7
    s1 = s.copy()
    s1[n - 1] = 0.5
    n1 = neg.copy()
    n1[0] += 1                                                          # N > 0 without giving a NaN row weight
    check_against_twin(s1, p1, n1, (n, "one positive row"))


@pytest.mark.parametrize("n", SLICE_SIZES)
def test_kernel_is_the_twin_where_the_slices_grow(n):
    s, pos, neg = rows(n, 7, 48)
    check_against_twin(s, pos, neg, (n, "rounded"))


def test_flags():
    L = __import__("lstc_vad_amd._lib", fromlist=["_lib"])
    s, pos, neg = rows(4099, 5)
    s[2000] = np.nan
    pos[2000], neg[2000] = 0, 3                                           # a weighted row with a NaN score
    got = device_auc(s, pos, neg)
    assert got.flags == L.AUC_NAN_SCORE and math.isnan(got.auc)
    assert (got.pos, got.neg) == (int(pos.astype(np.int64).sum()), int(neg.astype(np.int64).sum()))
    s, pos, neg = rows(4099, 6)
    s[np.isnan(s)] = 0.5                                                  # every row gets weight below
    pos[:], neg[:] = 1 << 14, 1 << 14                                     # 4099 * 2^15 frames > 2^26
    got = device_auc(s, pos, neg)
    assert got.flags == L.AUC_TOO_MANY_FRAMES and math.isnan(got.auc)
    assert (got.pos, got.neg) == (4099 << 14, 4099 << 14)
    pos[:], neg[:] = 1 << 13, 1 << 13                                     # 4099 * 2^14 frames sit just above 2^26 as well
    assert device_auc(s, pos, neg).flags == L.AUC_TOO_MANY_FRAMES
    pos[:], neg[:] = 8186, 8186                                           # 4099 * 16372 = 67 108 828 <= 2^26: not flagged, and exact
    check_against_twin(s, pos, neg, "at the limit")


def test_one_realistic_size():
    """n = 40 000 (an STN pass over ShanghaiTech has 37 k rows): real-shaped weights - most rows cover 16 label-0 frames."""
    rs = np.random.RandomState(11)
    n = 40000
    s = rs.rand(n).astype(np.float32)
    s[::50] = np.round(s[::50], 1)
    neg = np.full(n, 16, np.int32)
    pos = np.zeros(n, np.int32)
    hot = rs.rand(n) < 0.04
    pos[hot] = rs.randint(1, 17, int(hot.sum()))
    neg[hot] = 16 - pos[hot]
    check_against_twin(s, pos, neg, "40 000")


def test_bits_do_not_depend_on_the_launch():
    """The same input twice through the cached workspace, and once more through a workspace 4 bytes off a 16-byte boundary."""
    from lstc_vad_amd import _lib as L
    Fn = _Fn()
    n = 4099
    s, pos, neg = rows(n, 9, 4000)
    ds, dp, dn = (torch.from_numpy(a).to(DEV) for a in (s, pos, neg))
    a = Fn.weighted_auc(ds, dp, dn).clone()
    b = Fn.weighted_auc(ds, dp, dn, out=torch.empty(5, dtype=torch.int64, device=DEV))
    lib = L.load()
    need = int(lib.lstc_auc_workspace_bytes(n))
    store = torch.full((need + 32,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = store[4:4 + need]
    assert ws.data_ptr() % 16 == 4
    c = torch.empty(5, dtype=torch.int64, device=DEV)
    L.check(lib.lstc_auc_weighted(L.dev_ptr(ds), L.dev_ptr(dp), L.dev_ptr(dn), n, L.dev_ptr(ws), need, L.dev_ptr(c), L.stream_ptr()),
            "lstc_auc_weighted")
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert bool((store[:4] == 0xAB).all()) and bool((store[4 + need:] == 0xAB).all())          # nothing outside the workspace is written
    assert Fn.read_auc(a).flags == 0 and Fn.read_auc(a).u2 > 1 << 32


# ---------------------------------------------------------------------------------------------------- the passes
def _passes(world, dialect):
    """(name, mode, models, kwargs of evaluate_auc, resident factory) of a dialect's test list."""
    from lstc_vad_amd import pipeline
    if dialect == "UCF":
        feats, txt, masks, keys = world["ucf_feats"], world["ucf_test"], world["ucf_gt"], _keys(world["ucf_test"], True)
        make = lambda r, w: pipeline.ResidentSet.from_archive(feats, keys, DEV, n_patch=9, view=True, owns=_owns(r, w))
        return [("LTN", "ucf", (feats, txt, masks, 2, 9), dict(pool_sequences=20), make)]
    tag = "sht" if dialect == "SHT" else "ubn"
    feats, txt, masks, keys = world[tag + "_feats"], world[tag + "_test"], world[tag + "_masks"], _keys(world[tag + "_test"])
    make = lambda r, w: pipeline.ResidentSet.from_archive(feats, keys, DEV, n_patch=16, owns=_owns(r, w))
    return [("LTN", "ltn", (feats, txt, masks, 3, 16), dict(pool_sequences=5), make),
            ("STN", "stn", (feats, txt, masks, 3, 16), dict(pool_sequences=5), make)]


@pytest.mark.parametrize("dialect", ["SHT", "UBnormal", "UCF"])
def test_evaluate_auc_on_the_device_is_the_host_auc(world, dialect, monkeypatch):
    from lstc_vad_amd import pipeline
    for mode, which, (feats, txt, masks, part_len, n_patch), kw, make in _passes(world, dialect):
        enc, head = _models(world, which)

        def ev(rs=None, masks=masks, **more):
            return pipeline.evaluate_auc(enc, head, mode, dialect, feats, txt, masks, part_len, n_patch, resident=rs, **kw, **more)
        whole = make(None, None)
        for route, rs_of in (("host-fed", lambda r, w: None), ("resident", lambda r, w: whole if w is None else make(r, w))):
            want, fs, _ = ev(rs_of(None, None), return_frames=True)
            tol = bar(fs)
            w = pipeline.AucWeights()
            got = [ev(rs_of(None, None), device_auc=True), ev(rs_of(None, None), device_auc=w), ev(rs_of(None, None), device_auc=w)]
            got.append(_two(lambda r, n, ex: ev(rs_of(r, n), rank=r, world=n, exchange=ex, device_auc=w)))
            print(dialect, mode, route, "AUC %.17g, device - host %s, bar %.2e" % (want, [g - want for g in got], tol))
            assert all(isinstance(g, float) for g in got) and got[0] == got[1] == got[2] == got[3]
            assert abs(got[0] - want) <= tol, (dialect, mode, route, got[0], want)
            assert w.filled and w.frames == fs.size
            if route == "resident":
                # filled weights over a resident set: no mask file or ground-truth archive is opened, nothing is uploaded
                with monkeypatch.context() as m:
                    _no_uploads(m)
                    again = ev(whole, masks=os.path.join(world["root"], "no_such_masks") + os.sep, device_auc=w)
                assert again == got[0]
        with pytest.raises(ValueError, match="return_frames"):
            ev(device_auc=True, return_frames=True)


@pytest.mark.parametrize("mode,which", [("LTN", "ltn"), ("STN", "stn")])
def test_evaluate_train_auc_on_the_device_is_the_host_auc(world, mode, which, monkeypatch):
    from lstc_vad_amd import pipeline
    enc, head = _models(world, which)
    feats, txt, masks = world["sht_feats"], world["sht_train"], world["sht_masks"]
    make = lambda r, w: pipeline.ResidentSet.from_archive(feats, _keys(txt), DEV, n_patch=16, owns=_owns(r, w))
    whole = make(None, None)

    def tr(rs=None, masks=masks, **more):
        return pipeline.evaluate_train_auc(enc, head, mode, "SHT", feats, txt, masks, 3, 16, pool_sequences=6, resident=rs, **more)
    for route, rs_of in (("host-fed", lambda r, w: None), ("resident", lambda r, w: whole if w is None else make(r, w))):
        want, fs, _ = tr(rs_of(None, None), return_frames=True)
        w = pipeline.AucWeights()
        got = [tr(rs_of(None, None), device_auc=True), tr(rs_of(None, None), device_auc=w), tr(rs_of(None, None), device_auc=w)]
        got.append(_two(lambda r, n, ex: tr(rs_of(r, n), rank=r, world=n, exchange=ex, device_auc=w)))
        print("train", mode, route, "AUC %.17g, device - host %s, bar %.2e" % (want, [g - want for g in got], bar(fs)))
        assert got[0] == got[1] == got[2] == got[3] and abs(got[0] - want) <= bar(fs), (mode, route, got, want)
        if route == "resident":
            with monkeypatch.context() as m:
                _no_uploads(m)
                assert tr(whole, masks=os.path.join(world["root"], "no_such_masks") + os.sep, device_auc=w) == got[0]
    with pytest.raises(ValueError, match="score rows"):
        tr(whole, device_auc=_other_total(w))


def _other_total(w):
    from lstc_vad_amd import pipeline
    o = pipeline.AucWeights()
    o.pos, o.neg, o.pos_host, o.neg_host, o.total, o.frames = w.pos[:-1], w.neg[:-1], w.pos_host[:-1], w.neg_host[:-1], w.total - 1, w.frames
    return o


# ---------------------------------------------------------------------------------------------------- the command line
def test_device_auc_flag_on_the_command_line(world, tmp_path):
    """Train/temporal_transformer_shanghaitech.py with --resident_eval --device_auc against --resident_eval alone: the AUC values
    of the log agree within the bar (K <= 130, the clips of the longer list: a pass has at most one score row per clip) and the
    same checkpoints are written (their names end in str(AUC))."""
    model = ["--d_model", "32", "--n_head", "2", "--d_k", "16", "--d_v", "16", "--n_hidden", "64", "--MHA_layerNorm", "--FFN_layerNorm",
             "--relative_position_encoding", "--part_len", "3"]
    train = model + ["--dataset_path", world["sht_feats"], "--training_txt", world["sht_train"], "--testing_txt", world["sht_test"],
                     "--test_mask_dir", world["sht_masks"], "--batch_size", "2", "--part_num", "3", "--n_patch", "16", "--load_model",
                     "--lr_encoder", "0", "--lr_classifier", "0", "--epochs", "1", "--inter_epoch", "1", "--seed", "3",
                     "--save_threshold", "0", "--load_temporal_model_path", world["ltn_sht_enc.ckpt"], "--load_classifier_model_path",
                     world["ltn_sht_cls.ckpt"], "--saved_prefix", "pre_"]
    tol = (130 + 4) * U52
    number = re.compile(r"[-+]?\d+\.\d+(?:[eE][-+]?\d+)?|nan")
    got = {}
    for tag, flag in (("host", ["--resident_eval"]), ("device", ["--resident_eval", "--device_auc"])):
        save = str(tmp_path / f"ck_{tag}") + os.sep
        os.makedirs(save)
        r = _cli("Train", "temporal_transformer_shanghaitech.py", train + flag + ["--model_save_dir", save, "--log_dir", str(tmp_path / f"log_{tag}")])
        assert r.returncode == 0, r.stderr[-2500:]
        lines = [l.split(": ", 1)[-1] for l in r.stderr.splitlines() if "_AUC" in l]
        got[tag] = (lines, sorted(os.listdir(save)))
    (a_lines, a_ck), (b_lines, b_ck) = got["host"], got["device"]
    assert a_lines and any("train_AUC" in l for l in a_lines) and len(a_lines) == len(b_lines)
    for la, lb in zip(a_lines, b_lines):
        assert number.sub("#", la) == number.sub("#", lb), (la, lb)             # the same text around the numbers
        va, vb = [float(x) for x in number.findall(la)], [float(x) for x in number.findall(lb)]
        assert va and len(va) == len(vb) and all(abs(x - y) <= tol for x, y in zip(va, vb)), (la, lb)
    assert a_ck and len(a_ck) == len(b_ck)
    for fa, fb in zip(a_ck, b_ck):
        (ha, xa), (hb, xb) = fa.rsplit("_", 1), fb.rsplit("_", 1)
        assert ha == hb and abs(float(xa) - float(xb)) <= tol, (fa, fb)


def test_device_auc_flag_on_the_evaluation_script(world):
    """Test/evaluation_shanghaitech_ubnormal.py with --device_auc, with and without --resident_eval, against the script without it:
    the printed AUC agrees within the bar (K <= 42, the clips of the test list)."""
    ev = ["--d_model", "32", "--temporal_n_head", "2", "--temporal_d_k", "16", "--temporal_d_v", "16", "--temporal_n_hidden", "64",
          "--temporal_MHA_layerNorm", "--temporal_FFN_layerNorm", "--temporal_relative_position_encoding", "--part_len", "3", "--dataset", "SHT",
          "--dataset_path", world["sht_feats"], "--testing_txt", world["sht_test"], "--test_mask_dir", world["sht_masks"],
          "--temporal_model_path", world["ltn_sht_enc.ckpt"], "--classifier_model_path", world["ltn_sht_cls.ckpt"]]
    got = []
    for flag in ([], ["--device_auc"], ["--resident_eval", "--device_auc"]):
        e = _cli("Test", "evaluation_shanghaitech_ubnormal.py", ev + flag)
        assert e.returncode == 0, e.stderr[-2000:]
        got.append(float(e.stdout.strip().split("auc = ")[-1]))
    assert 0.0 <= got[0] <= 1.0 and all(abs(g - got[0]) <= (42 + 4) * U52 for g in got[1:]), got
