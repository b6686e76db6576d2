"""Resident scoring on the GPU: lstc_cls_concat_span_fwd against lstc_cls_concat_var_fwd on the materialised tokens (bit for bit),
lstc_segment_mean against float64, Encoder.forward_cls_spans against forward_cls_unpadded in every compute mode and in training,
and the pipeline passes with ``resident=`` against the host-fed passes on the synthetic world of tests/golden/pipeline_world.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import util_ragged as R

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import pipeline_world as pw                                   # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F64 = torch.float64
U24 = 2.0 ** -24
NAN = float("nan")


def _Fn():
    from lstc_vad_amd import functional as Fn
    return Fn


def _L():
    from lstc_vad_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------- 5. the span concat
# (first row, tokens): lengths 1, 2, 16, 127; the 16-token span overlaps the first 127-token one, which is repeated; src0 is neither
# sorted nor increasing
SPANS = [(200, 127), (190, 16), (100, 2), (50, 1), (200, 127), (20, 16), (51, 2)]
BANK_ROWS = 400


def _span_bank(d, shift):
    """A bank [BANK_ROWS, d] that is NaN outside the spans; ``shift``: its base lies 4 bytes behind a 16-byte boundary."""
    g = torch.Generator().manual_seed(100 + d)
    store = torch.full((BANK_ROWS * d + 4,), NAN)
    bank = store[1:1 + BANK_ROWS * d].view(BANK_ROWS, d) if shift else store[:BANK_ROWS * d].view(BANK_ROWS, d)
    for s, L in SPANS:
        bank[s:s + L] = torch.randn(L, d, generator=g)
    store = store.to(DEV)
    bank = store[1:1 + BANK_ROWS * d].view(BANK_ROWS, d) if shift else store[:BANK_ROWS * d].view(BANK_ROWS, d)
    assert bank.data_ptr() % 16 == (4 if shift else 0) and bank.is_contiguous()
    return bank


def _guarded(M, d):
    """y [M, d] inside a buffer with one NaN guard row before and one after -> (buffer, y)."""
    buf = torch.full((M + 2, d), NAN, device=DEV)
    return buf, buf[1:M + 1]


@pytest.mark.parametrize("with_tok", [False, True])
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("d", [30, 32, 40, 2048])
def test_span_concat_is_bitwise_the_var_concat_of_the_materialised_tokens(d, shift, with_tok):
    """d = 32, 40: the 16-B path; d = 30 (not a multiple of 4) and every bank whose base is shifted by 4 bytes: the 4-B path;
    d = 2048: 2 column groups on the 16-B path, 8 on the 4-B one.  With the learned token and the position table set and null; N = 1
    alone and all spans in one call."""
    L = _L()
    lib = L.load()
    bank = _span_bank(d, shift)
    g = torch.Generator().manual_seed(7)
    cls = torch.randn(d, generator=g).to(DEV) if with_tok else None
    pos = torch.randn(128, d, generator=g).to(DEV) if with_tok else None
    alone = {}
    for spans in (SPANS[:1], SPANS[3:4], SPANS):
        N = len(spans)
        lens = [t for _, t in spans]
        row0 = torch.tensor(np.concatenate([[0], np.cumsum([t + 1 for t in lens])]), dtype=torch.int32).to(DEV)
        src0 = torch.tensor([s for s, _ in spans], dtype=torch.int64).to(DEV)
        M = sum(lens) + N
        x = torch.cat([bank[s:s + t] for s, t in spans], 0).contiguous()           # the reference input: the materialised tokens
        assert torch.isfinite(x).all()
        ref_buf, ref = _guarded(M, d)
        L.check(lib.lstc_cls_concat_var_fwd(L.dev_ptr(x), L.dev_ptr(row0), L.dev_ptr(cls), L.dev_ptr(pos), L.dev_ptr(ref), N, d,
                                            L.stream_ptr()), "lstc_cls_concat_var_fwd")
        buf, y = _guarded(M, d)
        L.check(lib.lstc_cls_concat_span_fwd(L.dev_ptr(bank), BANK_ROWS, L.dev_ptr(src0), L.dev_ptr(row0), L.dev_ptr(cls),
                                             L.dev_ptr(pos), L.dev_ptr(y), N, d, L.stream_ptr()), "lstc_cls_concat_span_fwd")
        torch.cuda.synchronize()
        assert torch.isfinite(y).all()
        assert torch.equal(y, ref), (d, shift, with_tok, N)
        assert torch.isnan(buf[0]).all() and torch.isnan(buf[M + 1]).all()          # the guard rows are untouched
        if N == 1:
            alone[spans[0]] = y.clone()
    for n, sp in enumerate(SPANS):               # a sequence's bits depend neither on its neighbours nor on its place in the call
        if sp in alone:
            assert torch.equal(y[int(row0[n]):int(row0[n + 1])], alone[sp]), sp
    if not shift and d % 4 == 0:
        # the two access paths give the same bits: the same spans out of an aligned and out of a shifted bank
        other = _span_bank(d, True)
        _, y2 = _guarded(M, d)
        L.check(lib.lstc_cls_concat_span_fwd(L.dev_ptr(other), BANK_ROWS, L.dev_ptr(src0), L.dev_ptr(row0), L.dev_ptr(cls),
                                             L.dev_ptr(pos), L.dev_ptr(y2), N, d, L.stream_ptr()), "lstc_cls_concat_span_fwd")
        torch.cuda.synchronize()
        assert torch.equal(y2, y)


# ---------------------------------------------------------------------------------------------------- 6.-8. the segment mean
SEG_CLIPS = 200
COUNTS = [1, 2, 7, 190]


@functools.lru_cache(maxsize=None)
def _seg_bank(P, d):
    g = torch.Generator().manual_seed(1000 * P + d)
    return torch.randn(SEG_CLIPS, P, d, generator=g).to(DEV)


def _table(n_seg, seed):
    """n_seg segments whose counts cycle through COUNTS, first clips anywhere they fit (they overlap)."""
    rs = np.random.RandomState(seed)
    count = [COUNTS[(s + seed) % 4] for s in range(n_seg)]
    first = [int(rs.randint(0, SEG_CLIPS - c + 1)) for c in count]
    return first, count


def _mean64(bank, first, count):
    """(float64 mean, mean over the clips of |x|) of every segment."""
    ref = torch.stack([bank[f:f + c].to(F64).mean(0) for f, c in zip(first, count)])
    mag = torch.stack([bank[f:f + c].to(F64).abs().mean(0) for f, c in zip(first, count)])
    return ref, mag


@pytest.mark.parametrize("n_seg", [1, 64])
@pytest.mark.parametrize("d", [30, 40, 1024, 2048])
@pytest.mark.parametrize("P", [1, 9])
def test_segment_mean_against_float64(P, d, n_seg):
    """|out - ref| <= 2 count 2^-24 mean_c|x| elementwise: the first-order bound of a sequential f32 sum of ``count`` terms plus one
    division, times 2 for the higher-order terms.  A count of 1 is a bit-exact copy.  d = 30: the 4-B path."""
    Fn = _Fn()
    bank = _seg_bank(P, d)
    tables = [_table(64, 3)] if n_seg == 64 else [([11 + 3 * i], [c]) for i, c in enumerate(COUNTS)]
    worst = 0.0
    for first, count in tables:
        out = Fn.segment_mean(bank, first, count)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (len(first), P, d)
        ref, mag = _mean64(bank, first, count)
        for s, (f, c) in enumerate(zip(first, count)):
            if c == 1:
                assert torch.equal(out[s], bank[f]), (P, d, s)
                continue
            err, bound = (out[s].to(F64) - ref[s]).abs(), 2 * c * U24 * mag[s]
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), (P, d, s, c, float((err / bound).max()))
    print(f"segment_mean P={P} d={d} n_seg={n_seg}: worst err / bound {worst:.3f}")
    # a count below 1 is clamped to 1
    assert torch.equal(Fn.segment_mean(bank, [5, 6], [0, -3]), bank[5:7])


@pytest.mark.parametrize("d", [30, 40, 1024, 2048])
@pytest.mark.parametrize("P", [1, 9])
def test_segment_mean_normalisation(P, d):
    """Count-1 segments, so the mean is exact: |out - ref64| <= (d / 2 + 3) 2^-24 |ref64| bounds any summation order of d squares, a
    square root and a division.  An all-zero row gives zeros."""
    Fn = _Fn()
    bank = _seg_bank(P, d).clone()
    bank[17, 0] = 0.0
    bank[18] = bank[18] * 1e-3                              # a small row and a large one: the norm is not near 1
    bank[19] = bank[19] * 1e3
    first = [17, 18, 19, 3, 199, 0]
    out = Fn.segment_mean(bank, first, [1] * len(first), l2=True)
    torch.cuda.synchronize()
    x = bank[first].to(F64)
    ref = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    err, bound = (out.to(F64) - ref).abs(), (d / 2 + 3) * U24 * ref.abs()
    assert torch.isfinite(out).all()
    assert bool((out[0, 0] == 0).all())
    assert bool((err <= bound).all()), (P, d, float((err / bound.clamp_min(1e-300)).max()))
    print(f"segment_mean l2 P={P} d={d}: worst err / bound {float((err / bound.clamp_min(1e-300))[bound > 0].max()):.3f}")
    # and on real means: against F.normalize of the unnormalised result, at the same bound plus the rounding of the mean itself
    f2, c2 = _table(8, 5)
    plain, normed = Fn.segment_mean(bank, f2, c2), Fn.segment_mean(bank, f2, c2, l2=True)
    want = plain.to(F64) / plain.to(F64).norm(dim=-1, keepdim=True).clamp_min(1e-12)
    assert bool(((normed.to(F64) - want).abs() <= (d / 2 + 3) * U24 * want.abs()).all())


@pytest.mark.parametrize("l2", [False, True])
def test_segment_mean_bits_do_not_depend_on_the_launch(l2):
    Fn = _Fn()
    for P, d in ((9, 2048), (1, 40), (9, 30)):
        bank = _seg_bank(P, d)
        first, count = _table(64, 9)
        pool = Fn.segment_mean(bank, first, count, l2=l2)
        for s in (0, 1, 2, 3, 37, 63):
            alone = Fn.segment_mean(bank, first[s:s + 1], count[s:s + 1], l2=l2)
            assert torch.equal(alone[0], pool[s]), (P, d, s, count[s])
        # device tables are taken as they are
        again = Fn.segment_mean(bank, torch.tensor(first, dtype=torch.int64, device=DEV), torch.tensor(count, dtype=torch.int32, device=DEV), l2=l2)
        assert torch.equal(again, pool)


# ---------------------------------------------------------------------------------------------------- 9.-10. the encoder
ENC_SPANS = [(150, 63), (10, 1), (140, 127), (300, 15), (150, 63), (0, 32), (5, 2), (320, 96)]
_built = {}


def _encoder(**extra):
    key = tuple(sorted(extra.items()))
    if key not in _built:
        from lstc_vad_amd.models import Encoder
        torch.manual_seed(29)
        enc = Encoder(**R.encoder_kw(8, 0.0, **extra))              # window_depth 8: the relative index covers 127 patch tokens
        with torch.no_grad():
            for layer in enc.layer_stack:
                layer.slf_attn.relative_position_bias_table.normal_(0.0, 0.4)
        _built[key] = enc.to(DEV)
    return _built[key]


@functools.lru_cache(maxsize=None)
def _enc_bank():
    """[420, 32] rows, NaN outside the spans."""
    g = torch.Generator().manual_seed(31)
    bank = torch.full((420, 32), NAN)
    for s, t in ENC_SPANS:
        bank[s:s + t] = torch.randn(t, 32, generator=g)
    return bank.to(DEV)


class _LibSpy:
    """Records every C entry point the Python layer calls (``_lib.load()`` hands out this proxy)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("lstc_") or name in ("lstc_strerror", "lstc_pack1_bytes", "lstc_version"):
            return fn

        def wrapped(*a):
            self.calls.append(name)
            return fn(*a)
        return wrapped


@pytest.mark.parametrize("mode", ["fp32", "f32x3", "bf16"])
def test_forward_cls_spans_is_bitwise_forward_cls_unpadded(mode, monkeypatch):
    Fn, L = _Fn(), _L()
    enc = _encoder().eval()
    bank = _enc_bank()
    starts, lens = [s for s, _ in ENC_SPANS], [t for _, t in ENC_SPANS]
    tokens = torch.cat([bank[s:s + t] for s, t in ENC_SPANS], 0)
    Fn.set_compute_dtype(mode)
    Fn.set_x3_threshold(0, 0, 0)
    try:
        with torch.no_grad():
            ref = enc.forward_cls_unpadded(tokens, lens)
            spy = _LibSpy(L.load())
            monkeypatch.setattr(L, "load", lambda: spy)
            got = enc.forward_cls_spans(bank, starts, lens)
            monkeypatch.undo()
            got3 = enc.forward_cls_spans(bank.view(105, 4, 32), torch.tensor(starts), torch.tensor(lens))     # [clips, P, d], CPU tensors
        torch.cuda.synchronize()
    finally:
        monkeypatch.undo()
        Fn.set_compute_dtype("fp32")
        Fn.set_x3_threshold()
    assert tuple(got.shape) == (len(lens), 32) and torch.isfinite(got).all()
    assert torch.equal(got, ref) and torch.equal(got3, ref), (mode, float((got - ref).abs().max()))
    assert spy.calls.count("lstc_cls_concat_span_fwd") == 1 and "lstc_cls_concat_var_fwd" not in spy.calls
    assert spy.calls.count("lstc_attn_var_fwd") == 2 and "lstc_attn_fwd" not in spy.calls      # the unpadded chain behind the embed


def test_forward_cls_spans_training_gradients_are_those_of_the_unpadded_route():
    """Dropout 0, a learned CLS token and the position table: every parameter's gradient equals the unpadded route's bit for bit (the
    token-row sums come from lstc_cls_concat_var_bwd with dx = NULL in both); the bank gets none."""
    enc = _encoder(CLS_learned=True, position_encoding=True, max_position_tokens=128).train()
    bank = _enc_bank()
    starts, lens = [s for s, _ in ENC_SPANS], [t for _, t in ENC_SPANS]
    tokens = torch.cat([bank[s:s + t] for s, t in ENC_SPANS], 0)
    W = torch.randn(len(lens), 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    grads = []
    for route in ("unpadded", "spans"):
        enc.zero_grad(set_to_none=True)
        out = enc.forward_cls_unpadded(tokens, lens) if route == "unpadded" else enc.forward_cls_spans(bank, starts, lens)
        (out * W).sum().backward()
        torch.cuda.synchronize()
        grads.append(({k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None}, out.detach().clone()))
    enc.zero_grad(set_to_none=True)
    (ga, oa), (gb, ob) = grads
    assert torch.equal(oa, ob)
    assert set(ga) == set(gb) and "cls_token" in ga and "position_enc" in ga
    for k in ga:
        assert torch.isfinite(gb[k]).all() and torch.equal(ga[k], gb[k]), k
    assert bank.grad is None and not bank.requires_grad


# ---------------------------------------------------------------------------------------------------- 11. the pipeline passes
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from lstc_vad_amd.models import Classifier, Encoder, Regressor
    return pw.build(str(tmp_path_factory.mktemp("world")), Encoder, Regressor, Classifier)


def _load(world, enc_ckpt, enc_kw, head_ckpt, head_cls):
    from lstc_vad_amd.models import Encoder
    strip = lambda sd: {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    enc = Encoder(**enc_kw)
    enc.load_state_dict(strip(torch.load(world[enc_ckpt], map_location="cpu")), strict=True)
    head = head_cls(32)
    head.load_state_dict(strip(torch.load(world[head_ckpt], map_location="cpu")), strict=True)
    return enc.to(DEV).eval(), head.to(DEV).eval()


_loaded = {}


def _models(world, which):
    """The world's checkpoints on the GPU, loaded once (the world is built once per module; the weights are never modified)."""
    from lstc_vad_amd.models import Classifier, Regressor
    if which not in _loaded:
        _loaded[which] = {"ltn": lambda: _load(world, "ltn_sht_enc.ckpt", pw.LTN_SHT, "ltn_sht_cls.ckpt", Classifier),
                          "ucf": lambda: _load(world, "ltn_ucf_enc.ckpt", pw.LTN_UCF, "ltn_ucf_cls.ckpt", Classifier),
                          "stn": lambda: _load(world, "stn_sht_enc.ckpt", pw.STN_SHT, "stn_sht_reg.ckpt", Regressor)}[which]()
    return _loaded[which]


def _keys(txt, ucf=False):
    lines = open(txt).read().splitlines()
    return [l.split(" ")[0].split("/")[-1].split(".")[0] for l in lines] if ucf else [l.split(",")[0] for l in lines]


def _no_uploads(monkeypatch):
    """From here on a feature upload by a pass is an error: the resident passes must not call pipeline._dev."""
    from lstc_vad_amd import pipeline

    def boom(*a, **k):
        raise AssertionError("pipeline._dev called: a feature was uploaded after the resident set was built")
    monkeypatch.setattr(pipeline, "_dev", boom)


def _two(run):
    """``run(rank, world, exchange)`` as two emulated ranks in one process -> rank 0's result."""
    kept = {}
    run(1, 2, lambda flat: kept.__setitem__(1, flat.clone()))
    return run(0, 2, lambda flat: flat.add_(kept[1]))


def _owns(rank, world_size):
    return None if world_size is None else (lambda i: i % world_size == rank)


def _same_frames(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[1].dtype == b[1].dtype


def _same_labels(a, b):
    return list(a) == list(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("dialect", ["SHT", "UBnormal"])
def test_evaluate_auc_resident_is_bitwise_the_host_fed_pass(world, dialect, monkeypatch):
    from lstc_vad_amd import pipeline
    tag = "sht" if dialect == "SHT" else "ubn"
    feats, txt, masks = world[tag + "_feats"], world[tag + "_test"], world[tag + "_masks"]
    keys = _keys(txt)
    runs = [("LTN", "ltn", False), ("LTN", "ltn", "unpadded"), ("STN", "stn", False)]

    def ev(mode, which, ragged, rs_of, r=None, w=None, ex=None):
        enc, head = _models(world, which)
        return pipeline.evaluate_auc(enc, head, mode, dialect, feats, txt, masks, 3, 16, return_frames=True, pool_sequences=5,
                                     ragged=ragged, rank=r, world=w, exchange=ex, resident=rs_of(r, w) if rs_of else None)
    host = [ev(m, wh, rg, None) for m, wh, rg in runs]
    make = lambda r, w: pipeline.ResidentSet.from_archive(feats, keys, DEV, n_patch=16, owns=_owns(r, w))
    whole = make(None, None)
    _no_uploads(monkeypatch)
    for (m, wh, rg), h in zip(runs, host):
        res = ev(m, wh, rg, lambda r, w: whole)
        print(dialect, m, rg, "max |score diff| %.3e, |dAUC| %.3e" % (float(np.abs(res[1] - h[1]).max()), abs(res[0] - h[0])))
        assert _same_frames(res, h), (dialect, m, rg)
        # two emulated ranks, each holding only the videos it scores
        two = _two(lambda r, w, ex: ev(m, wh, rg, make, r, w, ex))
        assert _same_frames(two, res), (dialect, m, rg, "two ranks")
    assert whole.bank.shape[0] == sum(whole.lens) and make(1, 2).bank.shape[0] == sum(whole.lens[1::2])


@pytest.mark.parametrize("dialect", ["SHT", "UBnormal"])
def test_generate_pseudo_labels_resident_is_bitwise_the_host_fed_pass(world, dialect, monkeypatch, tmp_path):
    from lstc_vad_amd import pipeline
    tag = "sht" if dialect == "SHT" else "ubn"
    feats, txt = world[tag + "_feats"], world[tag + "_train"]
    keys = _keys(txt)
    runs = [("LTN", "ltn", False, 0.45), ("LTN", "ltn", "unpadded", 0.45), ("STN", "stn", False, 0.34)]

    def gen(mode, which, ragged, thr, rs_of, r=None, w=None, ex=None, out_path=None):
        enc, head = _models(world, which)
        return pipeline.generate_pseudo_labels(enc, head, mode, dialect, feats, txt, thr, part_len=3 if mode == "LTN" else 1,
                                               pool_sequences=7, ragged=ragged, rank=r, world=w, exchange=ex, out_path=out_path,
                                               resident=rs_of(r, w) if rs_of else None)
    host = [gen(m, wh, rg, thr, None) for m, wh, rg, thr in runs]
    make = lambda r, w: pipeline.ResidentSet.from_archive(feats, keys, DEV, owns=_owns(r, w))      # the generators score every stored patch
    whole = make(None, None)
    _no_uploads(monkeypatch)
    for (m, wh, rg, thr), h in zip(runs, host):
        p = str(tmp_path / f"pl_{m}_{rg}.npy")
        res = gen(m, wh, rg, thr, lambda r, w: whole, out_path=p)
        assert list(res) == [k + ".npy" for k in keys]
        assert _same_labels(res, h), (dialect, m, rg)
        assert any((v > 0).any() for v in res.values()) and any((v == 0).any() for v in res.values())     # the threshold cuts
        assert _same_labels(np.load(p, allow_pickle=True).tolist(), h)
        assert _same_labels(_two(lambda r, w, ex: gen(m, wh, rg, thr, make, r, w, ex)), res), (dialect, m, rg, "two ranks")


@pytest.mark.parametrize("mode,which", [("LTN", "ltn"), ("STN", "stn")])
def test_evaluate_train_auc_from_the_training_bank_is_bitwise(world, mode, which, monkeypatch):
    """ResidentSet.from_pairs of a real ResidentPairs: the train-AUC pass reads the bank the training feed already holds."""
    from lstc_vad_amd import load_dataset as lds
    from lstc_vad_amd import pipeline
    np.random.seed(3)
    ds = lds.SH_Train_Origin_Dataset(part_num=3, part_len=3, h5_path=world["sht_feats"], train_txt=world["sht_train"], n_patch=16,
                                     sample="uniform")
    pairs = lds.ResidentPairs(ds, 2, DEV)
    rs = pipeline.ResidentSet.from_pairs(pairs)
    assert rs.bank.data_ptr() == pairs.bank.data_ptr() and len(rs) == len(pw.SHT_TRAIN)
    enc, head = _models(world, which)

    def tr(resident, r=None, w=None, ex=None):
        return pipeline.evaluate_train_auc(enc, head, mode, "SHT", world["sht_feats"], world["sht_train"], world["sht_masks"], 3, 16,
                                           return_frames=True, pool_sequences=6, rank=r, world=w, exchange=ex, resident=resident)
    host = tr(None)
    _no_uploads(monkeypatch)
    res = tr(rs)
    print(mode, "train AUC: max |score diff| %.3e, |dAUC| %.3e" % (float(np.abs(res[1] - host[1]).max()), abs(res[0] - host[0])))
    assert _same_frames(res, host)
    assert _same_frames(_two(lambda r, w, ex: tr(rs, r, w, ex)), res)


def test_ucf_resident_passes_track_the_host_fed_passes(world, monkeypatch):
    """The UCF dialect bins on the device (lstc_segment_mean: the clips of a bin are added in order, torch's mean adds them in
    another): labels identical, scores within 1e-4 - the project's fp32 score bar."""
    from lstc_vad_amd import pipeline
    enc, head = _models(world, "ucf")
    feats = world["ucf_feats"]
    test_keys, train_keys = _keys(world["ucf_test"], True), _keys(world["ucf_train"], True)

    def ev(rs_of, r=None, w=None, ex=None):
        return pipeline.evaluate_auc(enc, head, "LTN", "UCF", feats, world["ucf_test"], world["ucf_gt"], 2, 9, return_frames=True,
                                     pool_sequences=20, rank=r, world=w, exchange=ex, resident=rs_of(r, w) if rs_of else None)

    def gen(rs_of, r=None, w=None, ex=None):
        return pipeline.generate_pseudo_labels(enc, head, "LTN", "UCF", feats, world["ucf_train"], 0.25, part_len=2, n_patch=9,
                                               pool_sequences=20, rank=r, world=w, exchange=ex, resident=rs_of(r, w) if rs_of else None)
    h_ev, h_gen = ev(None), gen(None)
    mk_test = lambda r, w: pipeline.ResidentSet.from_archive(feats, test_keys, DEV, n_patch=9, view=True, owns=_owns(r, w))
    mk_train = lambda r, w: pipeline.ResidentSet.from_archive(feats, train_keys, DEV, n_patch=9, view=True, owns=_owns(r, w))
    _no_uploads(monkeypatch)
    r_ev = ev(mk_test)
    diff = float(np.abs(r_ev[1] - h_ev[1]).max())
    print("UCF evaluate: max |score diff| %.3e, |dAUC| %.3e" % (diff, abs(r_ev[0] - h_ev[0])))
    assert np.array_equal(r_ev[2], h_ev[2]) and r_ev[1].shape == h_ev[1].shape and r_ev[1].dtype == h_ev[1].dtype
    assert diff <= 1e-4
    assert _same_frames(_two(lambda r, w, ex: ev(mk_test, r, w, ex)), r_ev)
    r_gen = gen(mk_train)
    assert list(r_gen) == list(h_gen) == [k + ".npy" for k in train_keys]
    worst = 0.0
    for k in h_gen:
        a, b = h_gen[k], r_gen[k]
        assert a.shape == b.shape == (32, 1) and a.dtype == b.dtype == np.float32
        near = np.abs(np.where(a > 0, a, b) - 0.25) < 1e-4              # a score sitting on the threshold may fall on either side
        assert np.array_equal((a > 0)[~near], (b > 0)[~near]), k
        worst = max(worst, float(np.abs(a - b)[~near].max()))
    print("UCF generate: max |score diff| %.3e" % worst)
    assert worst <= 1e-4
    assert _same_labels(_two(lambda r, w, ex: gen(mk_train, r, w, ex)), r_gen)


# ---------------------------------------------------------------------------------------------------- the command line
def _cli(script_dir, script, argv):
    import subprocess
    root = os.path.dirname(HERE)
    return subprocess.run([sys.executable, script] + argv, cwd=os.path.join(root, script_dir), capture_output=True, text=True, timeout=600,
                          env=dict(os.environ, PYTHONPATH=root, HIP_VISIBLE_DEVICES="0"))


def test_resident_eval_flag_on_the_command_lines(world, tmp_path):
    """--resident_eval on a Train/ script (the test set uploaded once, the train AUC from the training bank), on the label generator
    and on the Test/ script: the same AUC lines, the same label file and the same AUC as without the flag, character for character."""
    model = ["--d_model", "32", "--n_head", "2", "--d_k", "16", "--d_v", "16", "--n_hidden", "64", "--MHA_layerNorm", "--FFN_layerNorm",
             "--relative_position_encoding", "--part_len", "3"]
    train = model + ["--dataset_path", world["sht_feats"], "--training_txt", world["sht_train"], "--testing_txt", world["sht_test"],
                     "--test_mask_dir", world["sht_masks"], "--batch_size", "2", "--part_num", "3", "--n_patch", "16", "--load_model",
                     "--lr_encoder", "0", "--lr_classifier", "0", "--epochs", "1", "--inter_epoch", "1", "--seed", "3",
                     "--save_threshold", "2", "--load_temporal_model_path", world["ltn_sht_enc.ckpt"], "--load_classifier_model_path",
                     world["ltn_sht_cls.ckpt"], "--saved_prefix", "pre_"]
    gen = model + ["--dataset", "SHT", "--dataset_path", world["sht_feats"], "--training_txt", world["sht_train"], "--temporal_model_path",
                   world["ltn_sht_enc.ckpt"], "--classifier_model_path", world["ltn_sht_cls.ckpt"], "--threshold", "0.45"]
    ev = ["--d_model", "32", "--temporal_n_head", "2", "--temporal_d_k", "16", "--temporal_d_v", "16", "--temporal_n_hidden", "64",
          "--temporal_MHA_layerNorm", "--temporal_FFN_layerNorm", "--temporal_relative_position_encoding", "--part_len", "3", "--dataset", "SHT",
          "--dataset_path", world["sht_feats"], "--testing_txt", world["sht_test"], "--test_mask_dir", world["sht_masks"],
          "--temporal_model_path", world["ltn_sht_enc.ckpt"], "--classifier_model_path", world["ltn_sht_cls.ckpt"]]
    auc_lines = lambda err: [l.split(": ", 1)[-1] for l in err.splitlines() if "_AUC" in l]      # the train AUC is the log record's second line
    got = {}
    for tag, flag in (("host", []), ("resident", ["--resident_eval"])):
        save = str(tmp_path / f"ck_{tag}") + os.sep
        r = _cli("Train", "temporal_transformer_shanghaitech.py", train + flag + ["--model_save_dir", save, "--log_dir", str(tmp_path / f"log_{tag}")])
        assert r.returncode == 0, r.stderr[-2500:]
        p = str(tmp_path / f"pl_{tag}.npy")
        g = _cli("Train", "pseudo_labels_generator_temporal.py", gen + flag + ["--pseudo_labels_path", p])
        assert g.returncode == 0, g.stderr[-2000:]
        e = _cli("Test", "evaluation_shanghaitech_ubnormal.py", ev + flag)
        assert e.returncode == 0, e.stderr[-2000:]
        got[tag] = (auc_lines(r.stderr), np.load(p, allow_pickle=True).tolist(), e.stdout.strip().split("auc = ")[-1])
    (a_auc, a_pl, a_ev), (b_auc, b_pl, b_ev) = got["host"], got["resident"]
    assert a_auc and any("train_AUC" in l for l in a_auc) and a_auc == b_auc, (a_auc, b_auc)
    assert _same_labels(a_pl, b_pl) and len(a_pl) == len(pw.SHT_TRAIN)
    assert a_ev == b_ev and 0.0 <= float(a_ev) <= 1.0
