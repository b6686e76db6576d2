"""Layer-0 Q / K / V projections on the distinct rows of a batch (exact-f32 mode).

The window sampler's parts overlap whenever a video has fewer clips than part_num * part_len, so one (clip, patch) bank row sits in
several sequences.  Layer 0 has no LayerNorm in front of its projections: ``feed.ResidentBank.gather(lazy=True)`` finds the batch's
distinct clips on the host, ``MHAFunction`` projects Xu = [CLS rows; bank[distinct clips]] and ``lstc_expand_rows`` writes the
ordinary [M, H d_k] Q, K, V.  Everything here is an equality: the kernel against ``torch.index_select``, the map against a numpy
restatement, Q / K / V, the step's scalars and every weight against the same run with ``LSTC_DEDUP_ROWS=0``.

Shapes: d = 128, 4 heads x 32, P = 4, L = 3, pn = 8, bs = 2, a bank of 40 clips (four videos of 10).  A batch of 2 * bs * pn * L = 96
clip slots cannot be free of repeats on 40 clips, so the batch without duplicates draws its 96 clips from a bank of 100."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

gpu = pytest.mark.gpu
DEV = torch.device("cuda", 0) if torch.cuda.is_available() else None
D, H, DK, P, L, PN, BS = 128, 4, 32, 4, 3, 8, 2
GUARD = -7.0


def _windows(lengths):
    """[2, BS, PN * L] clip indices from the reference's window sampler, video v of kind k = clips offset[k, v] .. + lengths[k][v]."""
    from lstc_vad_amd.load_dataset import window_indices
    keep = np.random.get_state()
    np.random.seed(11)
    try:
        idx, off = np.empty((2, BS, PN * L), np.int64), 0
        for k in range(2):
            for v in range(BS):
                idx[k, v] = window_indices(lengths[k][v], PN, L, "uniform") + off
                off += lengths[k][v]
    finally:
        np.random.set_state(keep)
    return idx, off


def _bank(clips, seed=3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return 0.5 * torch.relu(torch.randn(clips, P, D, device=DEV, generator=g))


# ------------------------------------------------------------------------------------------------ the kernel
def _maps():
    rs = np.random.RandomState(5)
    return {
        "one row": (np.zeros(1, np.int64), 1),
        "every row repeated": (np.repeat(np.arange(25), 2)[:49], 25),
        "identity": (np.arange(49), 49),
        "cls + 7 clips": (np.concatenate([[0], 1 + rs.randint(0, 3, 7).repeat(P) * P + np.tile(np.arange(P), 7)]), 1 + 3 * P),
        "random": (rs.randint(0, 9, 49), 9),
    }


@gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("pad", [0, 8], ids=["ld=cols", "ld>cols"])
def test_expand_rows_is_index_select(n, pad):
    """dst_j[m, :] = src_j[map[m], :] for n = 1 and 3 matrices in one launch, rows = 1, 49 (13 workgroups of four rows) and 1 + 7 * 4,
    with ld == cols and ld > cols on both sides; destination rows sit between guard rows and, with ld > cols, guard columns, all of
    which stay as they were."""
    from lstc_vad_amd import functional as Fn
    g = torch.Generator(device=DEV).manual_seed(2)
    for name, (m, src_rows) in _maps().items():
        rows = len(m)
        dmap = torch.from_numpy(m.astype(np.int32)).to(DEV)
        srcs = [torch.randn(src_rows, D + pad, device=DEV, generator=g)[:, :D] for _ in range(n)]
        full = [torch.full((rows + 2, D + pad), GUARD, device=DEV) for _ in range(n)]
        Fn.expand_rows(srcs, [f[1:-1, :D] for f in full], dmap)
        torch.cuda.synchronize()
        for s, f in zip(srcs, full):
            assert torch.equal(f[1:-1, :D], torch.index_select(s, 0, dmap.long())), name
            assert bool((f[0] == GUARD).all()) and bool((f[-1] == GUARD).all()) and bool((f[:, D:] == GUARD).all()), name


@gpu
def test_expand_rows_refusals_come_by_return_code():
    from lstc_vad_amd import _lib
    lib = _lib.load()
    src, dst = torch.zeros(8, 16, device=DEV), torch.zeros(8, 16, device=DEV)
    dmap = torch.zeros(8, dtype=torch.int32, device=DEV)

    def call(sp, dp, n, cols, ld=16, mp=dmap.data_ptr(), rows=8):
        k = max(1, min(n, 4))
        return lib.lstc_expand_rows((C.c_void_p * k)(*[sp] * k), (C.c_int64 * k)(*[ld] * k), (C.c_void_p * k)(*[dp] * k),
                                    (C.c_int64 * k)(*[ld] * k), n, mp, rows, cols, None)
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    assert call(src.data_ptr(), dst.data_ptr(), 1, 16, rows=1) == 0
    assert call(src.data_ptr() + 4, dst.data_ptr(), 1, 12) == E_ALIGN          # misaligned source
    assert call(src.data_ptr(), dst.data_ptr() + 8, 1, 12) == E_ALIGN          # misaligned destination
    assert call(src.data_ptr(), dst.data_ptr(), 1, 14) == E_SHAPE              # cols % 4
    assert call(src.data_ptr(), dst.data_ptr(), 4, 16) == E_SHAPE              # n = 4
    assert call(src.data_ptr(), dst.data_ptr(), 0, 16) == E_SHAPE
    assert call(src.data_ptr(), dst.data_ptr(), 1, 16, ld=18) == E_ALIGN       # row stride not a multiple of 4
    assert call(src.data_ptr(), dst.data_ptr(), 1, 16, ld=12) == E_SHAPE       # row stride below cols
    assert call(src.data_ptr(), dst.data_ptr(), 1, 16, rows=0) == E_SHAPE
    assert call(src.data_ptr(), dst.data_ptr(), 1, 16, rows=2 ** 31 + 1) == E_SHAPE
    assert call(None, dst.data_ptr(), 1, 16) == E_NULL
    assert call(src.data_ptr(), dst.data_ptr(), 1, 16, mp=None) == E_NULL
    torch.cuda.synchronize()
    assert lib.lstc_strerror(E_ALIGN) and bool((dst == 0).all())


# ------------------------------------------------------------------------------------------------ the map (host)
@pytest.mark.parametrize("length", [10, 30, 200])
@pytest.mark.parametrize("learned_cls", [False, True])
def test_row_map_restated_in_numpy(length, learned_cls):
    """``feed.unique_clips`` + ``LazyRows.row_map`` on overlapping windows from ``window_indices``: Xu[map] is the gathered and
    concatenated batch, for one shared CLS row (a learned token: row 0) and for one CLS row per sequence (the token mean: row n)."""
    from lstc_vad_amd.feed import LazyRows, unique_clips
    idx, clips = _windows([[length] * BS, [length] * BS])
    rs = np.random.RandomState(1)
    bank = rs.rand(clips, P, D).astype(np.float32)
    uniq, inv = unique_clips(idx)
    assert np.array_equal(uniq, np.unique(idx)) and np.array_equal(uniq[inv], idx.reshape(-1))
    assert len(uniq) < idx.size or length > 10          # 24 window rows out of 10 clips: repeats for certain
    N, S = idx.size // L, 1 + L * P
    lazy = LazyRows(torch.from_numpy(bank), torch.from_numpy(idx.reshape(-1)), 0, BS, PN * L, torch.from_numpy(uniq),
                    torch.from_numpy(inv), len(uniq))
    n_cls = 1 if learned_cls else N
    got = lazy.row_map(L, n_cls)
    assert got.dtype == torch.int32 and got.shape == (N * S,) and lazy.row_map(L, n_cls) is got
    # numpy restatement, token by token
    want = np.empty((N, S), np.int64)
    place = {int(c): u for u, c in enumerate(uniq)}
    for n in range(N):
        want[n, 0] = 0 if learned_cls else n
        for s in range(1, S):
            want[n, s] = n_cls + place[int(idx.reshape(-1)[n * L + (s - 1) // P])] * P + (s - 1) % P
    assert np.array_equal(got.numpy(), want.reshape(-1))
    # Xu[map] == the gathered, concatenated batch
    tokens = bank[idx.reshape(-1)].reshape(N, L * P, D)
    cls = rs.rand(1, D).astype(np.float32) if learned_cls else tokens.mean(1)
    batch = np.concatenate([np.broadcast_to(cls[:, None, :], (N, 1, D)) if learned_cls else cls[:, None, :], tokens], 1)
    xu = np.concatenate([cls, bank[uniq].reshape(-1, D)], 0)
    assert np.array_equal(xu[got.numpy()], batch.reshape(N * S, D))


# ------------------------------------------------------------------------------------------------ layer 0
def _encoder(fuse, learned_cls=False, drop=0.0):
    from lstc_vad_amd.models import Encoder
    torch.manual_seed(1)
    enc = Encoder(n_layers=3, n_head=H, d_k=DK, d_v=DK, d_model=D, d_inner=2 * D, MHA_attn_dropout=drop, MHA_fc_dropout=drop,
                  FFN_dropout=drop, MHA_layerNorm=True, FFN_layerNorm=True, relative_pe=True, window_size=2, window_depth=L,
                  CLS_learned=learned_cls).to(DEV).train()
    if fuse:
        for layer in enc.layer_stack[:-1]:
            layer.slf_attn.fuse_qkv_()
    return enc


def _layer0_qkv(enc, bank, idx, monkeypatch, env):
    """Q, K, V as layer 0's attention core receives them, and how often lstc_expand_rows / the fused gather ran."""
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.feed import ResidentBank
    monkeypatch.setenv("LSTC_DEDUP_ROWS", env)
    seen, calls = [], {"expand": 0, "gather": 0}
    real_attn, real_expand, real_gather = Fn.attn_fwd, Fn.expand_rows, Fn.ClsConcatFunction._forward_gather

    def attn_spy(q, k, v, *a, **kw):
        seen.append(tuple(t.clone() for t in (q, k, v)))
        return real_attn(q, k, v, *a, **kw)

    def expand_spy(*a, **kw):
        calls["expand"] += 1
        return real_expand(*a, **kw)

    def gather_spy(*a, **kw):
        calls["gather"] += 1
        return real_gather(*a, **kw)
    monkeypatch.setattr(Fn, "attn_fwd", attn_spy)
    monkeypatch.setattr(Fn, "expand_rows", expand_spy)
    monkeypatch.setattr(Fn.ClsConcatFunction, "_forward_gather", staticmethod(gather_spy))
    (nf, af), = ResidentBank(bank).gather(idx, lazy=True)
    Fn.reset_rng()
    x = enc._embed((bank, nf.idx_flat, idx.size // L, L, nf))
    enc.layer_stack[0](x)
    Fn.drop_producer_packs()
    torch.cuda.synchronize()
    monkeypatch.undo()
    return seen[0], calls, nf


@gpu
@pytest.mark.parametrize("fuse", [False, True], ids=["separate", "fused_qkv"])
@pytest.mark.parametrize("learned_cls", [False, True], ids=["mean_cls", "learned_cls"])
def test_layer0_qkv_are_bitwise_the_full_projections(fuse, learned_cls, monkeypatch):
    """Path on against LSTC_DEDUP_ROWS=0 on a batch whose four videos have 10 clips each (24 window rows out of 10 clips) and on a batch
    without repeats; on the second the ordinary projections run and lstc_expand_rows is never called."""
    enc = _encoder(fuse, learned_cls)
    idx_dup, clips = _windows([[10] * BS, [10] * BS])
    assert clips == 40
    bank = _bank(clips)
    on, c_on, lazy = _layer0_qkv(enc, bank, idx_dup, monkeypatch, "1")
    off, c_off, _ = _layer0_qkv(enc, bank, idx_dup, monkeypatch, "0")
    assert lazy.n_unique <= 40 < idx_dup.size
    assert c_on == {"expand": 1, "gather": 1} and c_off == {"expand": 0, "gather": 1}
    for a, b in zip(on, off):
        assert a.shape == (idx_dup.size // L * (1 + L * P), H * DK) and torch.equal(a, b)
    bank2 = _bank(100, seed=4)
    idx_uni = np.random.RandomState(2).permutation(100)[:2 * BS * PN * L].reshape(2, BS, PN * L).astype(np.int64)
    on, c_on, lazy = _layer0_qkv(enc, bank2, idx_uni, monkeypatch, "1")
    off, c_off, _ = _layer0_qkv(enc, bank2, idx_uni, monkeypatch, "0")
    assert lazy.n_unique == idx_uni.size
    assert c_on == c_off == {"expand": 0, "gather": 1}
    for a, b in zip(on, off):
        assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("fuse", ["off", "on"])
def test_two_steps_are_bitwise_the_steps_without_the_path(fuse, monkeypatch):
    """Two TrainStep steps in exact f32 on LazyRows with dropout on: the five scalars of both steps and every weight, path on against
    LSTC_DEDUP_ROWS=0."""
    from argparse import Namespace
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.engine import TrainStep
    from lstc_vad_amd.feed import ResidentBank
    from lstc_vad_amd.models import Classifier
    lengths = [[[10, 30], [10, 17]], [[30, 10], [12, 10]]]
    rs = np.random.RandomState(4)
    labs = [rs.rand(BS, PN * L, 1).astype(np.float32) for _ in range(2)]

    def run(env):
        monkeypatch.setenv("LSTC_DEDUP_ROWS", env)
        calls = []
        real = Fn.expand_rows
        monkeypatch.setattr(Fn, "expand_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        enc = _encoder(False, drop=0.1)
        head = Classifier(D, 0.3).to(DEV).train()
        args = Namespace(batch_size=BS, part_num=PN, part_len=L, n_patch=P, lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8,
                         temporal_only=False, clip_grad=False)
        Fn.reset_rng()
        ts = TrainStep(args, "LTN", enc, head, 1e-5, 1e-4, 1e-3, fuse_qkv=fuse)
        out = []
        for lens, lab in zip(lengths, labs):
            idx, clips = _windows(lens)
            (nf, af), al = ResidentBank(_bank(clips)).gather(idx, lab, lazy=True)
            out.append(ts.step(nf, af, al).clone())
        torch.cuda.synchronize()
        monkeypatch.undo()
        return out, {k: v.detach().clone() for k, v in list(enc.state_dict().items()) + list(head.state_dict().items())}, len(calls)
    a, wa, na = run("1")
    b, wb, nb = run("0")
    assert (na, nb) == (2, 0)
    for x, y in zip(a, b):
        assert x.numel() == 5 and torch.equal(x, y), (x, y)
    for k in wa:
        assert torch.equal(wa[k], wb[k]), k
