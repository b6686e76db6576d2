"""Layer-0 Q / K / V weight gradients over the distinct rows of a batch (exact-f32 mode).

The forward projects Xu, the distinct rows of the batch, and spreads the result over the tokens (tests/test_dedup_rows_gpu.py).  The
backward mirrors it: ``lstc_segment_sum_rows`` adds up the rows of dQ, dK, dV that share an input row - fixed order, no atomics - and
the weight gradients contract those sums with Xu, padded with zero rows to a multiple of 512 so that ``wgrad`` keeps its batched
deterministic split.  Checked here: the kernel against a sequential float32 restatement (bitwise), its refusals, the CSR of
``feed.LazyRows.row_csr`` against numpy, layer 0 with the path on and off against dQ^T X in float64 within the GEMM tests' bound and
bitwise everywhere else, and the gate.

Shapes are those of tests/test_dedup_rows_gpu.py, whose helpers are used: d = 128, 4 heads x 32, P = 4, L = 3, 32 sequences x 13
tokens = 416 rows, four 10-clip videos.  The product path takes the weight gradients over distinct rows only from
``functional.WGRAD_SPLIT_MIN_ROWS`` = 4096 contracted rows on; the layer tests lower that boundary to 256."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import util_gemm as ug                                                   # noqa: E402
from test_dedup_rows_gpu import BS, D, DEV, DK, GUARD, H, L, P, PN, _bank, _encoder, _maps, _windows      # noqa: E402

gpu = pytest.mark.gpu
LOW_ROWS = 256


def _csr_of(m, groups):
    """order, ptr of a row map in numpy: tokens sorted by row, ascending inside a row."""
    return np.argsort(m, kind="stable").astype(np.int32), np.concatenate([[0], np.cumsum(np.bincount(m, minlength=groups))]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the kernel
@gpu
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("pad", [0, 8], ids=["ld=cols", "ld>cols"])
@pytest.mark.parametrize("extra", [0, 5], ids=["dst_rows=U", "dst_rows=U+5"])
def test_segment_sum_rows_is_the_sequential_f32_sum(n, pad, extra):
    """dst_j[u, :] = the float32 sum, in ascending token order from the first token's value, of src_j[m, :] over map[m] = u, for
    n = 1 and 3 matrices in one launch, sources of 1 and 49 rows, groups of 1, 2, ~5 and 49 tokens, with ld == cols and ld > cols on
    both sides; rows behind the groups are exact zeros, guard rows and guard columns stay as they were."""
    from lstc_vad_amd import functional as Fn
    g = torch.Generator(device=DEV).manual_seed(2)
    maps = dict(_maps(), **{"one group of 49": (np.zeros(49, np.int64), 1)})
    for name, (m, groups) in maps.items():
        rows = len(m)
        order, ptr = (torch.from_numpy(t).to(DEV) for t in _csr_of(m, groups))
        srcs = [torch.randn(rows, D + pad, device=DEV, generator=g)[:, :D] for _ in range(n)]
        full = [torch.full((groups + extra + 2, D + pad), GUARD, device=DEV) for _ in range(n)]
        Fn.segment_sum_rows(srcs, [f[1:-1, :D] for f in full], order, ptr)
        torch.cuda.synchronize()
        for s, f in zip(srcs, full):
            sh, want = s.cpu().numpy(), np.zeros((groups + extra, D), np.float32)
            seen = np.zeros(groups, bool)
            for tok in range(rows):                       # ascending token order, float32 adds, the first token's value as it is
                u = int(m[tok])
                want[u] = sh[tok] if not seen[u] else (want[u] + sh[tok]).astype(np.float32)
                seen[u] = True
            got = f[1:-1, :D].cpu().numpy()
            assert np.array_equal(got.view(np.uint32)[:groups], want.view(np.uint32)[:groups]), name
            assert not got[groups:].any() and not np.signbit(got[groups:]).any(), name                 # pad rows: +0.0
            for u in np.flatnonzero(np.bincount(m, minlength=groups) == 1):
                assert np.array_equal(got[u].view(np.uint32), sh[int(np.flatnonzero(m == u)[0])].view(np.uint32)), name
            assert bool((f[0] == GUARD).all()) and bool((f[-1] == GUARD).all()) and bool((f[:, D:] == GUARD).all()), name


@gpu
def test_segment_sum_rows_refusals_come_by_return_code():
    from lstc_vad_amd import _lib
    lib = _lib.load()
    src, dst = torch.ones(8, 16, device=DEV), torch.full((8, 16), GUARD, device=DEV)
    order = torch.arange(8, dtype=torch.int32, device=DEV)
    ptr = torch.arange(9, dtype=torch.int32, device=DEV)

    def call(sp, dp, n, cols, ld=16, op=order.data_ptr(), pp=ptr.data_ptr(), src_rows=8, groups=8, dst_rows=8, ld_dst=None, arrays=True):
        k = max(1, min(n, 4))
        arr = lambda t, v: (t * k)(*[v] * k) if arrays else None
        return lib.lstc_segment_sum_rows(arr(C.c_void_p, sp), arr(C.c_int64, ld), arr(C.c_void_p, dp),
                                         arr(C.c_int64, ld if ld_dst is None else ld_dst), n, op, pp, src_rows, groups, dst_rows, cols, None)
    E_NULL, E_SHAPE, E_ALIGN = -1, -2, -3
    s, d = src.data_ptr(), dst.data_ptr()
    assert call(s + 4, d, 1, 12) == E_ALIGN                        # misaligned source
    assert call(s, d + 8, 1, 12) == E_ALIGN                        # misaligned destination
    assert call(s, d, 1, 16, ld=18) == E_ALIGN                     # row stride not a multiple of 4
    assert call(s, d, 1, 14) == E_SHAPE                            # cols % 4
    assert call(s, d, 1, 0) == E_SHAPE
    assert call(s, d, 4, 16) == E_SHAPE                            # n = 4
    assert call(s, d, 0, 16) == E_SHAPE
    assert call(s, d, 1, 16, ld=12) == E_SHAPE                     # source row stride below cols
    assert call(s, d, 1, 16, ld_dst=12) == E_SHAPE                 # destination row stride below cols
    assert call(s, d, 1, 16, src_rows=0) == E_SHAPE
    assert call(s, d, 1, 16, groups=0) == E_SHAPE
    assert call(s, d, 1, 16, dst_rows=-1) == E_SHAPE
    assert call(s, d, 1, 16, dst_rows=7) == E_SHAPE                # fewer destination rows than groups
    assert call(s, d, 1, 16, dst_rows=2 ** 31) == E_SHAPE
    assert call(None, d, 1, 16) == E_NULL
    assert call(s, None, 1, 16) == E_NULL
    assert call(s, d, 1, 16, op=None) == E_NULL
    assert call(s, d, 1, 16, pp=None) == E_NULL
    assert call(s, d, 1, 16, arrays=False) == E_NULL
    torch.cuda.synchronize()
    assert lib.lstc_strerror(E_ALIGN) and bool((dst == GUARD).all())           # nothing was written


# ------------------------------------------------------------------------------------------------ the CSR (host)
@pytest.mark.parametrize("length", [10, 30, 200])
@pytest.mark.parametrize("learned_cls", [False, True], ids=["n_cls=N", "n_cls=1"])
def test_row_csr_restated_in_numpy(length, learned_cls):
    """``LazyRows.row_csr`` is ``row_map`` turned round: ``order`` a permutation of the tokens sorted by their row of Xu, ascending
    inside a row (stable), ``ptr`` the running ``np.bincount`` of the map - with the host's stable argsort of the clip slots and
    with the one formed on the tensor's own device, for a CLS row per sequence and for one shared CLS row (a group of N tokens)."""
    from lstc_vad_amd.feed import LazyRows, unique_clips
    idx, clips = _windows([[length] * BS, [length] * BS])
    uniq, inv = unique_clips(idx)
    N, S = idx.size // L, 1 + L * P
    n_cls = 1 if learned_cls else N
    U = n_cls + len(uniq) * P
    bank = torch.zeros(clips, P, 4)
    for so in (None, torch.from_numpy(np.argsort(inv, kind="stable"))):
        lazy = LazyRows(bank, torch.from_numpy(idx.reshape(-1)), 0, BS, PN * L, torch.from_numpy(uniq), torch.from_numpy(inv), len(uniq),
                        slot_order=so)
        rmap = lazy.row_map(L, n_cls).numpy()
        order, ptr = lazy.row_csr(L, n_cls)
        assert lazy.row_csr(L, n_cls)[0] is order                 # cached like the map
        assert order.dtype == torch.int32 and ptr.dtype == torch.int32 and order.shape == (N * S,) and ptr.shape == (U + 1,)
        order, ptr = order.numpy(), ptr.numpy()
        assert np.array_equal(np.sort(order), np.arange(N * S))                                   # a permutation
        assert np.array_equal(ptr, np.concatenate([[0], np.cumsum(np.bincount(rmap, minlength=U))]))
        for u in range(U):
            grp = order[ptr[u]:ptr[u + 1]]
            assert len(grp) >= 1 and np.all(rmap[grp] == u) and np.all(np.diff(grp) > 0)           # one row's tokens, ascending
        assert np.array_equal(order, np.argsort(rmap, kind="stable"))
        if learned_cls:
            assert ptr[1] == N and np.array_equal(order[:N], np.arange(N) * S)                   # the one group of N CLS tokens


# ------------------------------------------------------------------------------------------------ layer 0
def _layer0_step(enc, bank, idx, monkeypatch, env, low=True, rows_boundary=LOW_ROWS):
    """Forward + backward of layer 0 on the fused gather's input with a fixed upstream gradient.  -> what the node returned, the
    gradient of every parameter it reaches, dQ / dK / dV as the attention backward wrote them, the token rows X, and how often
    the segment sum, the batched and the atomic split-K weight-gradient forms ran."""
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.feed import ResidentBank
    monkeypatch.setenv("LSTC_DEDUP_ROWS", env)
    if low:
        monkeypatch.setattr(Fn, "WGRAD_SPLIT_MIN_ROWS", rows_boundary)
    seen, calls = [], {"segsum": 0, "batched": 0, "atomic": 0}
    real_bwd, real_sum, real_batched, real_gemm = Fn.attn_bwd, Fn.segment_sum_rows, Fn.gemm_batched, Fn.gemm

    def bwd_spy(*a, **kw):
        r = real_bwd(*a, **kw)
        seen.append(tuple(t.clone() for t in (kw["out"] if kw.get("out") is not None else r[:3])))
        return r

    def sum_spy(*a, **kw):
        calls["segsum"] += 1
        return real_sum(*a, **kw)

    def batched_spy(*a, **kw):
        calls["batched"] += 1
        return real_batched(*a, **kw)

    def gemm_spy(*a, **kw):
        calls["atomic"] += int(kw.get("split_k", 1) > 1)
        return real_gemm(*a, **kw)
    monkeypatch.setattr(Fn, "attn_bwd", bwd_spy)
    monkeypatch.setattr(Fn, "segment_sum_rows", sum_spy)
    monkeypatch.setattr(Fn, "gemm_batched", batched_spy)
    monkeypatch.setattr(Fn, "gemm", gemm_spy)
    (nf, af), = ResidentBank(bank).gather(idx, lazy=True)
    Fn.reset_rng()
    enc.zero_grad(set_to_none=True)
    x = enc._embed((bank, nf.idx_flat, idx.size // L, L, nf))
    out, probs = enc.layer_stack[0](x, return_attn=True)[:2]
    up = torch.randn(out.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9))
    out.backward(up)
    Fn.drop_producer_packs()
    torch.cuda.synchronize()
    monkeypatch.undo()
    grads = {k: p.grad.detach().clone() for k, p in enc.named_parameters() if p.grad is not None}
    return dict(out=out.detach(), probs=probs.detach(), grads=grads, dqkv=seen[0], x=x.detach().reshape(-1, D), calls=calls, lazy=nf)


def _is_qkv(name):
    return any(w in name for w in ("w_qs", "w_ks", "w_vs"))


@gpu
@pytest.mark.parametrize("fuse", [False, True], ids=["separate", "fused_qkv"])
@pytest.mark.parametrize("learned_cls", [False, True], ids=["mean_cls", "learned_cls"])
def test_layer0_weight_gradients_over_distinct_rows(fuse, learned_cls, monkeypatch):
    """Path on against LSTC_DEDUP_ROWS=0, dropout 0.1, 416 token rows in at most 32 + 40 * 4 (mean CLS) or 1 + 40 * 4 (learned CLS,
    one group of 32 tokens) distinct rows, contracted over 512 padded rows.  dW_q, dW_k, dW_v of BOTH arms lie within
    util_gemm.tolerance of dQ^T X in float64, formed from the attention backward's own dQ, dK, dV and the token rows - the bound of
    tests/test_gemm_f64_gpu.py, from the reference side alone.  (A CPU emulation of this grouping puts the pre-summed form at
    0.02 - 0.06 of that bound: a miss is a bug.)  Everything else is bitwise equal between the arms: output, probabilities, dQ / dK
    / dV, and the gradient of every other parameter (fc, LayerNorms, bias table, FFN, the learned CLS token)."""
    enc = _encoder(fuse, learned_cls, drop=0.1)
    idx, clips = _windows([[10] * BS, [10] * BS])
    bank = _bank(clips)
    on = _layer0_step(enc, bank, idx, monkeypatch, "1")
    off = _layer0_step(enc, bank, idx, monkeypatch, "0")
    assert on["calls"]["segsum"] == 1 and off["calls"]["segsum"] == 0
    assert on["calls"]["atomic"] == 0 and off["calls"]["atomic"] == 0 and on["calls"]["batched"] >= (1 if fuse else 3)
    assert torch.equal(on["out"], off["out"]) and torch.equal(on["probs"], off["probs"]) and torch.equal(on["x"], off["x"])
    for a, b in zip(on["dqkv"], off["dqkv"]):
        assert torch.equal(a, b)
    assert set(on["grads"]) == set(off["grads"]) and sum(_is_qkv(k) for k in on["grads"] if "layer_stack.0." in k) == 3
    X = on["x"].cpu()
    for name in sorted(on["grads"]):
        if not (_is_qkv(name) and "layer_stack.0." in name):
            assert torch.equal(on["grads"][name], off["grads"][name]), name
            continue
        dy = on["dqkv"]["qkv".index(name.split("w_")[1][0])].cpu()
        A = dy.t().contiguous()
        ref = ug.ref64(A, X)
        tol = ug.tolerance(ref, ug.eval32(A, X), ug.terms_abs(A, X))
        for arm, res in (("on", on), ("off", off)):
            err = float((res["grads"][name].cpu().to(torch.float64) - ref).abs().max())
            print(f"{name} [{arm}]: max |dW - ref64| = {err:.3e}, tolerance {tol:.3e}, ratio {err / tol:.3f}")
            assert err <= tol, (name, arm, err, tol)


# ------------------------------------------------------------------------------------------------ the gate
@gpu
def test_gate_keeps_the_token_rows(monkeypatch):
    """The segment sum never runs: with the default constants at this shape (512 padded rows < 4096), on a batch without repeats,
    and under LSTC_DEDUP_ROWS=0."""
    enc = _encoder(False, drop=0.1)
    idx, clips = _windows([[10] * BS, [10] * BS])
    bank = _bank(clips)
    assert _layer0_step(enc, bank, idx, monkeypatch, "1", low=False)["calls"]["segsum"] == 0
    assert _layer0_step(enc, bank, idx, monkeypatch, "0")["calls"]["segsum"] == 0
    bank2 = _bank(100, seed=4)
    idx_uni = np.random.RandomState(2).permutation(100)[:2 * BS * PN * L].reshape(2, BS, PN * L).astype(np.int64)
    res = _layer0_step(enc, bank2, idx_uni, monkeypatch, "1")
    assert res["lazy"].n_unique == idx_uni.size and res["calls"]["segsum"] == 0


@gpu
def test_padded_rows_keep_the_batched_split(monkeypatch):
    """Videos of 10, 30, 17 and 12 clips: U = 32 + 4 * distinct clips is no multiple of the split factor 16 that ``wgrad`` picks for a
    [128, 128] gradient.  Contracted over U' = U rounded up to 512 rows the three products still take the deterministic batched
    split - never the atomic split-K form - and two runs give equal bits."""
    from lstc_vad_amd import functional as Fn
    enc = _encoder(False, drop=0.1)
    idx, clips = _windows([[10, 30], [17, 12]])
    bank = _bank(clips)
    a = _layer0_step(enc, bank, idx, monkeypatch, "1", rows_boundary=128)
    b = _layer0_step(enc, bank, idx, monkeypatch, "1", rows_boundary=128)
    U = 32 + a["lazy"].n_unique * P
    assert Fn._wgrad_split(H * DK, D) == 16 and U % 16 != 0 and U < 416
    assert a["calls"] == b["calls"] and a["calls"]["segsum"] == 1 and a["calls"]["atomic"] == 0 and a["calls"]["batched"] >= 3
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k
