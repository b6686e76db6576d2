"""Shared helpers for the parity tests: load a golden case, build oracle configs, the float64 attention reference."""
import os

import numpy as np
import torch

from cases import CASES
from oracle import lstc_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    mode, enc_kw, st_kw = CASES[name]
    return z, mode, dict(enc_kw), dict(st_kw)


def sub(z, prefix, as_torch=True):
    out = {}
    for k in z.files:
        if k.startswith(prefix):
            v = z[k]
            out[k[len(prefix):]] = torch.from_numpy(np.array(v)) if as_torch else np.array(v)
    return out


def oracle_cfgs(mode, enc_kw, st_kw, dropout=0.0):
    ecfg = orc.EncoderCfg(n_layers=3, MHA_attn_dropout=dropout, MHA_fc_dropout=dropout, FFN_dropout=dropout,
                          position_dropout=dropout, **enc_kw)
    st = orc.StepCfg(mode=mode, head_dropout=dropout, **st_kw)
    return ecfg, st


def max_abs_diff(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def host_dropout_keep(i, p, seed):
    """numpy restatement of the library's counter-based keep/drop rule (csrc/lstc_common.h: drop_key_mix = splitmix64's
    finaliser over the 64-bit seed, drop_hash = two-multiply avalanche of the flat element index): True where element ``i``
    is kept.  Part of the ABI contract - masks are replayed by tests."""
    m = (1 << 64) - 1
    zz = (int(seed) + 0x9E3779B97F4A7C15) & m
    zz = ((zz ^ (zz >> 30)) * 0xBF58476D1CE4E5B9) & m
    zz = ((zz ^ (zz >> 27)) * 0x94D049BB133111EB) & m
    zz ^= zz >> 31
    k0, k1, thr = zz & 0xffffffff, zz >> 32, min(int(p * 4294967296.0), 0xffffffff)
    u, lo = np.uint64, np.uint64(0xffffffff)
    h = (np.asarray(i).astype(np.uint64) ^ u(k0)) & lo
    h = (h * u(0x9E3779B1)) & lo
    h ^= h >> u(15)
    h = (h + u(k1)) & lo
    h = (h * u(0x85EBCA77)) & lo
    h ^= h >> u(13)
    h = (h * u(0xC2B2AE3D)) & lo
    h ^= h >> u(16)
    return h >= u(thr)


def attn_reference(q, k, v, do, N, S, H, dk, dv, table, index, keep, p_drop, cut_key=None):
    """float64 restatement of the attention contract (include/lstc_hip.h, "attention"), computed by torch autograd on the
    device of its inputs: A = (Q / sqrt(d_k)) K^T; A[:, :, 1:, 1:] += table[index[i-1, j-1], h] over the top-left
    (S-1) x (S-1) corner of a possibly wider index; P = softmax(A); O = (P * keep / (1 - p)) V, head-merged.  Returns
    (P [N, H, S, S], O [N*S, H*dv], dQ, dK, dV, dtable): the gradients for the output gradient ``do`` (all None when ``do`` is
    None; dtable None without a table).  ``keep``: the [N, H, S, S] dropout mask (``Fn.dropout_mask``), None without dropout.
    ``cut_key``: a key left out of the softmax (its logit -inf) - the bar-sensitivity check of the tests."""
    grad = do is not None
    qd, kd, vd = (t.detach().double().reshape(N, S, H, -1).transpose(1, 2).requires_grad_(grad) for t in (q, k, v))
    td = table.detach().double().requires_grad_(grad) if table is not None else None
    a = torch.matmul(qd * (1.0 / dk ** 0.5), kd.transpose(-1, -2))
    if td is not None and S > 1:
        ix = index[: S - 1, : S - 1].reshape(-1).to(td.device)
        bias = td[ix].view(S - 1, S - 1, H).permute(2, 0, 1)
        a = a + torch.nn.functional.pad(bias, (1, 0, 1, 0))
    if cut_key is not None:
        cut = torch.zeros(S, dtype=torch.bool, device=a.device)
        cut[cut_key] = True
        a = a.masked_fill(cut, float("-inf"))
    p = torch.softmax(a, -1)
    pd = p * keep.double() / (1.0 - p_drop) if p_drop > 0 else p
    o = torch.matmul(pd, vd)
    out = o.detach().transpose(1, 2).reshape(N * S, H * dv)
    if not grad:
        return p.detach(), out, None, None, None, None
    o.backward(do.detach().double().reshape(N, S, H, dv).transpose(1, 2))
    g = lambda t: t.grad.transpose(1, 2).reshape(N * S, -1)
    return p.detach(), out, g(qd), g(kd), g(vd), (td.grad if td is not None else None)


def attn_rounded_probs(q, k, N, S, H, dk, table, index):
    """f64 softmax of the logits the bf16 long forward contracts (csrc/attention_long.hip tile_xt): K and Q * scale (an f32
    product, scale the float LstcAttnDesc.scale) rounded to bf16 (RNE), products and sums in f64, the f32 bias added."""
    scale = torch.tensor(1.0 / dk ** 0.5, dtype=torch.float32, device=q.device)
    qs = (q * scale).to(torch.bfloat16).double().reshape(N, S, H, dk).transpose(1, 2)
    kr = k.to(torch.bfloat16).double().reshape(N, S, H, dk).transpose(1, 2)
    a = torch.matmul(qs, kr.transpose(-1, -2))
    if table is not None and S > 1:
        ix = index[: S - 1, : S - 1].reshape(-1).to(q.device)
        bias = table.double()[ix].view(S - 1, S - 1, H).permute(2, 0, 1)
        a = a + torch.nn.functional.pad(bias, (1, 0, 1, 0))
    return torch.softmax(a, -1)


def attn_layout(kind, ts):
    """Views holding the values of the contiguous [M, cols] tensors ``ts`` (Q, K, V, dO) in the layout ``kind``:
    "odd_ld": Q | K | V column blocks of one buffer whose row length is odd, dO in its own odd-length rows;
    "offset": every base one float past a 16-B boundary; "strides": four buffers, four different row strides;
    "fused": Q | K | V column blocks of one [M, cols(Q) + cols(K) + cols(V)] matrix (the fused projection's output: every
    base 16-B aligned when the widths are multiples of 4, row stride the sum of the three), dO contiguous."""
    dev = ts[0].device
    M = ts[0].shape[0]
    cols = [t.shape[1] for t in ts]
    if kind in ("odd_ld", "fused"):
        pad = 1 if kind == "odd_ld" else 0
        buf = torch.zeros(M, sum(cols[:3]) + pad, device=dev)
        c0 = [0, cols[0], cols[0] + cols[1]]
        views = [buf[:, c: c + n] for c, n in zip(c0, cols[:3])] + [torch.zeros(M, cols[3] + pad, device=dev)[:, : cols[3]]]
    elif kind == "offset":
        views = [torch.zeros(t.numel() + 4, device=dev)[1: 1 + t.numel()].view(t.shape) for t in ts]
    elif kind == "strides":
        views = [torch.zeros(M, n + extra, device=dev)[:, :n] for n, extra in zip(cols, (1, 2, 3, 5))]
    else:
        raise ValueError(kind)
    for dst, src in zip(views, ts):
        dst.copy_(src)
    return views


class _LibSpy:
    """Records every C entry point the Python layer calls, with the row count of each GEMM (hand it out in place of the library:
    ``monkeypatch.setattr(_lib, "load", lambda: spy)``)."""

    def __init__(self, lib):
        self._lib, self.calls, self.gemm_rows = lib, [], []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("lstc_") or name in ("lstc_strerror", "lstc_pack1_bytes", "lstc_version"):
            return fn

        def wrapped(*a):
            self.calls.append(name)
            if name == "lstc_gemm":
                self.gemm_rows.append(int(a[0]._obj.M))
            return fn(*a)
        return wrapped


_BATCH_CACHE = {}


def cached_training_batch(*args, **kw):
    """``synthetic.training_batch`` with the last three results kept: the headline-size batches (2 x 403 MB from the portable
    generator, several seconds each) are asked for by five tests in a row.  Returns copies: a test may write into its arrays."""
    from lstc_vad_amd import synthetic as syn
    key = (args, tuple(sorted(kw.items())))
    hit = _BATCH_CACHE.get(key)
    if hit is None:
        hit = syn.training_batch(*args, **kw)
        while len(_BATCH_CACHE) >= 3:
            _BATCH_CACHE.pop(next(iter(_BATCH_CACHE)))
        _BATCH_CACHE[key] = hit
    return tuple(a.copy() for a in hit)
