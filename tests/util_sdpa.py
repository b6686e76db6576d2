"""Helpers of the rectangular-attention tests (tests/test_sdpa_gpu.py, tests/test_sdpa_host.py): the float64 restatement of the
``lstc_sdpa_*`` contract (include/lstc_hip.h, "Rectangular attention"), input and mask recipes and the fixture loader.  The bars
are the project's (``util_mask.bar``)."""
import os

import numpy as np
import torch

from util_mask import GOLDEN, bar, key_lengths  # noqa: F401  (re-exported)

NAMES = ("P", "O", "dQ", "dK", "dV")
MASK_KINDS = ("lengths", "rows", "full")


def sdpa_reference(q, k, v, do, scale, keep=None, p_drop=0.0, mask=None):
    """float64: A = (q scale) k^T; A = -1e9 where ``mask`` (anything that broadcasts against [N, H, Sq, Sk]; zero = masked) is 0;
    P = softmax(A); Pd = P keep / (1 - p); O = Pd v, and autograd for the rest - masked keys of a row that keeps a key have
    probability 0, a fully masked row is uniform, and no gradient reaches q.k at a masked position (``where`` passes none).
    q [N, H, Sq, dk], k [N, H, Sk, dk], v [N, H, Sk, dv], do [N, H, Sq, dv] or None.  Returns (P, O, dQ, dK, dV)."""
    grad = do is not None
    qd, kd, vd = (t.detach().double().requires_grad_(grad) for t in (q, k, v))
    a = torch.matmul(qd * float(scale), kd.transpose(-1, -2))
    if mask is not None:
        a = torch.where((mask.to(a.device) != 0).expand(a.shape), a, torch.full_like(a, -1e9))
    p = torch.softmax(a, -1)
    pd = p * keep.double() / (1.0 - p_drop) if p_drop > 0 else p
    o = torch.matmul(pd, vd)
    if not grad:
        return p.detach(), o.detach(), None, None, None
    o.backward(do.detach().double())
    return p.detach(), o.detach(), qd.grad, kd.grad, vd.grad


def sdpa_inputs(N, H, Sq, Sk, dk, dv, seed, device):
    """q [N, H, Sq, dk], k [N, H, Sk, dk], v [N, H, Sk, dv], dO [N, H, Sq, dv] ~ randn (the sweep tests' recipe)."""
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.randn(N, H, Sq, dk, device=device, generator=g)
    k = torch.randn(N, H, Sk, dk, device=device, generator=g)
    v = torch.randn(N, H, Sk, dv, device=device, generator=g)
    do = torch.randn(N, H, Sq, dv, device=device, generator=g)
    return q, k, v, do


def make_mask_x(kind, N, H, Sq, Sk, seed, device="cpu"):
    """bool masks (True = kept) over [N, H, Sq, Sk]:
      "lengths": [N, 1, 1, Sk] key padding, ``key_lengths(N, Sk)`` (sequence 0 keeps every key);
      "rows":    [N, 1, Sq, Sk] about 30 % masked at random, query row Sq // 2 of the last sequence fully masked;
      "full":    [N, H, Sq, Sk] about 30 % masked at random, a different pattern per head.
    Returns (mask, dead_row) with dead_row = (n, i) or None."""
    g = torch.Generator().manual_seed(seed)
    dead = None
    if kind == "lengths":
        m = (torch.arange(Sk)[None, :] < torch.tensor(key_lengths(N, Sk))[:, None]).view(N, 1, 1, Sk)
    elif kind == "rows":
        m = torch.rand(N, 1, Sq, Sk, generator=g) >= 0.3
        m[N - 1, 0, Sq // 2, :] = False
        dead = (N - 1, Sq // 2)
    elif kind == "full":
        m = torch.rand(N, H, Sq, Sk, generator=g) >= 0.3
    else:
        raise ValueError(kind)
    return m.to(device), dead


def load_sdpa_case(name):
    """(npz, case dict) of a committed rectangular-attention fixture (tests/golden/sdpa_cases.py)."""
    from sdpa_cases import SDPA_CASES
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False), SDPA_CASES[name]
