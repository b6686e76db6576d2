"""Helpers of the attention-mask tests (tests/test_attn_mask_gpu.py, tests/test_attn_mask_host.py): the float64 restatement
of the masked attention contract (include/lstc_hip.h, "Attention masks"), the mask recipes, the input recipe of
tests/test_attention_sweep_gpu.py and the fixture loader."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("P", "O", "dQ", "dK", "dV", "dtable")
MASK_KINDS = ("lengths", "rows", "full", "causal")


def attn_reference_masked(q, k, v, do, N, S, H, dk, dv, table, index, keep, p_drop, mask, fill_after_bias=False):
    """tests/util.py ``attn_reference`` with one extra step between the logits and the bias: where ``mask`` (anything that
    broadcasts against [N, H, S, S]; zero = masked; None = no mask) is 0 the logit becomes ``bias - bias.detach() - 1e9`` -
    the value -1e9 (the f32 sum -1e9f + bias rounds back to -1e9f for |bias| < 32) and the derivative 1 with respect to the
    bias, which is added after the fill - and ``a + bias`` elsewhere.  Autograd then gives the rest: masked keys of a row that
    keeps a key have probability 0, a fully masked row is uniform, no gradient reaches q.k at a masked position, and the
    table gradient still receives dA there.  ``fill_after_bias``: the other restatement, "mask everything the same way" (the
    constant -1e9 in place of logit AND bias: no gradient to the table either) - what the fully-masked-row test must tell apart.
    Returns (P, O, dQ, dK, dV, dtable) as ``attn_reference``."""
    grad = do is not None
    qd, kd, vd = (t.detach().double().reshape(N, S, H, -1).transpose(1, 2).requires_grad_(grad) for t in (q, k, v))
    td = table.detach().double().requires_grad_(grad) if table is not None else None
    a = torch.matmul(qd * (1.0 / dk ** 0.5), kd.transpose(-1, -2))
    bias = torch.zeros(H, S, S, dtype=torch.float64, device=a.device)
    if td is not None and S > 1:
        ix = index[: S - 1, : S - 1].reshape(-1).to(td.device)
        bias = torch.nn.functional.pad(td[ix].view(S - 1, S - 1, H).permute(2, 0, 1), (1, 0, 1, 0))
    if mask is None:
        a = a + bias
    else:
        kept = (mask.to(a.device) != 0).expand(N, H, S, S)
        filled = torch.full_like(a, -1e9) if fill_after_bias else (bias - bias.detach() - 1e9).expand(N, H, S, S)
        a = torch.where(kept, a + bias, filled)
    p = torch.softmax(a, -1)
    pd = p * keep.double() / (1.0 - p_drop) if p_drop > 0 else p
    o = torch.matmul(pd, vd)
    out = o.detach().transpose(1, 2).reshape(N * S, H * dv)
    if not grad:
        return p.detach(), out, None, None, None, None
    o.backward(do.detach().double().reshape(N, S, H, dv).transpose(1, 2))
    g = lambda t: t.grad.transpose(1, 2).reshape(N * S, -1)
    return p.detach(), out, g(qd), g(kd), g(vd), (td.grad if td is not None else None)


def model_index(S, device):
    """The models' index for S tokens at 16 patches and its table row count (tests/test_attention_sweep_gpu.py)."""
    from lstc_vad_amd.models.MultiHeadAttention import relative_position_index_3d
    L = max(1, -(-(S - 1) // 16))
    return relative_position_index_3d(L, 4).to(device), (2 * L - 1) * 49


def sweep_inputs(N, S, H, dk, dv, seed, device):
    """q, k [N*S, H*dk], v, dO [N*S, H*dv] ~ randn, a 0.4 * randn table over the models' index."""
    g = torch.Generator(device=device).manual_seed(seed)
    q, k = (torch.randn(N * S, H * dk, device=device, generator=g) for _ in range(2))
    v, do = (torch.randn(N * S, H * dv, device=device, generator=g) for _ in range(2))
    index, rows = model_index(S, device)
    table = 0.4 * torch.randn(rows, H, device=device, generator=g)
    return q, k, v, do, table, index


def key_lengths(N, S):
    """A different kept length per sequence, from S (sequence 0: nothing masked) down to about S / 3."""
    return [max(1, S - (n * 2 * S) // (3 * max(1, N - 1))) if n else S for n in range(N)]


def make_mask(kind, N, H, S, seed, device="cpu"):
    """bool masks (True = kept) of the four kinds the kernels are tested with, and what the tests need to know about them:
      "lengths": [N, 1, 1, S] key padding, ``key_lengths(N, S)``;
      "rows":    [N, 1, S, S] about 30 % masked at random, query row S // 2 of the last sequence fully masked and, where S > 32,
                 the aligned 32-key block 0..31 of query row 1 of sequence 0 masked (that row keeps key S - 1);
      "full":    [N, H, S, S] about 30 % masked at random, a different pattern per head;
      "causal":  [1, 1, S, S] lower triangle.
    Returns (mask, info) with info["dead_row"] = (n, i) or None."""
    g = torch.Generator().manual_seed(seed)
    info = {"dead_row": None}
    if kind == "lengths":
        m = torch.arange(S)[None, :] < torch.tensor(key_lengths(N, S))[:, None]
        m = m.view(N, 1, 1, S)
    elif kind == "rows":
        m = torch.rand(N, 1, S, S, generator=g) >= 0.3
        m[N - 1, 0, S // 2, :] = False
        info["dead_row"] = (N - 1, S // 2)
        if S > 32:
            m[0, 0, 1, :32] = False
            m[0, 0, 1, S - 1] = True
    elif kind == "full":
        m = torch.rand(N, H, S, S, generator=g) >= 0.3
    elif kind == "causal":
        m = torch.ones(S, S, dtype=torch.bool).tril().view(1, 1, S, S)
    else:
        raise ValueError(kind)
    return m.to(device), info


def bar(name, ref):
    """The project's bars against f64: P within 2e-6; everything else within 2e-5 * max|ref| + 1e-6."""
    return 2e-6 if name == "P" else 2e-5 * float(ref.abs().max()) + 1e-6


def load_mask_case(name):
    """(npz, case dict) of a committed attention-mask fixture (tests/golden/mask_cases.py)."""
    from mask_cases import MASK_CASES
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False), MASK_CASES[name]
