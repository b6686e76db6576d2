#!/usr/bin/env python3
"""Generate the attention-mask fixtures (tests/golden/mask_*.npz) from the REAL reference ``Encoder`` run with ``src_mask``
over the case table of mask_cases.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mask.py [--out DIR] [--only a,b]

Each fixture holds the input ``x`` [N, S - 1, d], the mask, the fixed weights ``w`` of the objective sum(out * w), the encoder
output, the ``return_attn`` probabilities of every layer and the gradient of the objective with respect to every parameter and
to ``x``.  Build container only (needs /root/reference); the fixtures are data: inputs and expected outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (binds the reference on import)
from cases import fill_params  # noqa: E402
from mask_cases import MASK_CASES, build_mask, encoder_kw, seq_len  # noqa: E402


def objective_weights(N, S, d, seed):
    """Fixed weights in [-1, 1] / (N S d): the objective is a mean of O(1) terms, the size of a loss."""
    return (make_golden.syn.small_uniform((N, S, d), seed, 2, 1.0) / float(N * S * d)).astype(np.float32)


def run_mask_case(name, case):
    import torch
    N, S, d, seed = case["N"], seq_len(case), encoder_kw(case)["d_model"], case["seed"]
    enc = make_golden.RefEncoder(**encoder_kw(case))
    make_golden.assert_reference(type(enc))
    fill_params(enc, seed)
    enc.train()
    x = torch.from_numpy(make_golden.syn.small_uniform((N, S - 1, d), seed, 1, 1.0)).requires_grad_(True)
    w = objective_weights(N, S, d, seed)
    mask = build_mask(case)
    out, attns = enc(x, src_mask=torch.from_numpy(mask), return_attn=True)
    (out * torch.from_numpy(w)).sum().backward()
    res = {"x": x.detach().numpy(), "w": w, "mask": mask, "out": out.detach().numpy(), "grad_x": x.grad.numpy(),
           "seed": np.int64(seed)}
    for i, a in enumerate(attns):
        res[f"attn.{i}"] = a.detach().numpy()
    for k, p in enc.named_parameters():
        res["grad." + k] = p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    path = os.path.join(make_golden.OUT_DIR, name + ".npz")
    np.savez_compressed(path, **res)
    print(f"{name}: S = {S}, mask {mask.dtype} {list(mask.shape)}, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    # one CPU thread: the reference's bias-table gradient (an accumulating index_put) is summed in a thread-count-dependent
    # order, and the fixtures must regenerate bit for bit
    import torch
    torch.set_num_threads(1)
    if "--out" in sys.argv:
        make_golden.OUT_DIR = sys.argv[sys.argv.index("--out") + 1]
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    for name, case in MASK_CASES.items():
        if only is None or name in only:
            run_mask_case(name, case)
