#!/usr/bin/env python3
"""Generate the rectangular-attention fixtures (tests/golden/sdpa_*.npz) from the REAL reference
``ScaledDotProductAttention`` (models/MultiHeadAttention.py:9-23) in ``eval()`` over the case table of sdpa_cases.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sdpa.py [--out DIR] [--only a,b]

Each fixture holds q, k, v, the mask (where the case has one), the fixed weights ``w`` of the objective sum(output * w), the
module's ``output`` and ``attn`` and the gradients of the objective with respect to q, k and v.  Build container only (needs
/root/reference); the fixtures are data: inputs and expected outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (binds the reference on import)
from models.MultiHeadAttention import ScaledDotProductAttention as RefSDPA  # noqa: E402  (reference)
from sdpa_cases import SDPA_CASES, build_inputs, build_mask  # noqa: E402


def run_sdpa_case(name, case):
    import torch
    make_golden.assert_reference(RefSDPA)
    mod = RefSDPA(temperature=case["dk"] ** 0.5).eval()
    q, k, v, w = build_inputs(case)
    tq, tk, tv = (torch.from_numpy(a).requires_grad_(True) for a in (q, k, v))
    mask = build_mask(case)
    out, attn = mod(tq, tk, tv, mask=None if mask is None else torch.from_numpy(mask))
    (out * torch.from_numpy(w)).sum().backward()
    res = {"q": q, "k": k, "v": v, "w": w, "output": out.detach().numpy(), "attn": attn.detach().numpy(),
           "grad_q": tq.grad.numpy(), "grad_k": tk.grad.numpy(), "grad_v": tv.grad.numpy(), "seed": np.int64(case["seed"])}
    if mask is not None:
        res["mask"] = mask
    path = os.path.join(make_golden.OUT_DIR, name + ".npz")
    np.savez_compressed(path, **res)
    print(f"{name}: {case['Sq']} x {case['Sk']}, mask {None if mask is None else list(mask.shape)}, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    # one CPU thread: the fixtures must regenerate bit for bit
    import torch
    torch.set_num_threads(1)
    if "--out" in sys.argv:
        make_golden.OUT_DIR = sys.argv[sys.argv.index("--out") + 1]
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    for name, case in SDPA_CASES.items():
        if only is None or name in only:
            run_sdpa_case(name, case)
