#!/usr/bin/env python3
"""Generate the cross-attention fixtures (tests/golden/mha_cross_*.npz) from the REAL reference ``MultiHeadAttention``
(models/MultiHeadAttention.py:93-132) called with three inputs over the case table of mha_cross_cases.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mha_cross.py [--out DIR] [--only a,b]

Each fixture holds q, k, v, the mask (where the case has one), the fixed weights ``w`` of the objective sum(out * w), the
module's ``out`` and ``attn`` and the gradients of the objective with respect to q, k, v and every parameter (zeros where the
reference leaves None).  Where a case passes one tensor as k and v, ``grad_k`` holds that tensor's whole gradient and ``grad_v``
is zero.  Build container only (needs /root/reference); the fixtures are data: inputs and expected outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (binds the reference on import)
from cases import fill_params  # noqa: E402
from mha_cross_cases import MHA_CROSS_CASES, build_inputs, build_mask, module_kw  # noqa: E402


def run_case(name, case):
    import torch
    mod = make_golden.RefMHA(**module_kw(case))
    make_golden.assert_reference(type(mod))
    fill_params(mod, case["seed"])
    mod.train()
    q, k, v, w = build_inputs(case)
    tq, tk = (torch.from_numpy(a).requires_grad_(True) for a in (q, k))
    tv = tk if case["shared_kv"] else torch.from_numpy(v).requires_grad_(True)
    mask = build_mask(case)
    out, attn = mod(tq, tk, tv, mask=None if mask is None else torch.from_numpy(mask), return_attn=True)
    (out * torch.from_numpy(w)).sum().backward()
    res = {"q": q, "k": k, "v": v, "w": w, "out": out.detach().numpy(), "attn": attn.detach().numpy(),
           "grad_q": tq.grad.numpy(), "grad_k": tk.grad.numpy(),
           "grad_v": np.zeros_like(v) if case["shared_kv"] else tv.grad.numpy(), "seed": np.int64(case["seed"])}
    if mask is not None:
        res["mask"] = mask
    for key, p in mod.named_parameters():
        res["grad." + key] = p.grad.numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    path = os.path.join(make_golden.OUT_DIR, name + ".npz")
    np.savez_compressed(path, **res)
    print(f"{name}: {case['Sq']} x {case['Sk']}, mask {None if mask is None else list(mask.shape)}, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    # one CPU thread: the reference's bias-table gradient (an accumulating index_put) is summed in a thread-count-dependent
    # order, and the fixtures must regenerate bit for bit
    import torch
    torch.set_num_threads(1)
    if "--out" in sys.argv:
        make_golden.OUT_DIR = sys.argv[sys.argv.index("--out") + 1]
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    for name, case in MHA_CROSS_CASES.items():
        if only is None or name in only:
            run_case(name, case)
