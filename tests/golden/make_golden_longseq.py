#!/usr/bin/env python3
"""Generate the long-sequence golden fixtures (tests/golden/ltn_*_long*.npz) from the REAL reference, with the recipe of
make_golden.py (its ``run_case`` / ``run_full_case``, imported, unchanged) over the case table of longseq_cases.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_longseq.py [--out DIR] [--only a,b]

Build container only (needs /root/reference); the fixtures are data: inputs and expected outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (binds the reference on import)
from longseq_cases import LONG_CASES, LONG_FULL_CASES  # noqa: E402


def trim(name):
    """Keep each reduced fixture under the 1-MiB file limit: drop what tests/test_longseq_gpu.py does not read - the eval-mode
    passes, the head's weights after two steps, and five of the six identical copies of the [256, 256] relative-position index
    (the models rebuild it; layer 0's initial copy stays as the check that they build the reference's)."""
    path = os.path.join(make_golden.OUT_DIR, name + ".npz")
    z = np.load(path, allow_pickle=False)
    keep = {k: z[k] for k in z.files
            if not k.startswith(("eval_", "head_after2."))
            and not (k.endswith(".relative_position_index") and k != "enc_init.layer_stack.0.slf_attn.relative_position_index")}
    z.close()
    np.savez_compressed(path, **keep)
    print(f"{name}: trimmed to {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    # one CPU thread throughout: at S = 145 - 257 the reference's bias-table gradient (an accumulating index_put over S^2
    # entries) is summed in a thread-count-dependent order, and the fixtures must regenerate bit for bit
    import torch
    torch.set_num_threads(1)
    torch.set_num_threads = lambda n: None          # run_full_case asks for 8 threads: keep the one
    if "--out" in sys.argv:
        make_golden.OUT_DIR = sys.argv[sys.argv.index("--out") + 1]
    only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
    for i, (name, (mode, ekw, skw)) in enumerate(LONG_CASES.items()):
        if only is None or name in only:
            make_golden.run_case(name, mode, ekw, skw, seed=61 + i)
            trim(name)
    for name, (mode, ekw, skw, seed) in LONG_FULL_CASES.items():
        if only is None or name in only:
            make_golden.run_full_case(name, mode, ekw, skw, seed)
