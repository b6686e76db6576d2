#!/usr/bin/env python3
"""Record tests/golden/ln_bwd_bits.json: SHA-256 digests of the raw output bytes of lstc_layernorm_bwd,
lstc_layernorm_bwd_drop_pack and lstc_layernorm_bwd_drop, and the return codes of the calls they refuse, on the calls of
tests/util_ln_bwd_bits.py.

    python tools/record_ln_bwd_bits.py [OUT.json]        (needs the GPU; LSTC_LIBRARY names another build's liblstc_hip.so)

Run it on the commit whose bits are to be kept - the parent of a change that must not move them - and commit the file;
tests/test_ln_bwd_bits_gpu.py replays the same calls on the tree under test and compares."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import util_ln_bwd_bits as U  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ln_bwd_bits.json")
    digests = U.all_digests()
    with open(out, "w") as f:
        json.dump({"seed": U.SEED, "fill": U.FILL, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {out}")


if __name__ == "__main__":
    main()
