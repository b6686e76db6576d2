#!/usr/bin/env python3
"""Record tests/golden/cls_concat_bits.json: SHA-256 digests of the raw output bytes of the eight CLS-concat entry points and of
lstc_cls_dot{,_len,_var} / lstc_cls_wsum{,_var} / lstc_cls_outer{,_var}, on the calls of tests/util_cls_layouts.py.

    python tools/record_cls_concat_bits.py [OUT.json]        (needs the GPU; LSTC_LIBRARY names another build's liblstc_hip.so)

Run it on the commit whose bits are to be kept - the parent of a change that must not move them - and commit the file;
tests/test_cls_layouts_gpu.py replays the same calls on the tree under test and compares the digests."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import util_cls_layouts as U  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "cls_concat_bits.json")
    digests = U.all_digests()
    with open(out, "w") as f:
        json.dump({"seed": U.SEED, "fill": U.FILL, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(digests)} digests -> {out}")


if __name__ == "__main__":
    main()
