#!/usr/bin/env python3
"""Record tests/golden/block_calls.json and tests/golden/block_bits.json: the traces (autograd node, ordered C entry points with
the weight-gradient deliveries, dropout sites and seeds) and the SHA-256 digests (output, probabilities, input and parameter
gradients) of the encoder-block cases of tests/util_block_bits.py.

    python tools/record_block_bits.py COMMIT [OUTDIR]        (needs the GPU; COMMIT names the commit the tree stands on)

The table is run TWICE and the two runs must agree key for key - a result that differs between two runs of one build cannot be
held to a recording; the tool names the keys and writes nothing.  Run it on the commit whose behaviour is to be kept and commit the
files; tests/test_block_bits_gpu.py replays the cases on the tree under test and compares.  A change that moves kernel bits on
purpose re-records block_bits.json only (``--bits-only``)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import util_block_bits as U  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if a != "--bits-only"]
    if not args:
        sys.exit(__doc__)
    commit = args[0]
    out = args[1] if len(args) > 1 else os.path.join(ROOT, "tests", "golden")
    os.makedirs(out, exist_ok=True)
    t1, d1 = U.run_all()
    t2, d2 = U.run_all()
    moved = sorted(k for k in set(d1) | set(d2) if d1.get(k) != d2.get(k)) + sorted(k for k in set(t1) | set(t2) if t1.get(k) != t2.get(k))
    if moved:
        sys.exit(f"{len(moved)} keys differ between two runs of the same build: {moved}")
    head = {"seed": U.SEED, "commit": commit}
    files = [("block_bits.json", dict(head, digests=d1))]
    if "--bits-only" not in sys.argv:
        files.append(("block_calls.json", dict(head, traces=t1)))
    for name, body in files:
        with open(os.path.join(out, name), "w") as f:
            json.dump(body, f, indent=0, sort_keys=True)
            f.write("\n")
    print(f"{len(t1)} cases, {len(d1)} digests, two runs equal -> {out}")


if __name__ == "__main__":
    main()
