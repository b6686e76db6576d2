"""Scoring a pool of LONG parts with short tails two ways ("Unpadded above 128 tokens"): padded to the longest
(``ragged=True``) and unpadded on the key-tiled offset kernels (``ragged="unpadded_long"``).  A measurement tool, not on the product
path; the sibling of tools/unpadded_time.py for parts above 128 tokens.

Workload: ``--videos`` (199) videos of ``--clips`` (190 on average, 60 % .. 140 %: the SHT-shaped list of tools/resident_eval_time.py)
clips at 16 patches, d = 2048, cut into parts of ``--part_len`` clips (8 and 16: S = 129 and 257) whose last part keeps the clips
that are left (a short tail), the LTN-SHT encoder of bench.py with a relative index over part_len clips, eval(), exact f32.  The
arms run interleaved, ``--repeats`` (5) rounds after ``--warmup`` (1) rounds, both in batches of up to ``--max_batch`` (4096, the
scorers' default) parts; each time is a host clock around the call and a device synchronise.  Reported per arm: median, min, max
(the spread) in ms.
Run on an MI355X:  python tools/unpadded_long_time.py [--out profiles/unpadded_long.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstc_vad_amd import scoring                                     # noqa: E402
from lstc_vad_amd.models import Classifier, Encoder                  # noqa: E402

P, D = 16, 2048


def pool(bank, counts, part_len):
    """The parts of every video as views of the bank [clips, P, D]: part_len clips each, the tail part what is left."""
    seqs, first = [], 0
    for n in counts:
        for c in range(0, n, part_len):
            seqs.append(bank[first + c: first + min(c + part_len, n)].reshape(-1, D))
        first += n
    return seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=199)
    ap.add_argument("--clips", type=int, default=190)
    ap.add_argument("--part_len", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--max_batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("unpadded_long_time.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(11)
    counts = [max(4, int(a.clips * (0.6 + 0.8 * rs.rand()))) for _ in range(a.videos)]
    gd = torch.Generator(device=dev).manual_seed(2)
    bank = 0.5 * torch.relu(torch.randn(sum(counts), P, D, device=dev, generator=gd))
    lines = [f"{a.videos} videos, {sum(counts)} clips, P = {P}, d = {D}, LTN-SHT encoder (3 layers, 8 heads of 256), eval(), exact f32, "
             f"batches of up to {a.max_batch} parts",
             f"medians of {a.repeats} interleaved runs after {a.warmup} warm-up round(s) (min .. max = the spread); clips/s = clips of the "
             "list / median"]
    res = {"videos": a.videos, "clips": sum(counts), "rows": []}
    for L in a.part_len:
        torch.manual_seed(0)
        enc = Encoder(n_layers=3, n_head=8, d_k=256, d_v=256, d_model=D, d_inner=4096, MHA_layerNorm=True, FFN_layerNorm=True,
                      relative_pe=True, window_size=4, window_depth=L, weight_init=False).to(dev).eval()
        head = Classifier(D).to(dev).eval()
        seqs = pool(bank, counts, L)
        real = sum(s.shape[0] + 1 for s in seqs)
        padded = len(seqs) * (L * P + 1)
        arms = [("padded (ragged=True)", True), ("unpadded (ragged='unpadded_long')", "unpadded_long")]
        times, scores = {name: [] for name, _ in arms}, {}
        with torch.no_grad():
            for r in range(a.warmup + a.repeats):
                for name, ragged in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = scoring.ltn_sequence_scores(enc, head, seqs, max_batch=a.max_batch, ragged=ragged)
                    torch.cuda.synchronize()
                    if r >= a.warmup:
                        times[name].append((time.perf_counter() - t0) * 1e3)
                    scores[name] = out
        diff = float((scores[arms[0][0]] - scores[arms[1][0]]).abs().max())
        tails = sum(1 for s in seqs if s.shape[0] < L * P)
        lines.append(f"part_len {L} (S = {L * P + 1}): {len(seqs)} parts, {tails} of them short tails; {real} real rows, {padded} padded "
                     f"({padded / real:.3f}x); max |padded - unpadded| {diff:.1e}")
        med = {}
        for name, _ in arms:
            t = times[name]
            med[name] = statistics.median(t)
            lines.append(f"  {name:36s} {med[name]:9.1f} ms  ({min(t):.1f} .. {max(t):.1f}) = {sum(counts) / med[name]:7.1f} k clips/s")
        ratio = med[arms[1][0]] / med[arms[0][0]]
        lines.append(f"  unpadded / padded {ratio:.3f}")
        res["rows"].append({"part_len": L, "parts": len(seqs), "tails": tails, "real_rows": real, "padded_rows": padded,
                            "median_ms": {k: round(v, 2) for k, v in med.items()}, "unpadded_over_padded": round(ratio, 3),
                            "max_abs_score_diff": diff})
        del enc, head, seqs, scores
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
