"""Scoring a pool of parts of mixed lengths three ways ("Unpadded"): grouped by length (``ragged=False``), padded to the
longest (``ragged=True``) and unpadded (``ragged="unpadded"``), plus the unpadded route with one attention launch per tile count
T = ceil(S_n / 32) instead of ONE per layer (functional._ATTN_VAR_BUCKETS).  A measurement tool, not on the product path.

Workload: ``--parts`` (4096) parts of 1, 2 and 3 clips at 16 patches, d = 2048, the LTN-SHT encoder of bench.py, eval(), exact f32.
The arms run interleaved, ``--repeats`` (9) rounds after ``--warmup`` (2) rounds; each time is a host clock around the call and a
device synchronise.  Reported per arm: median, min, max (the spread) in ms, and the largest score difference to the grouped arm.
Run on an MI355X:  python tools/unpadded_time.py [--out profiles/unpadded_scoring_ab.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lstc_vad_amd import functional as Fn                            # noqa: E402
from lstc_vad_amd import scoring                                     # noqa: E402
from lstc_vad_amd.models import Classifier, Encoder                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("unpadded_time.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    enc = Encoder(n_layers=3, n_head=8, d_k=256, d_v=256, d_model=2048, d_inner=4096, MHA_layerNorm=True, FFN_layerNorm=True,
                  relative_pe=True, window_size=4, window_depth=3, weight_init=False).to(dev).eval()
    head = Classifier(2048).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    clips = [1 + int(v) for v in torch.randint(0, 3, (a.parts,), generator=g)]
    gd = torch.Generator(device=dev).manual_seed(2)
    seqs = [0.5 * torch.relu(torch.randn(c * 16, 2048, device=dev, generator=gd)) for c in clips]
    real = sum(c * 16 + 1 for c in clips)
    padded = a.parts * (max(clips) * 16 + 1)

    def arm(ragged, buckets=False):
        def run():
            Fn._ATTN_VAR_BUCKETS = buckets
            try:
                return scoring.ltn_sequence_scores(enc, head, seqs, ragged=ragged)
            finally:
                Fn._ATTN_VAR_BUCKETS = False
        return run
    arms = [("grouped (ragged=False)", arm(False)), ("padded (ragged=True)", arm(True)), ("unpadded, one attention launch", arm("unpadded")),
            ("unpadded, one attention launch per tile count", arm("unpadded", True))]
    times = {name: [] for name, _ in arms}
    scores = {}
    with torch.no_grad():
        for r in range(a.warmup + a.repeats):
            for name, fn in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) * 1e3
                if r >= a.warmup:
                    times[name].append(dt)
                scores[name] = out
    base = scores[arms[0][0]]
    res = {"workload": f"{a.parts} parts of 1-3 clips at P = 16 ({real} real rows, {padded} padded: {padded / real:.2f}x), d = 2048, "
                       "LTN-SHT encoder, eval(), exact f32", "repeats": a.repeats, "arms": {}}
    for name, _ in arms:
        t = times[name]
        res["arms"][name] = {"median_ms": round(statistics.median(t), 2), "min_ms": round(min(t), 2), "max_ms": round(max(t), 2),
                             "max_abs_score_diff_vs_grouped": float((scores[name] - base).abs().max())}
    med = {name: res["arms"][name]["median_ms"] for name, _ in arms}
    res["unpadded_over_padded"] = round(med[arms[2][0]] / med[arms[1][0]], 3)
    res["unpadded_over_grouped"] = round(med[arms[2][0]] / med[arms[0][0]], 3)
    res["bucketed_over_single_launch"] = round(med[arms[3][0]] / med[arms[2][0]], 3)
    lines = [res["workload"], f"medians of {a.repeats} interleaved runs after {a.warmup} warm-up rounds (min .. max = the spread):"]
    for name, _ in arms:
        r = res["arms"][name]
        lines.append(f"  {name:48s} {r['median_ms']:9.2f} ms  ({r['min_ms']:.2f} .. {r['max_ms']:.2f})   max |score - grouped| {r['max_abs_score_diff_vs_grouped']:.2e}")
    lines.append(f"unpadded / padded {res['unpadded_over_padded']}, unpadded / grouped {res['unpadded_over_grouped']}, "
                 f"bucketed attention launches / single launch {res['bucketed_over_single_launch']}")
    text = "\n".join(lines)
    print(text)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
