#!/usr/bin/env python3
"""Headline benchmark: snippets/sec of one full LSTC_VAD training step on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config ltn_sht|stn_sht|ltn_ucf|ltn_ubnormal|mixed_ubn_sht]
                    [--scaling strong|weak] [--feed resident|static] [--dtype fp32|bf16|f32x3] [--full] [--dump-outputs DIR]

Workload (BASELINE.json configs[1], the configuration the metric is quoted on): LTN temporal transformer, part_len=3,
n_head=8, d_k=d_v=256, relative position bias (window 4), d_model=2048, n_hidden=4096, 3 layers, MHA + FFN LayerNorm,
fp32; GLOBAL batch B=64 videos (--batch_size 32 normal/abnormal pairs), T=32 parts, P=16 patches; reference dropout rates
(0.2/0.2/0.1/0.6); synthetic I3D-like features resident in HBM.

A step = batch formation (the reference's window sampler on the host + lstc_gather_rows out of the HBM-resident feature
bank) + sequence reshape + Encoder + Classifier + MIL/CE loss + backward + [gradient all-reduce] + Adagrad.

Multi-GPU: one process per GPU over RCCL.  ``python bench.py --gpus N`` starts the N ranks itself (fresh child processes,
created before this process touches the GPU); it also runs unchanged under ``python -m torch.distributed.run
--nproc-per-node N bench.py --gpus N`` (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment).
``--scaling strong`` (default, the split the metric is quoted on): the global batch stays 32 pairs, rank r
owns pairs [r*32/N, (r+1)*32/N).  ``--scaling weak``: every rank gets its own 32 pairs.

A plain run sets up, warms up, times the K steps and prints ONE JSON line (rank 0): `metric`, `value`, `unit`,
`higher_is_better`, `dtype`, `ms_per_step` and the rest of the headline pass, with `roofline` where its events ride inside
the timed steps (fp32: dominant kernel = the exact-f32 MFMA GEMM; achieved = the launches' algorithmic 2MNK FLOPs / their
HIP-event durations, measured live on the launch stream).

``--full`` adds everything beyond the headline pass: `roofline` of the 16-bit modes (3 further event steps),
`cpu_baseline` (the oracle = CPU restatement of the reference, timed on the host cores on a bounded sample), `pcie_inclusive`
and, at N=1, the sub-objects `static_batch` (same step on one fixed batch: no batch formation), `stn_headline` (STN, the
literal [64,32,16,2048] input), `bf16` and `f32x3` (other GEMM compute modes; never `value`) and `coteach_loop`.

``--dump-outputs DIR`` writes, right after the timed steps, what the last timed step computed as float32 ``DIR/<name>.npy``
(rank 0): ``scalars`` (the five scalars ``TrainStep.step`` returns: loss, MIL, err, l1, aux) and, per model, a fixed seeded
sample of every parameter's gradient (``grad.<param>``) and of the updated weights (``weight.<param>``), at most 64 MB in all.
The inputs (synthetic bank, batch sampler, weights, dropout seeds) depend on the arguments only, so two builds can be
compared output for output.
"""
import argparse
import json
import os
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (mode, encoder kwargs, step kwargs, dropout (attn, fc, ffn, head), clip-count range of the synthetic videos)
    "ltn_sht": ("LTN", dict(d_model=2048, d_inner=4096, MHA_layerNorm=True, FFN_layerNorm=True, relative_pe=True,
                            window_size=4, window_depth=3), dict(part_len=3, n_patch=16), (0.2, 0.2, 0.1, 0.6), (24, 160)),
    "stn_sht": ("STN", dict(d_model=2048, d_inner=3027, FFN_layerNorm=True), dict(part_len=1, n_patch=16),
                (0.1, 0.1, 0.1, 0.6), (24, 160)),
    "ltn_ucf": ("LTN", dict(d_model=2048, d_inner=4096, MHA_layerNorm=True, FFN_layerNorm=True, relative_pe=True,
                            window_size=4, window_depth=2), dict(part_len=2, n_patch=9), (0.2, 0.2, 0.1, 0.6), (64, 4000)),
    "ltn_ubnormal": ("LTN", dict(d_model=1024, d_inner=4096, MHA_layerNorm=True, FFN_layerNorm=True, relative_pe=True,
                                 window_size=4, window_depth=5), dict(part_len=5, n_patch=16), (0.2, 0.2, 0.1, 0.6), (24, 160)),
}
FP32_MFMA_PEAK_TFLOPS = 157.3        # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
BF16_MFMA_PEAK_TFLOPS = 2500.0       # dense bf16 MFMA


def train_flops_per_sequence(S, d, Hd, F, n_layers, c):
    """F_fwd = L*[8 S d Hd + 4 S^2 Hd + 4 S d F] + head; F_alg = 3 F_fwd - 6 S d Hd."""
    f_fwd = n_layers * (8 * S * d * Hd + 4 * S * S * Hd + 4 * S * d * F) + 2 * (512 * d + 512 * 32 + 32 * c)
    return 3 * f_fwd - 6 * S * d * Hd


def cpu_baseline(cfg_name, threads):
    """Time the oracle's full training step (forward, loss, backward, Adagrad) on the host cores on a bounded
    sample of the same workload: same model width, 2+2 videos x 8 parts (32 sequences)."""
    import torch
    from oracle import lstc_oracle as orc
    mode, ekw, skw, drops, _ = CONFIGS[cfg_name]
    torch.set_num_threads(threads)
    bs, pn, L, P, d = 2, 8, skw["part_len"], skw["n_patch"], ekw["d_model"]
    ecfg = orc.EncoderCfg(n_layers=3, n_head=8, d_k=256, d_v=256, MHA_attn_dropout=drops[0], MHA_fc_dropout=drops[1],
                          FFN_dropout=drops[2], **ekw)
    st = orc.StepCfg(mode=mode, batch_size=bs, part_num=pn, part_len=L, n_patch=P, head_dropout=drops[3])
    g = torch.Generator().manual_seed(0)
    enc_P = {k: torch.randn(s, generator=g) * 0.02 for k, s in orc.encoder_param_shapes(ecfg).items()}
    for k in enc_P:
        if k.endswith("layer_norm.weight"):
            enc_P[k] = torch.ones_like(enc_P[k])
    if ekw.get("relative_pe"):
        for i in range(3):
            enc_P[f"layer_stack.{i}.slf_attn.relative_position_index"] = orc.relative_position_index_3d(L, 4)
    kind = "classifier" if mode == "LTN" else "regressor"
    head_P = {k: torch.randn(s, generator=g) * 0.02 for k, s in orc.head_param_shapes(d, kind).items()}
    enc_S = {k: torch.zeros_like(v) for k, v in enc_P.items() if v.is_floating_point()}
    head_S = {k: torch.zeros_like(v) for k, v in head_P.items()}
    nf = 0.5 * torch.relu(torch.randn(bs, pn * L, P, d, generator=g))
    af = 0.5 * torch.relu(torch.randn(bs, pn * L, P, d, generator=g))
    al = torch.rand(bs, pn * L, 1, generator=g)
    snippets = 2 * bs * pn * L
    # one untimed warm-up step (allocator, thread pool), then the MEDIAN of up to 5 timed steps at a pinned thread count: the best-of-2
    # of rounds 1-5 read 72.6 - 102.3 snippets/s over the boxes of the pool (VERDICT r5 upkeep); bounded to ~25 s of CPU work
    times = []
    for it in range(6):
        t0 = time.perf_counter()
        _, enc_P, head_P, enc_S, head_S, _, _ = orc.train_step(enc_P, head_P, enc_S, head_S, ecfg, st, nf, af, al)
        times.append(time.perf_counter() - t0)
        if it >= 3 and sum(times) > 25:
            break
    timed = sorted(times[1:]) if len(times) > 1 else times
    t = timed[len(timed) // 2] if len(timed) % 2 else 0.5 * (timed[len(timed) // 2 - 1] + timed[len(timed) // 2])
    return {"value": round(snippets / t, 2), "unit": "snippets/s", "cores": threads, "kind": "port",
            "sample": f"oracle train_step (fwd+loss+bwd+Adagrad), same model, {2 * bs} videos x {pn} parts x "
                      f"{L} snippets = {snippets} snippets/step, median of {len(timed)} timed steps after 1 warm-up "
                      f"(torch.set_num_threads({threads})), {t:.2f} s/step, min {timed[0]:.2f} max {timed[-1]:.2f}"}


DUMP_BUDGET_BYTES = 60 * 10**6       # --dump-outputs stays under 64 MB in all


def dump_outputs(out_dir, scalars, models, per_tensor=65536):
    """--dump-outputs: what the last timed step computed, as float32 ``out_dir/<name>.npy``.  ``scalars``: the step's returned
    scalar tensor(s); ``models``: [(prefix, TrainStep)].  Per parameter the same seeded index sample (seed = crc32 of the name,
    sorted, without replacement; whole tensor when smaller) of its last gradient and of its weight after the optimizer step."""
    import zlib
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"scalars": torch.stack([s.detach().float().reshape(-1) for s in scalars]).squeeze(0).cpu().numpy()}
    named = []
    for pre, ts in models:
        for tag, mod in (("enc.", ts.encoder), ("head.", ts.head)):
            named += [(pre + tag + n, p) for n, p in mod.named_parameters() if p.is_floating_point()]
    per_tensor = max(1, min(per_tensor, DUMP_BUDGET_BYTES // (4 * 2 * max(1, len(named)))))
    with torch.no_grad():
        for name, p in named:
            n = p.numel()
            if n > per_tensor:
                idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(n, per_tensor, replace=False))
                pick = lambda t: t.detach().reshape(-1)[torch.from_numpy(idx).to(t.device)]
            else:
                pick = lambda t: t.detach().reshape(-1)
            arrays["weight." + name] = pick(p).float().cpu().numpy()
            if p.grad is not None:
                arrays["grad." + name] = pick(p.grad).float().cpu().numpy()
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_BUDGET_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the budget of {DUMP_BUDGET_BYTES}")
    for name, v in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(v, dtype=np.float32))
    return {"dir": out_dir, "files": len(arrays), "MB": round(total / 1e6, 2)}


# ---------------------------------------------------------------------------------------------- N-rank launcher
def launch_ranks(n, argv, script=None, rank_timeout_s=600.0):
    """``python bench.py --gpus N`` without a launcher: lstc_vad_amd.launch.launch_ranks (N fresh rank processes started before this
    process touches the GPU, rank 0's JSON line relayed, watchdog, stderr tails) - the same launcher ``Train/*.py --data_parallel
    --gpu 0,1,...`` uses.  Replaces the reference's single-process ``nn.DataParallel`` wrap
    (Train/temporal_transformer_shanghaitech.py:76-78) with one process per GPU."""
    from lstc_vad_amd.launch import launch_ranks as _launch
    return _launch(n, argv, script=script or os.path.abspath(__file__), rank_timeout_s=rank_timeout_s, relay="json", tag="bench")


# ---------------------------------------------------------------------------------------------- synthetic resident feed
class SyntheticResidentPairs:
    """A synthetic training set resident in HBM, served like ``lstc_vad_amd.load_dataset.ResidentPairs`` serves a real one:
    per step the host runs the reference's window sampler (``window_indices``, utils/load_dataset.py:69-88) for every pair
    of the GLOBAL batch (identical ``np.random`` consumption on every rank), and ``lstc_gather_rows`` forms this rank's
    shard ``[bs_local, pn*L, P, d]`` x2 out of the bank.  Pair order: a fresh permutation per epoch (``shuffle_keys``)."""

    def __init__(self, cfg_name, bs_global, part_num, dev, rank, world, seed, max_clips=0):
        import numpy as np
        import torch
        from lstc_vad_amd.feed import ResidentBank
        mode, ekw, skw, _, (lo, hi) = CONFIGS[cfg_name]
        if max_clips:
            hi = max(min(hi, max_clips), lo)
        self.np, self.bs, self.pn, self.L = np, bs_global, part_num, skw["part_len"]
        self.rank, self.world = rank, world
        P, d = skw["n_patch"], ekw["d_model"]
        n_vid = max(2 * bs_global, 64)                               # per class
        rs = np.random.RandomState(seed)
        self.lengths = rs.randint(max(lo, self.L + 1), hi + 1, size=(2, n_vid))
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths.reshape(-1))]).astype(np.int64)
        total = int(self.offsets[-1])
        g = torch.Generator(device=dev).manual_seed(seed)
        bank = torch.empty((total, P, d), device=dev, dtype=torch.float32)
        step = max(1, (1 << 28) // (P * d))
        for o in range(0, total, step):                              # 0.5 * relu(N(0, 1)): I3D-like post-ReLU features
            n = min(step, total - o)
            bank[o:o + n] = 0.5 * torch.relu(torch.randn(n, P, d, device=dev, generator=g))
        self.feed = ResidentBank(bank)
        self.bank_GB = total * P * d * 4 / 1e9
        u = [rs.rand(int(n), 1).astype(np.float32) for n in self.lengths[1]]
        self.pseudo = [np.where(x > 0.9, x, np.float32(0.0)) for x in u]      # rule of README.md:27
        self.rng_state = np.random.RandomState(seed + 1).get_state()          # sampler stream (np.random global, saved/restored)
        self.n_vid, self.pos = n_vid, 0
        self.order = None
        self.lazy = os.environ.get("LSTC_EAGER_GATHER", "0") != "1"      # clip indices to the step (gather fused into the CLS concat)
        self._shuffle()

    def _with_rng(self, fn):
        np = self.np
        keep = np.random.get_state()
        np.random.set_state(self.rng_state)
        try:
            return fn()
        finally:
            self.rng_state = np.random.get_state()
            np.random.set_state(keep)

    def _shuffle(self):
        np = self.np
        self.order = self._with_rng(lambda: (np.random.permutation(self.n_vid), np.random.permutation(self.n_vid)))
        self.pos = 0

    def next_batch(self):
        from lstc_vad_amd.load_dataset import window_indices
        np = self.np
        if self.pos + self.bs > self.n_vid:
            self._shuffle()
        bl = self.bs // self.world
        lo = self.rank * bl
        rows = self.pn * self.L
        idx = np.empty((2, bl, rows), np.int64)
        labs = np.zeros((bl, rows, 1), np.float32)

        def draw():
            for j in range(self.bs):
                for kind in (0, 1):
                    vid = int(self.order[kind][self.pos + j])
                    w = window_indices(int(self.lengths[kind, vid]), self.pn, self.L, "uniform")
                    if lo <= j < lo + bl:
                        idx[kind, j - lo] = w + self.offsets[kind * self.n_vid + vid]
                        if kind == 1:
                            labs[j - lo] = self.pseudo[vid][w]
        self._with_rng(draw)
        self.pos += self.bs
        out, labs_d = self.feed.gather(idx, labs, lazy=self.lazy)
        return out[0], out[1], labs_d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="ltn_sht", choices=list(CONFIGS) + ["mixed_ubn_sht"],
                    help="mixed_ubn_sht = BASELINE config 5: half the videos UBnormal (d=1024, L=5), half SHT (d=2048, L=3), two "
                         "model pairs stepped in one iteration (lstc_vad_amd.engine.MixedStep)")
    ap.add_argument("--batch_size", type=int, default=32, help="normal/abnormal pairs of the GLOBAL batch under --scaling strong "
                    "(B = 2*batch_size videos), per GPU under --scaling weak")
    ap.add_argument("--part_num", type=int, default=32)
    ap.add_argument("--max_clips", type=int, default=0, help="cap the synthetic videos' clip counts (0 = the config's range; the UCF "
                    "config draws up to 4000 clips per video = a 19-GB bank, which the shared-device functional checks - N ranks on ONE "
                    "GPU, one bank each - cut down)")
    ap.add_argument("--scaling", default="strong", choices=["strong", "weak"])
    ap.add_argument("--feed", default="resident", choices=["resident", "static"],
                    help="resident (default): every step forms a fresh batch (host window sampler + lstc_gather_rows from the "
                         "HBM-resident bank) inside the timed region; static: one fixed batch")
    ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16", "f32x3"],
                    help="GEMM compute type of `value`: fp32 = exact-f32 MFMA (headline, parity mode); bf16 = bf16 MFMA, f32 "
                         "storage/accumulate (BASELINE configs 3/5); f32x3 = f32-accurate products on the f16 matrix cores")
    ap.add_argument("--act_dtype", default="bf16", choices=["bf16", "fp32"],
                    help="bf16 compute mode only: storage of the residual stream between encoder blocks - bf16 (default: every activation "
                         "and residual-stream gradient between the CLS concat and the last full layer exists only as a packed bf16 "
                         "operand, DESIGN 3.1d) or fp32 (rounds 1-4: f32 activations between the blocks)")
    ap.add_argument("--lr_scale", type=float, default=1e-3, help="multiplies the reference learning rates (1e-4 / 1e-2): with "
                    "i.i.d. synthetic features the classifier saturates within two Adagrad steps at the reference rates and the "
                    "backward then runs on near-zero operands; timing does not depend on it")
    ap.add_argument("--h2d", action="store_true", help="(default at N=1 under --full) also time the step with the batch arriving from "
                    "host memory every step through lstc_vad_amd.feed.PinnedFeeder (reported as pcie_inclusive, never as value)")
    ap.add_argument("--no-h2d", action="store_true", help="skip the pcie_inclusive pass of --full")
    ap.add_argument("--rank_timeout_s", type=float, default=600.0, help="--gpus N launcher watchdog: stop every rank and fail when "
                    "one is still running after this many seconds (0 = no watchdog)")
    ap.add_argument("--naive-last-layer", action="store_true", help="evaluate the last encoder layer for every token like the "
                    "reference (A/B only: the default skips rows/projections nobody reads, with identical results)")
    ap.add_argument("--fuse_qkv", default="auto", choices=["auto", "on", "off"], help="Q/K/V projections as one GEMM per layer (auto: when "
                    "the rank's token count leaves the three separate products with badly filled tile rounds, engine.TrainStep)")
    ap.add_argument("--grad_reduce_dtype", default="fp32", choices=["fp32", "bf16"], help="wire format of the gradient all-reduce "
                    "(bf16: buckets rounded by lstc_cast_f32_bf16, half the xGMI bytes; default fp32 = the reference's numerics)")
    ap.add_argument("--buckets", type=int, default=0, help="gradient all-reduce buckets per model (0 = default: head + the FFN half and "
                    "the attention half of every encoder layer, backward order - 7 buckets of <= 67 MB for the LTN; N = the same pieces "
                    "merged into N groups of about equal bytes; 1 = one all-reduce after the backward)")
    ap.add_argument("--nccl_algo", default="", help="sets NCCL_ALGO for RCCL (e.g. Ring, Tree) before the communicator is created; recorded in config")
    ap.add_argument("--nccl_proto", default="", help="sets NCCL_PROTO for RCCL (e.g. Simple, LL, LL128); recorded in config")
    ap.add_argument("--graph", action="store_true", help="run the step as ONE captured HIP graph (lstc_vad_amd.engine.GraphedStep; N=1 "
                    "only): removes the ~340-launch train that small per-rank batches cannot hide")
    ap.add_argument("--no-dropout", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-gemm-events", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the N=1 sub-objects (static_batch, stn_headline, bf16, f32x3, coteach_loop)")
    ap.add_argument("--no-coteach", action="store_true", help="skip the coteach_loop sub-object (BASELINE config 3: one timed round of the "
                    "co-teaching loop through the Train/ and Test/ entry points, tools/coteach_round.py)")
    ap.add_argument("--full", action="store_true", help="besides the headline pass, run what the line reports beyond it: cpu_baseline, "
                    "pcie_inclusive, the 16-bit modes' roofline event steps and, at N=1, static_batch, stn_headline, bf16, f32x3, "
                    "coteach_loop (the --no-* options above still skip single parts)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed as "
                    "float32 DIR/<name>.npy (rank 0): the step's five scalars and seeded samples of every gradient and updated weight")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.nccl_algo:
        os.environ["NCCL_ALGO"] = a.nccl_algo            # inherited by the rank processes launch_ranks starts
    if a.nccl_proto:
        os.environ["NCCL_PROTO"] = a.nccl_proto

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a.gpus, sys.argv[1:], rank_timeout_s=a.rank_timeout_s))   # before anything initialises the GPU here

    # The JSON line must be the only thing on stdout: RCCL prints a version banner through C stdio when a communicator is
    # created (flushed at exit, i.e. AFTER our line).  Keep the real stdout aside and point fd 1 at stderr for everything else.
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the LSTC_VAD hot path here is HIP-only (no CPU fallback)")
    share = os.environ.get("LSTC_SHARE_DEVICE") == "1"              # one-GPU test boxes: every rank on device 0 (a functional check
    if share:                                                       # of the N-rank path, never a measurement; RCCL refuses it: gloo)
        local_rank = 0
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f"rank {rank}: --gpus {world} but only {torch.cuda.device_count()} device(s) visible")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    force_dist = os.environ.get("LSTC_FORCE_DIST", "0") == "1"      # exercise the RCCL code path on a single GPU
    if world > 1 or force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if share:
            dist.init_process_group(os.environ.get("LSTC_DIST_BACKEND", "gloo"), rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)
        from lstc_vad_amd.launch import mark_rank_ready
        mark_rank_ready()
    if a.gpus != world and rank == 0:
        print(f"[bench] note: --gpus {a.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)
    strong = a.scaling == "strong"
    bs_global = a.batch_size if strong else a.batch_size * world
    if bs_global % world:
        raise SystemExit(f"--batch_size {a.batch_size} pairs cannot be split over {world} ranks (SURVEY.md 8e: rank r owns pairs "
                         f"[r*bs/N, (r+1)*bs/N))")
    bs_local = bs_global // world

    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.engine import MixedStep, TrainStep
    from lstc_vad_amd.models import Classifier, Encoder, Regressor
    Fn.set_act_dtype(a.act_dtype)
    if os.environ.get("LSTC_POISON_EMPTY") == "1":
        # diagnostic (tools/uninit_probe.sh): every torch.empty() - the step's workspaces, partial sums, packs - comes back filled with
        # NaN / 0xFF instead of whatever the allocator's block held: a kernel that reads an element nobody wrote shows up as a NaN loss
        torch.use_deterministic_algorithms(True, warn_only=True)
        torch.utils.deterministic.fill_uninitialized_memory = True

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce_report(t, op=None):
        """All-reduce of a few REPORTING scalars (timings, the loss of the timed steps).  Over RCCL: on the device.  Over gloo (the
        shared-device functional checks: N processes on one GPU) the tensor goes through the host explicitly - twice in 26 such runs
        the 2 x 5 loss vector came back ~0.5 % off while twelve identical runs and every model state agreed: gloo's own
        staging of device tensors is kept out of what the line reports."""
        op = op or dist.ReduceOp.SUM
        if dist.get_backend() == "gloo":
            torch.cuda.synchronize()
            h = t.detach().cpu()
            dist.all_reduce(h, op=op)
            t.copy_(h)
        else:
            dist.all_reduce(t, op=op)
        return t

    def make(cfg_name, bs_l, bs_g, seed_off=0, feed=None):
        """Fresh model + optimizer state (identical replica on every rank) and the batch source of one config."""
        mode, ekw, skw, drops, _ = CONFIGS[cfg_name]
        if a.no_dropout:
            drops = (0.0, 0.0, 0.0, 0.0)
        pn, L, P, d = a.part_num, skw["part_len"], skw["n_patch"], ekw["d_model"]
        args = Namespace(batch_size=bs_l, part_num=pn, part_len=L, n_patch=P, lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8,
                         lambda_BCE=1.0, lambda_normal=0.2, lambda_abnormal=2.0, temporal_only=False, clip_grad=False)
        torch.manual_seed(seed_off)       # same replica on every rank
        enc = Encoder(n_layers=3, n_head=8, d_k=256, d_v=256, MHA_attn_dropout=drops[0], MHA_fc_dropout=drops[1],
                      FFN_dropout=drops[2], weight_init=(mode != "LTN"), **ekw).to(dev).train()
        head = (Classifier(d, drops[3]) if mode == "LTN" else Regressor(d, drops[3])).to(dev).train()
        ts = TrainStep(args, mode, enc, head, lr_encoder=1e-4 * a.lr_scale, lr_head=1e-2 * a.lr_scale, weight_decay=1e-3,
                       cls_only=not a.naive_last_layer, fuse_qkv=a.fuse_qkv, grad_reduce_dtype=a.grad_reduce_dtype,
                       n_buckets=a.buckets or None)
        feed = feed or a.feed
        if feed == "resident":
            src = SyntheticResidentPairs(cfg_name, bs_g, pn, dev, rank if strong else 0, world if strong else 1,
                                         seed=1000 + 97 * seed_off + (0 if strong else rank), max_clips=a.max_clips)
            nxt = src.next_batch
        else:
            gen = torch.Generator(device=dev).manual_seed(1000 + rank + 97 * seed_off)
            T = pn * L
            nf = 0.5 * torch.relu(torch.randn(bs_l, T, P, d, device=dev, generator=gen))
            af = 0.5 * torch.relu(torch.randn(bs_l, T, P, d, device=dev, generator=gen))
            u = torch.rand(bs_l, T, 1, device=dev, generator=gen)
            al = torch.where(u > 0.9, u, torch.zeros_like(u))            # pseudo labels, rule of README.md:27
            src, nxt = None, (lambda: (nf, af, al))
        return ts, nxt, src

    def timed_pass(cfg, dtype, feed=None, steps=None, warmup=None, gemm_events=True, dump_dir=None):
        """Fresh weights and optimizer state, W untimed steps, K timed steps between barrier + synchronize; MAX over ranks.
        ``dump_dir``: write the last timed step's outputs there (rank 0) before anything else runs on the models."""
        steps = a.steps if steps is None else steps
        warmup = a.warmup if warmup is None else warmup
        Fn.set_compute_dtype(dtype)
        Fn.reset_rng(0)
        torch.cuda.reset_peak_memory_stats(dev)
        mixed = cfg == "mixed_ubn_sht"
        if mixed:
            if bs_local % 2:
                raise SystemExit("mixed_ubn_sht needs an even number of pairs per rank")
            parts = [make("ltn_ubnormal", bs_local // 2, bs_global // 2, 0, feed), make("ltn_sht", bs_local // 2, bs_global // 2, 1, feed)]
            ms_ = MixedStep([p[0] for p in parts])
            mixed_out = [None]                     # every model's scalars of the latest step (--dump-outputs)

            def run_step():
                mixed_out[0] = ms_.step([p[1]() for p in parts])
                return mixed_out[0][-1]
            tss = [p[0] for p in parts]
        else:
            ts, nxt, src = make(cfg, bs_local, bs_global, 0, feed)
            if a.graph and src is not None:
                src.lazy = False                   # a captured step reads its batch from static buffers
            if a.graph:
                if world > 1:
                    raise SystemExit("--graph captures the single-rank step only")
                from lstc_vad_amd.engine import GraphedStep
                gs = GraphedStep(ts, *nxt())
                run_step = lambda: gs.step(*nxt())
            else:
                run_step = lambda: ts.step(*nxt())
            tss = [ts]
        for _ in range(warmup):
            run_step()
        sync()
        if world > 1 or force_dist:
            for t in tss:                                          # backward / exposed-communication events of the timed steps
                t.comm_events = []
        want_events = gemm_events and not a.no_gemm_events and not a.graph      # a replayed graph records no per-GEMM events
        # exact-f32 steps are long (280 ms): the events around every GEMM ride inside the timed region.  In the 16-bit modes a
        # step is 5x shorter and the ~360 event records per step cost the HOST 2-5 ms of it (bf16, 8 pairs: 23.1 vs 17.8 ms per
        # step with / without events), so there the K steps are timed clean and the events are taken on 3 further steps.
        inline_events = want_events and dtype == "fp32"
        prof = [] if inline_events else None
        Fn.set_gemm_profiling(prof)
        Fn._pack_prof = None
        scs = []
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]      # step boundaries on the launch stream
        t0 = time.perf_counter()
        marks[0].record()
        for i in range(steps):
            scs.append(run_step())
            marks[i + 1].record()
        sync()
        dt = time.perf_counter() - t0
        dumped = None
        if dump_dir and rank == 0:
            dumped = dump_outputs(dump_dir, mixed_out[0] if mixed else [scs[-1]],
                                  list(zip(("ltn_ubnormal.", "ltn_sht."), tss)) if mixed else [("", tss[0])])
        step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
        comm = None
        if any(t.comm_events for t in tss):
            # per step: backward = first event -> after backward; exposed = after backward -> after reducer.finish() on the launch
            # stream (the buckets' reductions started inside the backward; what is left here is what the backward did not hide)
            # (a mixed step carries a 4th mark per model: the end of ALL models' backwards - a model's reductions that run beside
            # the next model's backward are hidden, not exposed; the last reduction may also land before the backward ends)
            exposed = lambda e: max(0.0, (e[3] if len(e) > 3 else e[1]).elapsed_time(e[2]))
            evs = [t.comm_events for t in tss if t.comm_events]
            bw = sum(e[0].elapsed_time(e[1]) for ev_ in evs for e in ev_) / steps
            ex = sum(max(exposed(ev_[i]) for ev_ in evs) for i in range(min(len(ev_) for ev_ in evs))) / steps
            cm = torch.tensor([bw, ex], device=dev, dtype=torch.float64)
            if world > 1:
                reduce_report(cm, dist.ReduceOp.MAX)
            comm = {"backward_ms_per_step": round(float(cm[0]), 3), "comm_exposed_ms_per_step": round(float(cm[1]), 3),
                    "allreduce_buckets": [len(t.reducer.buckets) for t in tss if t.reducer is not None],
                    "bucket_MB": [[round(b.numel() * 4 / 1e6, 1) for b in t.reducer.buckets] for t in tss if t.reducer is not None]}
            for t in tss:
                t.comm_events = None
        Fn.set_gemm_profiling(None)
        pprof, prof_steps = None, steps
        if want_events and not inline_events and a.full:
            prof, pprof, prof_steps = [], [], 3
            Fn.set_gemm_profiling(prof)
            Fn._pack_prof = pprof
            for _ in range(prof_steps):
                run_step()
            sync()
            Fn.set_gemm_profiling(None)
            Fn._pack_prof = None
        Fn.set_compute_dtype("fp32")
        if world > 1:
            tt = torch.tensor([dt], device=dev, dtype=torch.float64)
            reduce_report(tt, dist.ReduceOp.MAX)
            dt = float(tt.item())
        first, last = torch.stack([scs[0], scs[-1]]).clone()
        if world > 1:                      # scalars are rank-local contributions: their sum is the global loss
            both = torch.stack([first, last]); reduce_report(both); first, last = both
        med = step_ms[steps // 2] if steps % 2 else 0.5 * (step_ms[steps // 2 - 1] + step_ms[steps // 2])
        if world > 1:
            tm = torch.tensor([med], device=dev, dtype=torch.float64)
            reduce_report(tm, dist.ReduceOp.MAX)
            med = float(tm.item())
        res = {"dt": dt, "steps": steps, "step_ms_median": med, "step_ms_min": step_ms[0], "step_ms_max": step_ms[-1], "prof": prof, "pprof": pprof, "prof_steps": prof_steps, "events_inline": inline_events, "loss_first": float(first[0]), "loss_last": float(last[0]),
               "hbm": torch.cuda.max_memory_allocated(dev), "comm": comm,
               "allreduce_MB": round(sum(t.reducer.payload_bytes() for t in tss if t.reducer is not None) / 1e6, 1),
               "bank_GB": None if mixed or src is None else round(src.bank_GB, 2), "dumped": dumped}
        del tss, run_step
        if mixed:
            del parts, ms_
        else:
            del ts, nxt, src
        import gc
        gc.collect()
        torch.cuda.empty_cache()
        return res

    def snippets_per_step(cfg):
        names = ["ltn_ubnormal", "ltn_sht"] if cfg == "mixed_ubn_sht" else [cfg]
        b = bs_global // 2 if cfg == "mixed_ubn_sht" else bs_global
        return sum(2 * b * a.part_num * CONFIGS[n][2]["part_len"] for n in names)

    def roofline_of(res, dtype, cfg):
        prof = res["prof"]
        if not prof:
            return None
        fl = sum(p[0] for p in prof)
        ms = sum(p[1].elapsed_time(p[2]) for p in prof)
        ach = fl / (ms * 1e-3) / 1e12
        # f32x3: three f16 MFMA products per f32 product -> the f32-equivalent ceiling is the 16-bit peak / 3
        peak = {"fp32": FP32_MFMA_PEAK_TFLOPS, "f32x3": round(BF16_MFMA_PEAK_TFLOPS / 3, 1), "bf16": BF16_MFMA_PEAK_TFLOPS}[dtype]
        kname = {"fp32": "gemm_f32_kernel (v_mfma_f32_32x32x2_f32)",
                 "f32x3": "gemm_pk2s_kernel (3 x v_mfma_f32_32x32x16_f16 per f32 product, packed 2-plane operands; small products "
                          "on gemm_f32_kernel)",
                 "bf16": "gemm_bf16p_kernel (v_mfma_f32_16x16x32_bf16 (forward / input-gradient form) and v_mfma_f32_32x32x16_bf16 (weight-gradient form) on packed bf16 tiles streamed by LDS-DMA, 256x256x64; small / batched products on gemm_bf16c_kernel)"}[dtype]
        k = res["prof_steps"]
        roof = {"bound": "mfma", "kernel": kname, "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
                "frac": round(ach / peak, 4), "traffic": None, "launches_per_step": len(prof) // k,
                "gemm_ms_per_step": round(ms / k, 3), "step_executed_gemm_tflop": round(fl / k / 1e12, 3),
                "step_frac_of_peak_executed": round(fl / k / (res["dt"] / res["steps"]) / 1e12 / peak, 4),
                "events": "HIP events on the launch stream around every lstc_gemm, " +
                          ("inside the timed region" if res["events_inline"] else f"on {k} further steps right after the timed region")}
        if res["pprof"]:
            pms = sum(q[1].elapsed_time(q[2]) for q in res["pprof"])
            roof["pack_ms_per_step"] = round(pms / k, 3)
            roof["pack_launches_per_step"] = len(res["pprof"]) // k
            roof["pack_input_GBps"] = round(sum(q[0] for q in res["pprof"]) / (pms * 1e-3) / 1e9, 1)
        return roof

    def alg_tflop(cfg):
        names = ["ltn_ubnormal", "ltn_sht"] if cfg == "mixed_ubn_sht" else [cfg]
        b = bs_global // 2 if cfg == "mixed_ubn_sht" else bs_global
        tot = 0.0
        for n in names:
            m_, e_, s_, _, _ = CONFIGS[n]
            S_ = 1 + (s_["part_len"] * s_["n_patch"] if m_ == "LTN" else s_["n_patch"])
            tot += train_flops_per_sequence(S_, e_["d_model"], 2048, e_["d_inner"], 3, 2 if m_ == "LTN" else 1) * \
                2 * b * a.part_num * (1 if m_ == "LTN" else s_["part_len"])
        return tot / 1e12

    def pmc_traffic(cfg, dtype):
        """HBM-side bytes of ONE launch of the dominant GEMM shape, read from the committed rocprofv3 --pmc passes
        (profiles/gemm_pmc_traffic.json) - a per-launch counter figure for that one shape, not a per-step sum, and labelled so."""
        pmc = os.path.join(ROOT, "profiles", "gemm_pmc_traffic.json")
        if not os.path.exists(pmc) or world != 1:
            return None
        try:
            tab = json.load(open(pmc))
            key = cfg if dtype == "fp32" else f"{cfg}_{dtype}"
            if key not in tab:
                return None
            return {"bytes": tab[key], "algorithmic_bytes": tab.get(key + "_algorithmic"),
                    "scope": tab.get(key + "_scope", "one launch of the dominant GEMM shape, profiles/gemm_pmc_traffic.json"),
                    "source": "rocprofv3 --pmc FETCH_SIZE (x2 on gfx950) + WRITE_SIZE, separate passes; static figure from the committed "
                              "profile, not measured in this run"}
        except Exception:
            return None

    def sub_object(res, cfg, dtype):
        o = {"value": round(snippets_per_step(cfg) * res["steps"] / res["dt"], 1), "unit": "snippets/s",
             "ms_per_step": round(1e3 * res["dt"] / res["steps"], 3), "ms_per_step_median": round(res["step_ms_median"], 3),
             "loss_first_timed_step": res["loss_first"],
             "loss_last_timed_step": res["loss_last"], "hbm_peak_GB": round(res["hbm"] / 1e9, 2)}
        if dtype == "bf16":
            o["act_dtype"] = a.act_dtype
        r = roofline_of(res, dtype, cfg)
        if r:
            t = pmc_traffic(cfg, dtype)
            if t is not None:
                r["traffic"] = t
            else:
                del r["traffic"]               # sub-objects carry the key only with a counter figure behind it (profiles/gemm_pmc_traffic.json)
            o["roofline"] = r
        return o

    # ---- the CPU baseline leg first (rank 0, N = 1): the GPU passes then run back to back.  The GPU idles during this leg -
    # a utilisation average taken over the whole bench.py run (the driver's gpu_busy) includes these seconds; the line says so.
    cpu_base = None
    if a.full and world == 1 and not a.no_cpu_baseline and a.config != "mixed_ubn_sht":
        # torch-CPU sgemm on the GPU box's host peaks at 16-32 threads (tools/cpu_threads_scan.py: 1.3 TFLOP/s
        # at 16-32, 0.5 at 128 of 256 hardware threads), so the baseline uses min(32, available) threads
        t_cpu = time.perf_counter()
        cpu_base = cpu_baseline(a.config, min(32, len(os.sched_getaffinity(0))))
        cpu_base["wall_s"] = round(time.perf_counter() - t_cpu, 1)
        cpu_base["note"] = ("timed BEFORE the GPU passes with the GPU idle: a GPU-utilisation average over the whole bench.py run "
                            "includes these wall_s seconds of host-only work")

    # ---- the headline pass -------------------------------------------------------------------------------------------
    head_res = timed_pass(a.config, a.dtype, dump_dir=a.dump_outputs)
    value = snippets_per_step(a.config) * a.steps / head_res["dt"]

    # ---- --full: everything else the line can report ----------------------------------------------------------------
    extras = {}
    solo = a.full and world == 1 and not force_dist and not a.no_extras and a.config != "mixed_ubn_sht"
    if solo:
        if a.feed == "resident":
            extras["static_batch"] = dict(sub_object(timed_pass(a.config, a.dtype, feed="static", gemm_events=False), a.config, a.dtype),
                                          note="same step on ONE fixed HBM batch: no window sampling, no lstc_gather_rows")
        if a.config == "ltn_sht":
            extras["stn_headline"] = dict(sub_object(timed_pass("stn_sht", a.dtype), "stn_sht", a.dtype),
                                          workload="stn_sht: STN full training step on the literal [64,32,16,2048] input (L=1, S=17, "
                                                   "n_hidden=3027, 2048 sequences/step), MIL loss, resident feed",
                                          step_algorithmic_tflop=round(alg_tflop("stn_sht"), 3))
        if a.dtype == "fp32":
            extras["bf16"] = dict(sub_object(timed_pass(a.config, "bf16"), a.config, "bf16"),
                                  dtype="bf16 MFMA (operands rounded to bf16 RNE), f32 accumulate, f32 master weights / softmax / "
                                        "LayerNorm arithmetic / loss / Adagrad; activations between the full layers stored as bf16 packs "
                                        "when act_dtype is bf16 (BASELINE configs 3 and 5)")
            extras["f32x3"] = dict(sub_object(timed_pass(a.config, "f32x3"), a.config, "f32x3"),
                                   dtype="f32 storage and accumulation; products of the large GEMMs on the f16 matrix cores (two scaled "
                                         "f16 planes per operand, hh + hl + lh); narrower than IEEE f32 products, reported as an extra")
    if solo and a.config == "ltn_sht" and a.dtype == "fp32" and not a.no_coteach:
        # BASELINE config 3 ("Full STN -> pseudo-label -> LTN co-teaching loop, ShanghaiTech config, bf16, 1xMI355X"): one round through
        # the command-line entry points, timed stage by stage (tools/coteach_round.py; README.md:21-36 of the reference is the loop)
        import shutil
        import tempfile
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        tmp = tempfile.mkdtemp(prefix="lstc_coteach_")
        try:
            from coteach_round import run_round
            extras["coteach_loop"] = run_round(tmp, "bf16", steps=6, pairs=48)
        except Exception as e:                      # the headline must survive a failure of an extra
            extras["coteach_loop"] = {"error": f"{type(e).__name__}: {e}"}
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
            Fn.set_compute_dtype("fp32")
    pcie = None
    if (a.h2d or (a.full and not a.no_h2d)) and world == 1 and not force_dist and a.config != "mixed_ubn_sht":
        from lstc_vad_amd.feed import PinnedFeeder
        Fn.set_compute_dtype(a.dtype)
        ts, nxt, _ = make(a.config, bs_local, bs_global, 0, "static")
        nf, af, al = nxt()
        host = tuple(t.cpu() for t in (nf, torch.zeros_like(al), af, al))
        h_steps = a.steps if a.h2d else min(a.steps, 10)
        feeder = PinnedFeeder((host for _ in range(h_steps + 2)), dev)
        t1 = None
        for i, (hnf, _, haf, hal) in enumerate(feeder):
            if i == 2:
                torch.cuda.synchronize(); t1 = time.perf_counter()
            ts.step(hnf, haf, hal)
        torch.cuda.synchronize()
        dth = (time.perf_counter() - t1) / h_steps
        Fn.set_compute_dtype("fp32")
        pcie = {"value": round(snippets_per_step(a.config) / dth, 1), "unit": "snippets/s", "ms_per_step": round(1e3 * dth, 3),
                "batch_MB": round(sum(t.numel() * 4 for t in host) / 1e6, 1), "steps": h_steps,
                "note": "the reference's per-step H2D (Train/temporal_transformer_shanghaitech.py:115-118): the batch is copied "
                        "pageable->pinned->HBM every step on a side stream, overlapped with the previous step; never `value`"}
        del ts, nxt, feeder

    rccl_ranks = 1
    dist_backend = dist.get_backend() if dist.is_initialized() else None      # "nccl" = RCCL; "gloo" only in the shared-device functional checks
    if dist.is_initialized():
        # ranks that really joined the communicator: every rank contributes a 1 to a sum-all-reduce over RCCL
        one = torch.ones(1, device=dev, dtype=torch.float32)
        reduce_report(one)
        rccl_ranks = int(round(float(one.item())))
    if rank == 0:
        mixed = a.config == "mixed_ubn_sht"
        last = "ltn_sht" if mixed else a.config
        mode, ekw, skw, drops, _ = CONFIGS[last]
        pn, L, P, d = a.part_num, skw["part_len"], skw["n_patch"], ekw["d_model"]
        S = 1 + (L * P if mode == "LTN" else P)
        b_l = bs_local // 2 if mixed else bs_local
        nseq = 2 * b_l * pn * (1 if mode == "LTN" else L)
        roof = roofline_of(head_res, a.dtype, a.config)
        if roof is not None:
            if not mixed:
                roof["traffic"] = pmc_traffic(a.config, a.dtype)
            # SURVEY 8(d) counts the full last layer; the step skips its dead rows (only the CLS token of the last layer is
            # read) and re-associates its K/V projections, so executed GEMM FLOPs < algorithmic FLOPs.  frac is on EXECUTED
            # work; on the algorithmic count the same step would read frac_on_algorithmic_flops (can exceed 1).
            roof["step_algorithmic_tflop"] = round(alg_tflop(a.config) / world, 3)          # per rank
            roof["frac_on_algorithmic_flops"] = round(alg_tflop(a.config) / world / (head_res["dt"] / a.steps) / roof["peak"], 4)
        fused = os.environ.get("LSTC_EAGER_GATHER", "0") != "1" and not a.graph
        feed_txt = ("batch formed every step inside the timed region: host window sampler (utils/load_dataset.py:69-88 rule) + "
                    + ("the rows gathered inside the CLS concat (lstc_cls_concat_gather_fwd)" if fused else "lstc_gather_rows")
                    + " from an HBM-resident bank of %s GB" % head_res["bank_GB"]) if a.feed == "resident" else \
            "one fixed HBM-resident batch (no batch formation in the timed region)"
        out = {"metric": "snippets/sec training step (B=64,T=32,P=16,d=2048)", "value": round(value, 1),
               "unit": "snippets/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
               "ms_per_step": round(1e3 * head_res["dt"] / a.steps, 3),
               "ms_per_step_median": round(head_res["step_ms_median"], 3),
               "ms_per_step_min_max": [round(head_res["step_ms_min"], 3), round(head_res["step_ms_max"], 3)],
               "value_at_median_step": round(snippets_per_step(a.config) / (head_res["step_ms_median"] * 1e-3), 1),
               "timing": "value and ms_per_step = K steps between barrier + synchronize (wall clock, max over ranks); "
                         "ms_per_step_median = median of the K per-step intervals between HIP events on the launch stream "
                         "(SURVEY 8d's t_step)",
               "higher_is_better": True, "scaling": a.scaling,
               "vs_baseline": None, "dtype": {"fp32": "f32", "f32x3": "f32 (operands split into 2 scaled f16 planes, 3 f16-MFMA products, f32 accumulate)",
                                              "bf16": "bf16 (f32 accumulate, f32 master weights; activations as bf16 packs under act_dtype bf16)"}[a.dtype], "data": "synthetic",
               "config": {"workload": ("mixed batch (BASELINE config 5): UBnormal videos (d=1024, L=5, S=81) + SHT videos (d=2048, L=3, "
                                       "S=49) in equal numbers, two model pairs, one iteration; second model: " if mixed else "") +
                                      f"{last}: {mode} full training step (batch formation+fwd+loss+bwd+"
                                      f"{'allreduce+' if world > 1 else ''}Adagrad), GLOBAL batch B={2 * bs_global} videos x T={pn} parts x "
                                      f"L={L} snippets x P={P} patches, d_model={d}, n_hidden={ekw['d_inner']}, S={S}, "
                                      f"dropout={'off' if a.no_dropout else 'reference rates'}, lr = reference x {a.lr_scale:g}, "
                                      f"{'step replayed as one captured HIP graph, ' if a.graph else ''}last layer: "
                                      f"{'all tokens (naive)' if a.naive_last_layer else 'CLS token only, K/V projections re-associated (exact)'}; "
                                      f"fresh weights and Adagrad state for the timed pass",
                          "feed": feed_txt, "global_videos": 2 * bs_global, "parallelism": f"dp{world}",
                          "per_rank_pairs": bs_local, "per_rank_sequences": nseq, "allreduce_MB": head_res["allreduce_MB"],
                          # rccl_ranks counts the ranks of the process group that answered a sum-all-reduce; whether that group IS
                          # RCCL is dist_backend ("nccl" = RCCL over xGMI; "gloo" = the one-GPU functional check, never a measurement)
                          "rccl_ranks": rccl_ranks, "dist_backend": dist_backend,
                          # N > 1: HIP events on the launch stream around backward and around reducer.finish() (max over ranks, mean
                          # over the timed steps): how much of the gradient all-reduce the backward did not hide
                          **(head_res["comm"] or {}),
                          "grad_reduce_dtype": a.grad_reduce_dtype,
                          **({"act_dtype": a.act_dtype} if a.dtype == "bf16" else {}),
                          "nccl_env": {k: v for k, v in sorted(os.environ.items()) if k.startswith(("NCCL_", "RCCL_"))}},
               "loss_first_timed_step": head_res["loss_first"], "loss_last_timed_step": head_res["loss_last"],
               "hbm_peak_GB": round(head_res["hbm"] / 1e9, 2), "roofline": roof}
        if head_res["dumped"]:
            out["dumped_outputs"] = head_res["dumped"]
        out.update(extras)
        if pcie:
            out["pcie_inclusive"] = pcie
        if cpu_base is not None:
            out["cpu_baseline"] = cpu_base
        os.write(real_stdout, (json.dumps(out) + "\n").encode())
    if world > 1 or force_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
