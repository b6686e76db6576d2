"""Adam / AdamW on the device: ``lstc_adam_multi`` through the C ABI against the float64 reference of tests/util_adam.py, one
step at a time from the device's own state (errors do not accumulate; the bar per tensor is util_rowops.tol), and the Python
optimizers through the engine: partitions of a step, missing gradients, packed bf16 weight copies, the captured step and two
data-parallel ranks.  tests/test_adam_host.py proves what the bars used here can and cannot tell apart."""
import os
import sys

import pytest
import torch

import util_adam as ua
from util import load_case, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------- through the C ABI
def _run(items, arenas, offs, steps=3, split=None, lr_scale=None, keep_before=False):
    """``steps`` consecutive calls of lstc_adam_multi over ``items`` laid out in copies of the four host ``arenas``.  ``split``:
    two calls per step (items [0, split) then the rest).  ``lr_scale``: a device float, else NULL.  Returns the arenas and the
    step words on the host, and with ``keep_before`` the arenas in front of every step."""
    from lstc_vad_amd import _lib
    lib = _lib.load()
    dev = [a.to(DEV) for a in arenas]
    assert all(a.data_ptr() % 16 == 0 for a in dev)               # an offset that is 1 mod 4 floats is 4 bytes off a 16-byte boundary
    words = torch.zeros(len(items), dtype=torch.int32, device=DEV)
    scale = None if lr_scale is None else torch.tensor([lr_scale], dtype=torch.float32, device=DEV)
    rows = []
    for i, (it, o) in enumerate(zip(items, offs)):
        h = it.hyper
        rows.append(_lib.AdamItem(*(a.data_ptr() + 4 * o for a in dev), it.n, words.data_ptr() + 4 * i,
                                  None if scale is None else scale.data_ptr(), h.lr, h.beta1, h.beta2, h.eps, h.weight_decay,
                                  h.grad_scale, h.decoupled))
    before = []
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(steps):
        if keep_before:
            before.append([a.cpu() for a in dev])
        for part in ((rows,) if split is None else (rows[:split], rows[split:])):
            arr = (_lib.AdamItem * len(part))(*part)
            _lib.check(lib.lstc_adam_multi(arr, len(part), stream), "lstc_adam_multi")
    torch.cuda.synchronize()
    return [a.cpu() for a in dev], words.cpu(), before


@pytest.fixture(scope="module")
def case():
    items = ua.gpu_items()
    arenas, offs = ua.gpu_inputs(items)
    return items, arenas, offs


@pytest.fixture(scope="module")
def three_steps(case):
    items, arenas, offs = case
    return _run(items, arenas, offs, keep_before=True)


def test_each_of_three_steps_is_the_float64_step_from_the_device_state(case, three_steps):
    """60 items (two launches), both modes, every size the kernel treats differently, t = 1, 2, 3 read from the words."""
    items, arenas, offs = case
    after, words, before = three_steps
    assert words.tolist() == [3] * len(items)                     # the empty item's word included
    mask = ua.data_mask(items, offs, arenas[0].numel())
    for a0, a1 in zip(arenas, after):
        assert torch.isnan(a1[~mask]).all() and torch.isnan(a0[~mask]).all()          # nothing written outside the items
        assert torch.isfinite(a1[mask]).all()
    assert _same_bits(arenas[1], after[1])                         # gradients are read only
    states = before + [after]
    for t in (1, 2, 3):
        b4, now = states[t - 1], states[t]
        for i, (it, o) in enumerate(zip(items, offs)):
            if it.n == 0:
                continue
            sl = slice(o, o + it.n)
            ref, bar = ua.bars(*(a[sl] for a in b4), t, it.hyper)
            for name, k, r, b in zip("wmv", (0, 2, 3), ref, bar):
                err = float((now[k][sl].double() - r).abs().max())
                assert err <= b, (t, i, it.n, name, err, b)
    # pointers 4 bytes off a 16-byte boundary: the scalar path gives the bits of the float4 path
    u, a = offs[ua.UNALIGNED_AT], offs[ua.ALIGNED_TWIN_AT]
    n = items[ua.UNALIGNED_AT].n
    assert u % 4 == 1 and a % 4 == 0
    for k in (0, 2, 3):
        assert _same_bits(after[k][u:u + n], after[k][a:a + n])
        assert not _same_bits(after[k][u:u + n], arenas[k][u:u + n])


def test_runs_and_splits_into_calls_are_bit_identical(case, three_steps):
    items, arenas, offs = case
    after, words, _ = three_steps
    for split in (None, 30):
        again, words2, _ = _run(items, arenas, offs, split=split)
        assert torch.equal(words, words2)
        for a, b in zip(after, again):
            assert _same_bits(a, b), split


def test_lr_scale_word_is_the_halved_learning_rate_bit_for_bit():
    """lr = 2**-6 with a device lr_scale of 0.5 against lr = 2**-7 with NULL: the product is exact, so the bits must agree - and
    differ from the unscaled run."""
    full, half = ua.gpu_items(lr=2.0 ** -6), ua.gpu_items(lr=2.0 ** -7)
    arenas, offs = ua.gpu_inputs(full, seed=1)
    scaled, w1, _ = _run(full, arenas, offs, lr_scale=0.5)
    by_value, w2, _ = _run(half, arenas, offs)
    unscaled, _, _ = _run(full, arenas, offs, steps=1)
    one, _, _ = _run(full, arenas, offs, steps=1, lr_scale=1.0)
    assert torch.equal(w1, w2)
    for a, b in zip(scaled, by_value):
        assert _same_bits(a, b)
    assert not _same_bits(scaled[0], unscaled[0])
    for a, b in zip(one, unscaled):
        assert _same_bits(a, b)                                    # a word of 1.0 is NULL


def test_integer_family_equals_float64():
    """Inputs whose every intermediate is a float32 number (tests/test_adam_host.py asserts which): the kernel must EQUAL the
    float64 step.  beta2 = 0.75: w, m and v.  beta1 = beta2 = 0.5: m and v - sqrt(2) enters w, which meets its bar instead."""
    fams = [(b2, dec, ua.int_family(b2, dec)) for b2 in (0.5, 0.75) for dec in (0, 1)]
    items = [ua.Item(f[0].numel(), f[4], False) for _, _, f in fams]
    offs, total = ua.layout(items)
    arenas = [torch.full((total,), float("nan")) for _ in range(4)]
    for (_, _, f), o, it in zip(fams, offs, items):
        for a, x in zip(arenas, f[:4]):
            a[o:o + it.n] = x
    after, words, _ = _run(items, arenas, offs, steps=1)
    assert words.tolist() == [1] * 4
    for (b2, dec, f), o, it in zip(fams, offs, items):
        sl = slice(o, o + it.n)
        ref, bar = ua.bars(*f[:4], 1, it.hyper)
        assert torch.equal(after[2][sl].double(), ref[1]) and torch.equal(after[3][sl].double(), ref[2]), (b2, dec)
        if b2 == 0.75:
            assert torch.equal(after[0][sl].double(), ref[0]), (b2, dec)
        else:
            assert float((after[0][sl].double() - ref[0]).abs().max()) <= bar[0], (b2, dec)


# ------------------------------------------------------------------------------------------- through the Python optimizers
SHAPES = ((3, 7), (8193,), (64, 129), (1,), (5,), (300, 31), (4,))


def _params(seed=0, grads=True):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in SHAPES]
    if grads:
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(DEV)
    return ps


def _snapshot(opt, ps):
    torch.cuda.synchronize()
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), int(opt.state[p]["step"]),
             opt.host_step(p)) for p in ps]


def _same_snapshot(a, b):
    return all(_same_bits(x[0], y[0]) and _same_bits(x[1], y[1]) and _same_bits(x[2], y[2]) and x[3:] == y[3:] for x, y in zip(a, b))


def test_any_partition_into_only_sets_is_one_whole_step():
    from lstc_vad_amd.optim import AdamW
    kw = dict(lr=1e-2, weight_decay=0.1)
    ps = _params()
    whole = AdamW([{"params": ps[:3], "lr": 3e-3}, {"params": ps[3:]}], **kw)
    for _ in range(2):
        whole.step()
    want = _snapshot(whole, ps)
    assert [s[3] for s in want] == [2] * len(ps) == [s[4] for s in want]
    for order in ((0, 1, 2), (2, 0, 1)):
        qs = _params()
        parts = (qs[0:1] + qs[5:], qs[1:3], qs[3:5])
        opt = AdamW([{"params": qs[:3], "lr": 3e-3}, {"params": qs[3:]}], **kw)
        for _ in range(2):
            for k in order:
                opt.step(only=parts[k])
        assert _same_snapshot(want, _snapshot(opt, qs)), order


def test_a_parameter_without_gradient_keeps_weight_state_and_count():
    from lstc_vad_amd.optim import Adam
    ps = _params()
    opt = Adam(ps, lr=1e-2)
    opt.step()
    before = _snapshot(opt, ps)
    ps[2].grad = None
    opt.step()
    after = _snapshot(opt, ps)
    assert _same_snapshot(before[2:3], after[2:3]) and after[2][3:] == (1, 1)
    assert all(a[3:] == (2, 2) and not _same_bits(a[0], b[0]) for k, (a, b) in enumerate(zip(after, before)) if k != 2)
    sd = opt.state_dict()["state"]
    assert [float(sd[k]["step"]) for k in range(len(ps))] == [2.0, 2.0, 1.0] + [2.0] * (len(ps) - 3)


def test_stepped_weight_is_repacked_for_the_packed_bf16_gemm():
    """bf16 mode: a weight whose product takes the packed bf16 GEMM keeps a packed copy; AdamW rewrites the weight through a raw
    pointer.  The same product run again must be the product with a fresh parameter holding the stepped values - the shared
    bump_weight_epoch / repack_weights tail of the optimizers - and not the product with the stale pack."""
    from lstc_vad_amd import _lib
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.optim import AdamW
    # the smallest product functional.gemm sends to the packed kernel: min(M, N) and K at their bounds, then M N K at its own
    mn, kmin, mnk = Fn._x3_min[0], Fn._x3_min[1], min(Fn._x3_min[2], Fn._BF16P_MIN_MNK)
    M = N = mn
    K = max(kmin, -(-mnk // (M * N)))
    g = torch.Generator().manual_seed(2)
    x = torch.randn(M, K, generator=g).to(DEV)
    W = torch.nn.Parameter(torch.randn(N, K, generator=g).to(DEV))
    Fn.set_compute_dtype("bf16")
    try:
        y0 = Fn.gemm(x, W, trans_b=True)
        packs = W.__dict__.get("_lstc_packs")
        assert packs and all(kind == _lib.BF16P for _, kind in packs), "the product did not take the packed bf16 kernel"
        W.grad = torch.randn(N, K, generator=g).to(DEV)
        AdamW([W], lr=1e-1).step()
        y1 = Fn.gemm(x, W, trans_b=True)
        fresh = torch.nn.Parameter(W.detach().clone())
        y2 = Fn.gemm(x, fresh, trans_b=True)
        torch.cuda.synchronize()
    finally:
        Fn.set_compute_dtype("fp32")
    assert _same_bits(y1, y2)
    assert not _same_bits(y0, y1)


def _models(mode, ekw, d, dropout, head_dropout):
    from lstc_vad_amd.models import Classifier, Encoder, Regressor
    enc = Encoder(n_layers=3, MHA_attn_dropout=dropout, MHA_fc_dropout=dropout, FFN_dropout=dropout, position_dropout=dropout,
                  weight_init=False, **ekw)
    head = (Classifier if mode == "LTN" else Regressor)(d, head_dropout, weight_init=False)
    return enc, head


def _args(skw, bs=None):
    from argparse import Namespace
    return Namespace(batch_size=skw["batch_size"] if bs is None else bs, part_num=skw["part_num"], part_len=skw["part_len"],
                     n_patch=skw["n_patch"], lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8, lambda_BCE=1.0, lambda_normal=0.2,
                     lambda_abnormal=2.0, temporal_only=False, clip_grad=False)


def _opt_state(ts):
    torch.cuda.synchronize()
    ps = [p for grp in ts.optimizer.param_groups for p in grp["params"]]
    return ([p.detach().clone() for p in ps], [ts.optimizer.state[p]["exp_avg"].clone() for p in ps],
            [ts.optimizer.state[p]["exp_avg_sq"].clone() for p in ps], [int(ts.optimizer.state[p]["step"]) for p in ps],
            [ts.optimizer.host_step(p) for p in ps])


def _same_opt_state(a, b):
    return all(_same_bits(x, y) for k in range(3) for x, y in zip(a[k], b[k])) and a[3] == b[3] and a[4] == b[4]


@pytest.mark.parametrize("rescale", [False, True])
def test_graphed_adamw_step_is_bitwise_the_eager_step(rescale):
    """engine.GraphedStep with optimizer="adamw" on the reduced LTN case, dropout on: three replays against three eager steps -
    scalars, weights, exp_avg, exp_avg_sq, the device step words and the host's counts bit for bit; with ``rescale`` the
    learning-rate word is set to 0.5 before the second step of both runs (the replayed launch reads it on the device)."""
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.engine import GraphedStep, TrainStep
    z, mode, ekw, skw = load_case("ltn_sht")
    d = ekw["d_model"]
    batches = []
    for i in range(3):
        batches.append(tuple(t.to(DEV) for t in (torch.from_numpy(z["norm_feats"]) * (1.0 + 0.1 * i),
                                                 torch.from_numpy(z["abnorm_feats"]) * (1.0 - 0.05 * i), torch.from_numpy(z["abnorm_labs"]))))
    res = {}
    for how in ("eager", "graph"):
        enc, head = _models(mode, dict(ekw), d, 0.2, 0.3)
        enc.load_state_dict(sub(z, "enc_init."), strict=True)
        head.load_state_dict(sub(z, "head_init."), strict=True)
        enc, head = enc.to(DEV).train(), head.to(DEV).train()
        ts = TrainStep(_args(skw), mode, enc, head, 1e-3, 1e-2, 1e-2, fuse_qkv="off", optimizer="adamw",
                       optimizer_kw=dict(betas=(0.9, 0.99), eps=1e-6))
        assert type(ts.optimizer).__name__ == "AdamW" and ts.optimizer.param_groups[0]["betas"] == (0.9, 0.99)
        Fn.reset_rng(11)
        if how == "graph":
            untouched = _opt_state(ts)
            stepper = GraphedStep(ts, *batches[0])
            assert Fn._counter == 11 and _same_opt_state(untouched, _opt_state(ts))       # construction leaves everything as it was
            assert set(untouched[3]) == {0}
        else:
            stepper = ts
        scs = []
        for i in range(3):
            if rescale and i == 1:
                ts.optimizer.set_lr_scale(0.5)
            scs.append(stepper.step(*batches[i]).clone())
        res[how] = (scs, _opt_state(ts), Fn._counter, ts.optimizer.state_dict())
    for a, b in zip(res["eager"][0], res["graph"][0]):
        assert torch.equal(a, b), (a, b)
    assert res["eager"][2] == res["graph"][2]
    assert _same_opt_state(res["eager"][1], res["graph"][1])
    assert set(res["eager"][1][3]) <= {0, 3} and 3 in res["eager"][1][3] and res["eager"][1][3] == res["eager"][1][4]
    sa, sb = res["eager"][3]["state"], res["graph"][3]["state"]
    assert sa.keys() == sb.keys() and all(float(sa[k]["step"]) == float(sb[k]["step"]) == 3.0 for k in sa)


def _adam_rank(rank, world, port, q):
    """One rank of a two-rank job on the shared device (gloo): two AdamW steps on the reduced LTN case, once stepping after all
    reductions and once per bucket (LSTC_BUCKET_STEPS=1), from the same initial weights."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lstc_vad_amd.engine import TrainStep
        dev = torch.device("cuda", 0)
        z, mode, ekw, skw = load_case("ltn_sht")
        d, h = ekw["d_model"], skw["batch_size"] // world
        sl = slice(rank * h, (rank + 1) * h)
        nf, af, al = (torch.from_numpy(z[k])[sl].to(dev) for k in ("norm_feats", "abnorm_feats", "abnorm_labs"))
        flats, per_bucket, moved = [], [], []
        for bucket_steps in ("0", "1"):
            os.environ["LSTC_BUCKET_STEPS"] = bucket_steps
            enc, head = _models(mode, dict(ekw), d, 0.0, 0.0)
            enc.load_state_dict(sub(z, "enc_init."), strict=True)
            head.load_state_dict(sub(z, "head_init."), strict=True)
            enc, head = enc.to(dev).train(), head.to(dev).train()
            ts = TrainStep(_args(skw, bs=h), mode, enc, head, 1e-4, 1e-2, 1e-2, fuse_qkv="off", optimizer="adamw")
            assert ts.reducer is not None and ts.reducer.active and ts.bucket_steps == (bucket_steps == "1")
            flat = lambda: torch.cat([p.detach().reshape(-1) for p in list(enc.parameters()) + list(head.parameters())])
            init = flat()
            for _ in range(2):
                ts.step(nf, af, al)
            torch.cuda.synchronize()
            moved.append(not torch.equal(init, flat()))
            per_bucket.append(ts.reducer.landed is not None)
            flats.append(flat())
            steps = sorted({int(ts.optimizer.state[p]["step"]) for grp in ts.optimizer.param_groups for p in grp["params"]})
        out = {"bucket_steps_identical": bool(torch.equal(flats[0].view(torch.int32), flats[1].view(torch.int32))),
               "per_bucket": per_bucket, "steps": steps, "moved": all(moved)}
        both = [torch.empty_like(flats[0]) for _ in range(world)]
        dist.all_gather(both, flats[0])
        out["replicas_identical"] = bool(torch.equal(both[0].view(torch.int32), both[1].view(torch.int32)))
        out["finite"] = bool(torch.isfinite(flats[0]).all())
        if rank == 0:
            q.put(out)
        dist.barrier()
    finally:
        os.environ["LSTC_BUCKET_STEPS"] = "0"
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_hold_identical_weights_and_bucket_steps_change_nothing():
    from test_dist_gpu import _two_ranks
    res = _two_ranks(_adam_rank, ())
    assert res["finite"] and res["moved"] and res["replicas_identical"] and res["bucket_steps_identical"], res
    assert res["per_bucket"] == [False, True] and res["steps"] in ([2], [0, 2]), res
