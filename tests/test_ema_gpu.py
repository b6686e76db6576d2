"""EMA weights on the device: ``lstc_ema_multi`` and ``lstc_swap_multi`` through the C ABI against the float64 reference of
tests/util_ema.py, one update at a time from the device's own state (errors do not accumulate; the bar per tensor is
util_rowops.tol), and ``optim.EMA`` through the engine and the command line: partitions of an update, the state dict, packed bf16
weight copies around ``averaged()``, the captured step and two data-parallel ranks.  tests/test_ema_host.py proves what the bars
used here can and cannot tell apart."""
import os
import sys

import pytest
import torch

import util_ema as ue
from util import load_case, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------- through the C ABI
def _run(items, avg0, offs, w_of, updates, split=None, decay=ue.DECAY, keep_before=False):
    """Consecutive calls of lstc_ema_multi over ``items``: the averages in a copy of the host arena ``avg0``, the weights of
    update t copied from ``w_of(t)`` into ONE device arena in front of it (the pointers never move).  ``split``: two calls per
    update (items [0, split) then the rest).  Returns the average arena and the count words on the host, and with
    ``keep_before`` the average arena in front of every update."""
    from lstc_vad_amd import _lib
    lib = _lib.load()
    avg = avg0.to(DEV)
    w_first, offs_w = w_of(updates[0])
    w = torch.empty_like(w_first, device=DEV)
    assert avg.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0          # an offset that is 1 mod 4 floats is 4 bytes off a 16-byte boundary
    words = torch.zeros(len(items), dtype=torch.int32, device=DEV)
    rows = [_lib.EmaItem(avg.data_ptr() + 4 * o, w.data_ptr() + 4 * ow, it.n, words.data_ptr() + 4 * i, decay, it.warmup)
            for i, (it, o, ow) in enumerate(zip(items, offs, offs_w))]
    before = []
    stream = torch.cuda.current_stream().cuda_stream
    for t in updates:
        w.copy_(w_of(t)[0])
        if keep_before:
            before.append(avg.cpu())
        for part in ((rows,) if split is None else (rows[:split], rows[split:])):
            arr = (_lib.EmaItem * len(part))(*part)
            _lib.check(lib.lstc_ema_multi(arr, len(part), stream), "lstc_ema_multi")
    torch.cuda.synchronize()
    return avg.cpu(), words.cpu(), before


@pytest.fixture(scope="module")
def case():
    items = ue.gpu_items()
    avg0, offs = ue.first_average(items)
    ws = {t: ue.weights(items, t) for t in ue.UPDATES}
    return items, avg0, offs, ws.__getitem__


@pytest.fixture(scope="module")
def twelve_updates(case):
    items, avg0, offs, w_of = case
    return _run(items, avg0, offs, w_of, ue.UPDATES, keep_before=True)


def test_each_of_twelve_updates_is_the_float64_update_from_the_device_state(case, twelve_updates):
    """60 items (two launches), with and without warm-up, every size the kernel treats differently, t = 1 .. 12 read from the
    words: the copy, the ramp, its exact crossing at t = 9 and the plateau."""
    items, avg0, offs, w_of = case
    after, words, before = twelve_updates
    assert words.tolist() == [12] * len(items)                    # the empty item's word included
    mask = ue.data_mask(items, offs, avg0.numel())
    assert torch.isnan(after[~mask]).all() and torch.isnan(avg0[~mask]).all()          # nothing written outside the items
    assert torch.isfinite(after[mask]).all()
    states = before + [after]
    for t in ue.UPDATES:
        b4, now = states[t - 1], states[t]
        worst = 0.0
        w_arena, offs_w = w_of(t)
        for i, (it, o, ow) in enumerate(zip(items, offs, offs_w)):
            if it.n == 0:
                continue
            w = w_arena[ow:ow + it.n]
            if t == 1:
                assert _same_bits(now[o:o + it.n], w) and not _same_bits(b4[o:o + it.n], w), i          # a copy, not a blend
                continue
            ref, bar = ue.bar(b4[o:o + it.n], w, t, ue.DECAY, it.warmup)
            err = float((now[o:o + it.n].double() - ref).abs().max())
            worst = max(worst, err / bar)
            assert err <= bar, (t, i, it.n, err, bar)
        print(f"update {t}: largest error / bar over the items {worst:.3f}")
    # a weight 4 bytes off a 16-byte boundary: the scalar path gives the bits of the float4 path
    u, a = offs[ue.UNALIGNED_AT], offs[ue.ALIGNED_TWIN_AT]
    n = items[ue.UNALIGNED_AT].n
    assert w_of(1)[1][ue.UNALIGNED_AT] % 4 == 1 and w_of(1)[1][ue.ALIGNED_TWIN_AT] % 4 == 0
    for s in states[1:]:
        assert _same_bits(s[u:u + n], s[a:a + n])
    assert not _same_bits(after[u:u + n], states[1][u:u + n])


def test_runs_and_splits_into_calls_are_bit_identical(case, twelve_updates):
    items, avg0, offs, w_of = case
    after, words, _ = twelve_updates
    for split in (None, 30, 47):
        again, words2, _ = _run(items, avg0, offs, w_of, ue.UPDATES, split=split)
        assert torch.equal(words, words2)
        assert _same_bits(after, again), split


def test_integer_family_equals_float64():
    """Multiples of 8 below 2**10, decay 0.5, no warm-up (tests/test_ema_host.py asserts that every intermediate is a float32
    number): three updates must EQUAL float64."""
    avg0, ws = ue.int_family()
    items = [ue.Item(avg0.numel(), 0, False)]
    after, words, before = _run(items, avg0, [0], lambda t: (ws[t - 1], [0]), (1, 2, 3), keep_before=True)
    assert words.tolist() == [3]
    ref = avg0.double()
    for t, (w, got) in enumerate(zip(ws, before[1:] + [after]), 1):
        ref = ue.ema_step(ref, w, t, 0.5, False)
        assert torch.equal(got.double(), ref), t


def test_swap_exchanges_the_bits_of_every_item_and_twice_is_the_identity(case):
    from lstc_vad_amd import _lib
    lib = _lib.load()
    items, avg0, offs, w_of = case
    w0, offs_w = w_of(1)
    a0, b0 = avg0.clone(), w0.clone()
    # bit patterns an arithmetic path would not carry over: a NaN with a payload, -0, a denormal
    big = offs[ue.UNALIGNED_AT]
    _bits(a0)[big:big + 3] = torch.tensor([0x7FC12345, -0x80000000, 1], dtype=torch.int32)
    a, b = a0.to(DEV), b0.to(DEV)
    rows = [_lib.SwapItem(a.data_ptr() + 4 * o, b.data_ptr() + 4 * ow, it.n) for it, o, ow in zip(items, offs, offs_w)]
    arr = (_lib.SwapItem * len(rows))(*rows)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.lstc_swap_multi(arr, len(rows), stream), "lstc_swap_multi")
    a1, b1 = a.cpu(), b.cpu()
    _lib.check(lib.lstc_swap_multi(arr, len(rows), stream), "lstc_swap_multi")
    a2, b2 = a.cpu(), b.cpu()
    assert _same_bits(a2, a0) and _same_bits(b2, b0)
    for i, (it, o, ow) in enumerate(zip(items, offs, offs_w)):
        assert _same_bits(a1[o:o + it.n], b0[ow:ow + it.n]) and _same_bits(b1[ow:ow + it.n], a0[o:o + it.n]), i
    ma, mb = ue.data_mask(items, offs, a0.numel()), ue.data_mask(items, offs_w, b0.numel())
    assert _same_bits(a1[~ma], a0[~ma]) and _same_bits(b1[~mb], b0[~mb])               # nothing written outside the items
    assert not _same_bits(a1, a0)


# ------------------------------------------------------------------------------------------- optim.EMA
SHAPES = ((3, 7), (8193,), (64, 129), (1,), (5,), (300, 31), (4,))


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in SHAPES]


def _move(ps, k):
    """What an optimizer step would do between two updates."""
    g = torch.Generator().manual_seed(50 + k)
    with torch.no_grad():
        for p in ps:
            p.add_(torch.randn(p.shape, generator=g).to(DEV))


def _snapshot(e):
    torch.cuda.synchronize()
    return [(e.state[p]["avg"].clone(), int(e.state[p]["count"]), e.host_count(p)) for p in e.params]


def _same_snapshot(a, b):
    return len(a) == len(b) and all(_same_bits(x[0], y[0]) and x[1:] == y[1:] for x, y in zip(a, b))


def test_any_partition_into_only_sets_is_one_whole_update_and_a_state_dict_continues():
    from lstc_vad_amd.optim import EMA
    ps = _params()
    whole = EMA(ps, decay=0.9, warmup=True)
    for k in range(3):
        _move(ps, k)
        whole.update()
    want = _snapshot(whole)
    assert [s[1:] for s in want] == [(3, 3)] * len(ps)
    assert not any(_same_bits(s[0], p) for s, p in zip(want, ps))
    for order in ((0, 1, 2), (2, 0, 1)):
        qs = _params()
        parts = (qs[0:1] + qs[5:], qs[1:3], qs[3:5])
        e = EMA([{"params": qs[:3]}, {"params": qs[3:]}], decay=0.9, warmup=True)
        for k in range(3):
            _move(qs, k)
            for j in order:
                e.update(only=parts[j])
        assert _same_snapshot(want, _snapshot(e)), order
    # state_dict() -> load_state_dict() into a fresh EMA over fresh parameters: the next updates are the uninterrupted ones
    sd = whole.state_dict()
    assert sd["counts"] == [3] * len(ps) and (sd["decay"], sd["warmup"]) == (0.9, True)
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    cont = EMA(rs, decay=0.5)
    cont.load_state_dict(sd)
    assert _same_snapshot(want, _snapshot(cont))
    for k in (3, 4):
        _move(ps, k), _move(rs, k)
        whole.update(), cont.update()
    assert _same_snapshot(_snapshot(whole), _snapshot(cont)) and _snapshot(cont)[0][1:] == (5, 5)
    # averaged(): in, out, no nesting, no update inside
    before = [p.detach().clone() for p in ps]
    with whole.averaged():
        torch.cuda.synchronize()
        assert all(_same_bits(p, s[0]) for p, s in zip(ps, _snapshot(cont)))
        with pytest.raises(RuntimeError):
            whole.update()
        with pytest.raises(RuntimeError):
            with whole.averaged():
                pass
    assert all(_same_bits(p, b) for p, b in zip(ps, before)) and _same_snapshot(_snapshot(whole), _snapshot(cont))
    with pytest.raises(ZeroDivisionError):
        with whole.averaged():
            1 / 0
    assert all(_same_bits(p, b) for p, b in zip(ps, before))                    # swapped back on the way out of an exception


# ------------------------------------------------------------------------------------------- through the engine
def _models(mode, ekw, d, dropout, head_dropout, n_layers=3):
    from lstc_vad_amd.models import Classifier, Encoder, Regressor
    enc = Encoder(n_layers=n_layers, MHA_attn_dropout=dropout, MHA_fc_dropout=dropout, FFN_dropout=dropout, position_dropout=dropout,
                  weight_init=False, **ekw)
    head = (Classifier if mode == "LTN" else Regressor)(d, head_dropout, weight_init=False)
    return enc, head


def _args(skw, bs=None):
    from argparse import Namespace
    return Namespace(batch_size=skw["batch_size"] if bs is None else bs, part_num=skw["part_num"], part_len=skw["part_len"],
                     n_patch=skw["n_patch"], lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8, lambda_BCE=1.0, lambda_normal=0.2,
                     lambda_abnormal=2.0, temporal_only=False, clip_grad=False)


def _state(ts):
    """Weights, every tensor the optimizer keeps, the averages; the device counts and the host's."""
    torch.cuda.synchronize()
    ps = [p for grp in ts.optimizer.param_groups for p in grp["params"]]
    tensors = [p.detach().clone() for p in ps]
    for p in ps:
        tensors += [v.clone().float() for k, v in sorted(ts.optimizer.state[p].items()) if torch.is_tensor(v)]
    tensors += [ts.ema.state[p]["avg"].clone() for p in ts.ema.params]
    counts = ([ts.optimizer.host_step(p) for p in ps], [int(ts.ema.state[p]["count"]) for p in ts.ema.params],
              [ts.ema.host_count(p) for p in ts.ema.params])
    return tensors, counts


def _same_state(a, b):
    return len(a[0]) == len(b[0]) and all(_same_bits(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]


def test_averaged_rebuilds_the_packed_bf16_weights_on_the_way_in_and_out():
    """bf16 mode, 2 layers at d = 512 and 1056 token rows: the projections and the FFN take the packed bf16 GEMM, which reads
    packed COPIES of the weights.  Scores inside ``averaged()`` must be those of a fresh model holding the averages (not of stale
    packs of the trained weights), and the step after it that of a twin that never entered (not of stale packs of the averages)."""
    from lstc_vad_amd import _lib
    from lstc_vad_amd import functional as Fn
    d = 512
    ekw = dict(n_head=2, d_k=256, d_v=256, d_model=d, d_inner=512, MHA_layerNorm=True, FFN_layerNorm=True)
    skw = dict(batch_size=4, part_num=4, part_len=2, n_patch=16)
    g = torch.Generator().manual_seed(5)
    nf, af = (torch.randn(4, 8, 16, d, generator=g).to(DEV) for _ in range(2))
    al = torch.randint(0, 2, (4, 8), generator=g).float().to(DEV)
    from lstc_vad_amd.engine import TrainStep
    Fn.set_compute_dtype("bf16")
    try:
        torch.manual_seed(0)
        enc0, head0 = _models("LTN", ekw, d, 0.0, 0.0, n_layers=2)
        init = ({k: v.clone() for k, v in enc0.state_dict().items()}, {k: v.clone() for k, v in head0.state_dict().items()})
        twins = []
        for _ in range(2):
            enc, head = _models("LTN", ekw, d, 0.0, 0.0, n_layers=2)
            enc.load_state_dict(init[0]), head.load_state_dict(init[1])
            enc, head = enc.to(DEV).train(), head.to(DEV).train()
            ts = TrainStep(_args(skw), "LTN", enc, head, 1e-3, 1e-2, 1e-3, fuse_qkv="on", optimizer="adamw", ema_decay=0.5)
            for _ in range(2):
                ts.step(nf, af, al)
            twins.append(ts)
        a, b = twins
        assert _same_state(_state(a), _state(b))
        kinds = {kind for p in a.encoder.parameters() for _, kind in (p.__dict__.get("_lstc_packs") or {})}
        assert _lib.BF16P in kinds, "no product took the packed bf16 kernel"

        def scores(enc, head):
            enc.eval(), head.eval()
            with torch.no_grad():
                out = head(enc.forward_cls(a.sequences(nf, af))).clone()
            enc.train(), head.train()
            return out
        trained = scores(a.encoder, a.head)
        with a.ema.averaged():
            inside = scores(a.encoder, a.head)
            held = ({k: v.clone() for k, v in a.encoder.state_dict().items()}, {k: v.clone() for k, v in a.head.state_dict().items()})
        torch.cuda.synchronize()
        for mod, sd in ((a.encoder, held[0]), (a.head, held[1])):
            assert all(_same_bits(sd[k], a.ema.state[p]["avg"]) and not _same_bits(sd[k], p) for k, p in mod.named_parameters()
                       if p.grad is not None)
        assert not _same_bits(inside, trained)
        enc, head = _models("LTN", ekw, d, 0.0, 0.0, n_layers=2)
        enc.load_state_dict(held[0]), head.load_state_dict(held[1])
        enc, head = enc.to(DEV), head.to(DEV)
        for layer in list(enc.layer_stack)[:-1]:
            layer.slf_attn.fuse_qkv_()
        fresh = scores(enc, head)
        assert _same_bits(inside, fresh)
        assert _same_bits(scores(a.encoder, a.head), trained)                 # out again: the trained weights' packs are back
        a.step(nf, af, al), b.step(nf, af, al)
        assert _same_state(_state(a), _state(b))
    finally:
        Fn.set_compute_dtype("fp32")


def test_graphed_adamw_step_with_ema_is_bitwise_the_eager_step():
    """engine.GraphedStep with optimizer="adamw", ema_decay=0.5, ema_warmup=True on the reduced LTN case, dropout on: three replays
    against three eager steps - scalars, weights, optimizer state, averages and every count bit for bit - and constructing the
    GraphedStep (warm-up and capture run the EMA launch too) changed none of them."""
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
        ts = TrainStep(_args(skw), mode, enc, head, 1e-3, 1e-2, 1e-2, fuse_qkv="off", optimizer="adamw", ema_decay=0.5, ema_warmup=True)
        assert (ts.ema.decay, ts.ema.warmup) == (0.5, True) and len(ts.ema.params) == len(list(enc.parameters())) + len(list(head.parameters()))
        Fn.reset_rng(11)
        if how == "graph":
            untouched = _state(ts)
            stepper = GraphedStep(ts, *batches[0])
            assert Fn._counter == 11 and _same_state(untouched, _state(ts))       # construction leaves everything as it was
            assert set(untouched[1][1]) == {0} == set(untouched[1][2])
        else:
            stepper = ts
        scs = [stepper.step(*batches[i]).clone() for i in range(3)]
        res[how] = (scs, _state(ts), Fn._counter)
    for a, b in zip(res["eager"][0], res["graph"][0]):
        assert torch.equal(a, b), (a, b)
    assert res["eager"][2] == res["graph"][2]
    assert _same_state(res["eager"][1], res["graph"][1])
    counts = res["eager"][1][1]
    assert set(counts[1]) == {3} == set(counts[2])                            # every parameter is averaged, with or without a gradient
    # three updates with the ramp 1/10 -> 2/11 -> 3/12 are no copy of the weights
    n = len(ts.ema.params)
    assert not all(_same_bits(w, a) for w, a in zip(res["eager"][1][0][:n], res["eager"][1][0][-n:]))


def _ema_rank(rank, world, port, q):
    """One rank of a two-rank job on the shared device (gloo): two AdamW steps with an EMA on the reduced LTN case, once stepping
    after all reductions and once per bucket (LSTC_BUCKET_STEPS=1), from the same initial weights."""
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
        flats, avgs, per_bucket, counts = [], [], [], []
        for bucket_steps in ("0", "1"):
            os.environ["LSTC_BUCKET_STEPS"] = bucket_steps
            enc, head = _models(mode, dict(ekw), d, 0.0, 0.0)
            enc.load_state_dict(sub(z, "enc_init."), strict=True)
            head.load_state_dict(sub(z, "head_init."), strict=True)
            enc, head = enc.to(dev).train(), head.to(dev).train()
            ts = TrainStep(_args(skw, bs=h), mode, enc, head, 1e-4, 1e-2, 1e-2, fuse_qkv="off", optimizer="adamw", ema_decay=0.5)
            assert ts.reducer is not None and ts.reducer.active and ts.bucket_steps == (bucket_steps == "1")
            for _ in range(2):
                ts.step(nf, af, al)
            torch.cuda.synchronize()
            per_bucket.append(ts.reducer.landed is not None)
            flats.append(torch.cat([p.detach().reshape(-1) for p in ts.ema.params]))
            avgs.append(torch.cat([ts.ema.state[p]["avg"].reshape(-1) for p in ts.ema.params]))
            counts.append(sorted({(int(ts.ema.state[p]["count"]), ts.ema.host_count(p)) for p in ts.ema.params}))
        same = lambda x, y: bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
        out = {"bucket_steps_identical": same(flats[0], flats[1]) and same(avgs[0], avgs[1]), "per_bucket": per_bucket,
               "counts": counts, "average_is_no_copy": not same(flats[0], avgs[0])}
        both = [torch.empty_like(avgs[0]) for _ in range(world)]
        dist.all_gather(both, avgs[0])
        out["replicas_identical"] = same(both[0], both[1])
        out["finite"] = bool(torch.isfinite(avgs[0]).all())
        if rank == 0:
            q.put(out)
        dist.barrier()
    finally:
        os.environ["LSTC_BUCKET_STEPS"] = "0"
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_hold_identical_averages_and_bucket_steps_change_nothing():
    from test_dist_gpu import _two_ranks
    res = _two_ranks(_ema_rank, ())
    assert res["finite"] and res["replicas_identical"] and res["bucket_steps_identical"] and res["average_is_no_copy"], res
    assert res["per_bucket"] == [False, True] and res["counts"] == [[(2, 2)], [(2, 2)]], res


# ------------------------------------------------------------------------------------------- the command line
def test_command_line_saves_the_averages_and_trains_as_without_the_flag(tmp_path, monkeypatch):
    """``--synthetic --steps 6 --ema_decay 0.5 --save_final`` of temporal_transformer_shanghaitech at the small widths of the
    command-line tests, in this process so that the TrainStep can be looked at afterwards: the trained weights and the optimizer
    state are those of the run without the flag (an evaluation inside ``averaged()`` after step 2 included), the files differ from
    them and hold the averages."""
    from lstc_vad_amd import cli, engine
    from lstc_vad_amd import functional as Fn
    made = []

    class Recorded(engine.TrainStep):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(engine, "TrainStep", Recorded)
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", os.environ.get("HIP_VISIBLE_DEVICES", "0"))
    model = ["--d_model", "32", "--n_head", "2", "--d_k", "16", "--d_v", "16", "--n_hidden", "64", "--MHA_layerNorm", "--FFN_layerNorm",
             "--relative_position_encoding", "--part_len", "3", "--n_patch", "16", "--batch_size", "4", "--part_num", "3", "--seed", "3"]
    runs = {}
    for name, extra in (("plain", []), ("ema", ["--ema_decay", "0.5"])):
        Fn.reset_rng(0)
        prefix = str(tmp_path / (name + "_"))
        cli.train("temporal_transformer_shanghaitech", argv=model + extra + [
            "--synthetic", "--steps", "6", "--save_final", prefix, "--log_dir", str(tmp_path / ("log_" + name))])
        torch.cuda.synchronize()
        ts = made[-1]
        files = {**{"e." + k: v for k, v in torch.load(prefix + "encoder.ckpt", map_location="cpu").items()},
                 **{"h." + k: v for k, v in torch.load(prefix + "head.ckpt", map_location="cpu").items()}}
        live = {**{"e." + k: v.detach().cpu().clone() for k, v in ts.encoder.state_dict().items()},
                **{"h." + k: v.detach().cpu().clone() for k, v in ts.head.state_dict().items()}}
        opt = [v.detach().cpu().float() for p in (q for grp in ts.optimizer.param_groups for q in grp["params"])
               for k, v in sorted(ts.optimizer.state[p].items()) if torch.is_tensor(v)]
        runs[name] = (ts, files, live, opt)
    Fn.set_compute_dtype("fp32")
    (tp, fp, lp, op), (te, fe, le, oe) = runs["plain"], runs["ema"]
    assert tp.ema is None and te.ema is not None and (te.ema.decay, te.ema.warmup) == (0.5, False)
    assert lp.keys() == le.keys() == fp.keys() == fe.keys()
    assert all(_same_bits(lp[k], le[k]) for k in lp) and len(op) == len(oe) and all(_same_bits(x, y) for x, y in zip(op, oe))
    assert all(_same_bits(fp[k], lp[k]) for k in lp)                           # without the flag the files are the trained weights
    moved = [k for k in le if not _same_bits(fe[k], le[k])]
    assert any(k.startswith("e.") for k in moved) and any(k.startswith("h.") for k in moved), moved
    named = {**{"e." + k: p for k, p in te.encoder.named_parameters()}, **{"h." + k: p for k, p in te.head.named_parameters()}}
    assert len(named) == len(te.ema.params)
    for k, p in named.items():
        assert _same_bits(fe[k], te.ema.state[p]["avg"].cpu()), k
        assert te.ema.host_count(p) == 6 == int(te.ema.state[p]["count"])
