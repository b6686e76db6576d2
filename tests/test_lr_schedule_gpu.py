"""Learning-rate schedules on the device: ``lstc_lr_schedule`` against the host twin launch by launch, ``lstc_adagrad_multi_scaled``
bit for bit against ``lstc_adagrad_multi`` and against the float32 chain of tests/util_lr_schedule.py, and ``optim.LRSchedule``
through the optimizers and the engine: Adam under an attached schedule, partitions of a step, the captured step, a resumed run
and two data-parallel ranks.  tests/test_lr_schedule_host.py proves what the grid used here can tell apart."""
import ctypes as C
import os
import sys

import pytest
import torch

import util_adam as ua
import util_lr_schedule as ul
from util import load_case, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _cosine_word(word, want):
    """A cosine scale read from the device against the host twin's: the same float32 number or one next to it."""
    return abs(int(_bits(word.detach().cpu().reshape(1))) - int(_bits(torch.tensor([float(want)])))) <= 1


# ------------------------------------------------------------------------------------------- the schedule kernel
def _desc(kw):
    from lstc_vad_amd import _lib
    return _lib.LrSchedule(ul.KINDS.index(kw["kind"]), kw["warmup_steps"], kw["total_steps"] or 0, kw.get("step_size") or 0,
                           kw["warmup_start"], kw["min_scale"], kw.get("gamma", 0.1))


def _launches(kw, n, start=0):
    """``n`` consecutive launches on ONE word pair; the two words after each launch, read back once at the end."""
    from lstc_vad_amd import _lib
    lib, d = _lib.load(), _desc(kw)
    step = torch.full((1,), start, dtype=torch.int32, device=DEV)
    scale = torch.full((1,), float("nan"), device=DEV)
    steps, scales = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for i in range(n):
        _lib.check(lib.lstc_lr_schedule(C.byref(d), step.data_ptr(), scale.data_ptr(), stream), "lstc_lr_schedule")
        steps[i:i + 1].copy_(step)
        scales[i:i + 1].copy_(scale)
    torch.cuda.synchronize()
    return steps.cpu(), scales.cpu()


@pytest.mark.parametrize("W,T", ul.GPU_GRID)
def test_every_launch_writes_the_host_twins_scale_and_counts_one_step(W, T):
    """T + 4 launches per kind, floor and warm-up start: the step word is the launch count, the scale is the twin's - the same bits
    for the kinds made of float64 + - * / sqrt and one rounding, equal or adjacent float32 numbers for cosine, whose float64
    ``cos`` may differ in the last place between the device and the host."""
    seen = set()
    for kw in ul.configs(((W, T),)):
        steps, scales = _launches(kw, T + 4)
        assert steps.tolist() == list(range(1, T + 5)), kw
        want = torch.tensor([float(ul.twin(t, **kw)) for t in range(T + 4)], dtype=torch.float32)
        if kw["kind"] == "cosine":
            assert int((_bits(scales) - _bits(want)).abs().max()) <= 1, (kw, scales, want)
        else:
            assert _same_bits(scales, want), (kw, scales, want)
        seen.add((kw["kind"], kw.get("step_size")))
    assert seen == {("constant", None), ("linear", None), ("cosine", None), ("inv_sqrt", None), ("step", 1), ("step", 3)}


def test_a_step_word_at_int32_max_stays_there():
    for kw in (dict(kind="constant", warmup_steps=0, total_steps=0, min_scale=0.0, warmup_start=0.0),
               dict(kind="inv_sqrt", warmup_steps=4, total_steps=0, min_scale=0.0, warmup_start=0.0)):
        steps, scales = _launches(kw, 3, start=INT32_MAX - 1)
        assert steps.tolist() == [INT32_MAX] * 3, kw
        want = torch.tensor([float(ul.twin(t, **kw)) for t in (INT32_MAX - 1, INT32_MAX, INT32_MAX)], dtype=torch.float32)
        assert _same_bits(scales, want) and bool((want > 0).all()), (kw, scales, want)


# ------------------------------------------------------------------------------------------- scaled Adagrad
SIZES = (1, 3, 4, 5, ua.PER_WG - 1, ua.PER_WG, ua.PER_WG + 5, 2 * ua.PER_WG + 1)
N_ITEMS, UNALIGNED_AT = 49, 14          # 49 items: 48 + 1 over two launches; item 14 (PER_WG + 5 elements) starts 4 bytes off a 16-byte boundary


def _ada_items():
    items = [ua.Item(SIZES[i % len(SIZES)], (1e-2 * (1 + i % 3), (0.0, 1e-3)[i % 2], 1e-10, (1.0, 0.37)[(i // 2) % 2]), i == UNALIGNED_AT)
             for i in range(N_ITEMS)]
    assert items[UNALIGNED_AT].n == ua.PER_WG + 5
    return items


@pytest.fixture(scope="module")
def ada_case():
    """(items, offsets, the three host arenas w / grad / state): NaN guards between the items' regions, a state as earlier steps
    would have left it."""
    items = _ada_items()
    offs, total = ua.layout(items)
    assert offs[UNALIGNED_AT] % 4 == 1 and all(o % 4 == 0 for i, o in enumerate(offs) if i != UNALIGNED_AT)
    g = torch.Generator().manual_seed(7)
    arenas = [torch.full((total,), float("nan")) for _ in range(3)]
    for it, o in zip(items, offs):
        arenas[0][o:o + it.n] = torch.randn(it.n, generator=g)
        arenas[1][o:o + it.n] = torch.randn(it.n, generator=g)
        arenas[2][o:o + it.n] = 0.01 + torch.rand(it.n, generator=g)
    arenas[1][offs[2]] = 0.0                                            # a zero gradient where there is no weight decay
    return items, offs, arenas


def _ada_run(case, entry, scale=None, lr_of=lambda it: it.hyper[0]):
    """One call of ``entry`` over all 49 items from the case's start; returns the w and state arenas on the host."""
    from lstc_vad_amd import _lib
    lib = _lib.load()
    items, offs, arenas = case
    w, grad, s = (a.to(DEV) for a in arenas)
    assert all(a.data_ptr() % 16 == 0 for a in (w, grad, s))
    rows = [_lib.AdagradItem(w.data_ptr() + 4 * o, grad.data_ptr() + 4 * o, s.data_ptr() + 4 * o, it.n, lr_of(it), *it.hyper[1:])
            for it, o in zip(items, offs)]
    arr = (_lib.AdagradItem * len(rows))(*rows)
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "lstc_adagrad_multi":
        _lib.check(lib.lstc_adagrad_multi(arr, len(rows), stream), entry)
    else:
        word = torch.full((1,), scale, device=DEV)
        _lib.check(lib.lstc_adagrad_multi_scaled(arr, len(rows), word.data_ptr(), stream), entry)
    torch.cuda.synchronize()
    assert torch.equal(grad.cpu().view(torch.int32), arenas[1].view(torch.int32))          # the gradients are read only
    return w.cpu(), s.cpu()


def test_scaled_adagrad_at_scale_one_is_the_plain_entry_bit_for_bit(ada_case):
    items, offs, arenas = ada_case
    plain = _ada_run(ada_case, "lstc_adagrad_multi")
    scaled = _ada_run(ada_case, "lstc_adagrad_multi_scaled", 1.0)
    mask = ua.data_mask(items, offs, arenas[0].numel())
    for a, b, start in zip(plain, scaled, (arenas[0], arenas[2])):
        assert _same_bits(a, b)
        assert bool(torch.isnan(a[~mask]).all()) and bool(torch.isfinite(a[mask]).all())      # the guards between the items stay
        assert not _same_bits(a, start)


@pytest.mark.parametrize("scale", [0.37, 0.0])
def test_scaled_adagrad_is_the_chain_with_lr_t_rounded_once(ada_case, scale):
    """lr_t = (float)((double)lr * (double)scale), formed on the host in float64 as tests/util_adam.py forms Adam's and rounded once,
    then the element chain in float32, one correctly rounded operation after the other: every weight and every sum of the 49
    tensors equals the host's chain (tests/util_lr_schedule.adagrad_scaled_step) bit for bit, and equals the plain entry handed
    that lr_t as its ``lr``."""
    items, offs, arenas = ada_case
    got_w, got_s = _ada_run(ada_case, "lstc_adagrad_multi_scaled", scale)
    lr_t = lambda it: ul.f32(ul.f32(it.hyper[0]) * ul.f32(scale))
    via_w, via_s = _ada_run(ada_case, "lstc_adagrad_multi", lr_of=lr_t)
    assert _same_bits(got_w, via_w) and _same_bits(got_s, via_s)
    for i, (it, o) in enumerate(zip(items, offs)):
        w, grad, s = (a[o:o + it.n] for a in arenas)
        want_w, want_s = ul.adagrad_scaled_step(w, grad, s, *it.hyper, scale)
        differ = int((_bits(got_w[o:o + it.n]) != _bits(want_w)).sum()), int((_bits(got_s[o:o + it.n]) != _bits(want_s)).sum())
        assert differ == (0, 0), (i, it.n, differ)
        if scale == 0.0:
            assert _same_bits(got_w[o:o + it.n], w) and not _same_bits(got_s[o:o + it.n], s)   # lr_t = 0: the sums still move
    mask = ua.data_mask(items, offs, arenas[0].numel())
    assert bool(torch.isnan(got_w[~mask]).all()) and bool(torch.isnan(got_s[~mask]).all())


# ------------------------------------------------------------------------------------------- optim.LRSchedule and the optimizers
SHAPES = ((3, 7), (8193,), (64, 129), (1,), (5,), (300, 31), (4,))


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(DEV)) for s in SHAPES]


def _grads(ps, k):
    g = torch.Generator().manual_seed(100 + k)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)


def _groups(ps):
    return [{"params": ps[:3], "lr": 1e-2}, {"params": ps[3:], "lr": 3e-2}]


def _opt_state(opt, sched=None):
    """Every parameter, every tensor the optimizer keeps for it (Adam's step words as floats) and its host count; then the
    schedule's two words and its host count."""
    torch.cuda.synchronize()
    ps = [p for grp in opt.param_groups for p in grp["params"]]
    tensors = [p.detach().clone() for p in ps]
    for p in ps:
        tensors += [v.clone().float() for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
    counts = [opt.host_step(p) for p in ps]
    if sched is not None:
        tensors += [sched._scale.clone(), sched._step.clone().float()]
        counts += [int(sched._step), sched.host_step()]
    return tensors, counts


def _same_state(a, b):
    return len(a[0]) == len(b[0]) and all(_same_bits(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1]


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_adam_under_an_attached_schedule_is_adam_with_the_scale_set_by_hand(name):
    from lstc_vad_amd import optim
    kw = dict(kind="linear", warmup_steps=2, total_steps=5)
    ps, qs = _params(), _params()
    a, b = getattr(optim, name)(_groups(ps), weight_decay=0.1), getattr(optim, name)(_groups(qs), weight_decay=0.1)
    sched = optim.LRSchedule(a, **kw)
    scales = []
    for t in range(5):
        _grads(ps, t), _grads(qs, t)
        sched.step()
        a.step()
        b.set_lr_scale(optim.LRSchedule.scale_at(t, **kw))
        b.step()
        scales.append(float(sched._scale))
        assert sched.get_last_lr() == [g["lr"] * scales[-1] for g in a.param_groups]
    assert scales == [0.0, 0.5, 1.0, float(ul.twin(3, **kw)), float(ul.twin(4, **kw))] and 0.3 < scales[4] < scales[3] < 0.7
    assert _same_state(_opt_state(a), _opt_state(b))
    assert int(sched._step) == 5 == sched.host_step() and all(int(a.state[p]["step"]) == 5 for p in ps)
    assert not any(_same_bits(p, q) for p, q in zip(ps, _params()))


@pytest.mark.parametrize("name", ["Adagrad", "AdamW"])
def test_one_tick_then_any_partition_into_only_sets_is_one_tick_then_a_whole_step(name):
    from lstc_vad_amd import optim
    kw = dict(kind="cosine", warmup_steps=1, total_steps=4, min_scale=0.1, warmup_start=0.25)
    ps = _params()
    whole = getattr(optim, name)(_groups(ps), weight_decay=1e-3)
    ws = optim.LRSchedule(whole, **kw)
    plain_ps = _params()
    plain = getattr(optim, name)(_groups(plain_ps), weight_decay=1e-3)              # no schedule: the rates stay constant
    for k in range(3):
        _grads(ps, k), _grads(plain_ps, k)
        ws.step()
        whole.step()
        plain.step()
    want = _opt_state(whole, ws)
    assert want[1][-2:] == [3, 3] and _cosine_word(ws._scale, ul.twin(2, **kw)) and 0.7 < float(ws._scale) < 0.8
    assert not any(_same_bits(p, q) for p, q in zip(ps, plain_ps))                   # the schedule did move the weights
    for order in ((0, 1), (1, 0)):
        qs = _params()
        parts = (qs[0:1] + qs[4:], qs[1:4])                                          # A and B, each across both param groups
        opt = getattr(optim, name)(_groups(qs), weight_decay=1e-3)
        sc = optim.LRSchedule(opt, **kw)
        for k in range(3):
            _grads(qs, k)
            sc.step()                                                                # ONE tick per training step
            for j in order:
                opt.step(only=parts[j])
        assert _same_state(want, _opt_state(opt, sc)), order


@pytest.mark.parametrize("name", ["Adagrad", "AdamW"])
def test_a_state_dict_resumes_the_schedule_and_the_run_bit_for_bit(name):
    from lstc_vad_amd import optim
    kw = dict(kind="cosine", warmup_steps=1, total_steps=4, min_scale=0.1)
    ps = _params()
    opt = getattr(optim, name)(_groups(ps), weight_decay=1e-3)
    sched = optim.LRSchedule(opt, **kw)
    qs = _params()
    first = getattr(optim, name)(_groups(qs), weight_decay=1e-3)
    fs = optim.LRSchedule(first, **kw)
    for k in range(4):
        _grads(ps, k)
        sched.step()
        opt.step()
        if k < 2:
            _grads(qs, k)
            fs.step()
            first.step()
    torch.cuda.synchronize()
    sd_opt, sd_sched = first.state_dict(), fs.state_dict()
    assert sd_sched["step"] == 2
    rs = [torch.nn.Parameter(q.detach().clone()) for q in qs]
    cont = getattr(optim, name)(_groups(rs), weight_decay=1e-3)
    cont.load_state_dict(sd_opt)
    cs = optim.LRSchedule(cont, **kw)
    cs.load_state_dict(sd_sched)
    assert int(cs._step) == 2 == cs.host_step()
    for k in (2, 3):
        _grads(rs, k)
        cs.step()
        cont.step()
    got, want = _opt_state(cont, cs), _opt_state(opt, sched)
    assert _same_state(got, want) and want[1][-2:] == [4, 4] and set(want[1]) == {4}
    assert _cosine_word(cs._scale, ul.twin(3, **kw)) and 0.3 < float(cs._scale) < 0.35


# ------------------------------------------------------------------------------------------- through the engine
def _state(ts):
    """Weights, every tensor the optimizer keeps, the averages, the schedule's two words; the device counts and the host's."""
    tensors, counts = _opt_state(ts.optimizer, ts.schedule)
    if ts.ema is not None:
        tensors += [ts.ema.state[p]["avg"].clone() for p in ts.ema.params]
        counts += [int(ts.ema.state[p]["count"]) for p in ts.ema.params] + [ts.ema.host_count(p) for p in ts.ema.params]
    return tensors, counts


@pytest.mark.parametrize("optimizer,ema", [("adagrad", None), ("adamw", 0.5)])
def test_graphed_step_with_a_schedule_is_bitwise_the_eager_step(optimizer, ema):
    """engine.GraphedStep under a cosine schedule (W = 1, T = 3) on the reduced LTN case, dropout on: three replays against three
    eager steps - scalars, weights, optimizer state, averages, the schedule's step and scale words and every host count bit for
    bit.  Constructing the GraphedStep (its warm-up and its capture both run the tick) leaves the schedule at step 0, and a
    captured Adagrad step follows the schedule: its weights are not those of the constant-rate run."""
    from test_ema_gpu import _args, _models
    from lstc_vad_amd import functional as Fn
    from lstc_vad_amd.engine import GraphedStep, TrainStep
    z, mode, ekw, skw = load_case("ltn_sht")
    d = ekw["d_model"]
    batches = []
    for i in range(3):
        batches.append(tuple(t.to(DEV) for t in (torch.from_numpy(z["norm_feats"]) * (1.0 + 0.1 * i),
                                                 torch.from_numpy(z["abnorm_feats"]) * (1.0 - 0.05 * i), torch.from_numpy(z["abnorm_labs"]))))
    kw = dict(kind="cosine", warmup_steps=1, total_steps=3, warmup_start=0.25)
    res = {}
    for how in ("eager", "graph", "constant"):
        enc, head = _models(mode, dict(ekw), d, 0.2, 0.3)
        enc.load_state_dict(sub(z, "enc_init."), strict=True)
        head.load_state_dict(sub(z, "head_init."), strict=True)
        enc, head = enc.to(DEV).train(), head.to(DEV).train()
        extra = dict(ema_decay=ema, ema_warmup=True) if ema else {}
        ts = TrainStep(_args(skw), mode, enc, head, 1e-3, 1e-2, 1e-2, fuse_qkv="off", optimizer=optimizer,
                       lr_schedule=None if how == "constant" else kw, **extra)
        Fn.reset_rng(11)
        if how == "graph":
            untouched = _state(ts)
            stepper = GraphedStep(ts, *batches[0])
            assert Fn._counter == 11 and _same_state(untouched, _state(ts))       # construction leaves everything as it was
            assert int(ts.schedule._step) == 0 == ts.schedule.host_step()
        else:
            stepper = ts
        scs = [stepper.step(*batches[i]).clone() for i in range(3)]
        res[how] = (scs, _state(ts), Fn._counter)
        if how != "constant":
            assert int(ts.schedule._step) == 3 == ts.schedule.host_step() and _cosine_word(ts.schedule._scale, ul.twin(2, **kw))
    for a, b in zip(res["eager"][0], res["graph"][0]):
        assert torch.equal(a, b), (a, b)
    assert res["eager"][2] == res["graph"][2]
    assert _same_state(res["eager"][1], res["graph"][1])
    n = len(list(ts.optimizer.param_groups[0]["params"]))
    moved = [not _same_bits(x, y) for x, y in zip(res["graph"][1][0][:n], res["constant"][1][0][:n])]
    assert sum(moved) > n // 2, moved                                         # the captured step ran at the schedule's rates


def _sched_rank(rank, world, port, q):
    """One rank of a two-rank job on the shared device (gloo): three scheduled steps on the reduced LTN case per optimizer, once
    stepping after all reductions and once per bucket (LSTC_BUCKET_STEPS=1), from the same initial weights."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from test_ema_gpu import _args, _models
        from lstc_vad_amd.engine import TrainStep
        dev = torch.device("cuda", 0)
        z, mode, ekw, skw = load_case("ltn_sht")
        d, h = ekw["d_model"], skw["batch_size"] // world
        sl = slice(rank * h, (rank + 1) * h)
        nf, af, al = (torch.from_numpy(z[k])[sl].to(dev) for k in ("norm_feats", "abnorm_feats", "abnorm_labs"))
        kw = dict(kind="linear", warmup_steps=2, total_steps=4, warmup_start=0.25)
        same = lambda x, y: bool(torch.equal(x.view(torch.int32), y.view(torch.int32)))
        out = {"bucket_steps_identical": [], "per_bucket": [], "words": [], "replicas_identical": [], "finite": [], "moved": []}
        for optimizer in ("adagrad", "adamw"):
            flats = []
            for bucket_steps, sched in (("0", kw), ("1", kw), ("0", None)):
                os.environ["LSTC_BUCKET_STEPS"] = bucket_steps
                enc, head = _models(mode, dict(ekw), d, 0.0, 0.0)
                enc.load_state_dict(sub(z, "enc_init."), strict=True)
                head.load_state_dict(sub(z, "head_init."), strict=True)
                enc, head = enc.to(dev).train(), head.to(dev).train()
                ts = TrainStep(_args(skw, bs=h), mode, enc, head, 1e-4, 1e-2, 1e-2, fuse_qkv="off", optimizer=optimizer, lr_schedule=sched)
                assert ts.reducer is not None and ts.reducer.active and ts.bucket_steps == (bucket_steps == "1")
                for _ in range(3):
                    ts.step(nf, af, al)
                torch.cuda.synchronize()
                flats.append(torch.cat([p.detach().reshape(-1) for grp in ts.optimizer.param_groups for p in grp["params"]]))
                if sched is not None:
                    out["per_bucket"].append(ts.reducer.landed is not None)
                    out["words"].append((int(ts.schedule._step), ts.schedule.host_step(), float(ts.schedule._scale)))
            out["bucket_steps_identical"].append(same(flats[0], flats[1]))
            out["moved"].append(not same(flats[0], flats[2]))
            both = [torch.empty_like(flats[0]) for _ in range(world)]
            dist.all_gather(both, flats[0])
            out["replicas_identical"].append(same(both[0], both[1]))
            out["finite"].append(bool(torch.isfinite(flats[0]).all()))
        if rank == 0:
            q.put(out)
        dist.barrier()
    finally:
        os.environ["LSTC_BUCKET_STEPS"] = "0"
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_hold_identical_weights_and_bucket_steps_change_nothing():
    from test_dist_gpu import _two_ranks
    res = _two_ranks(_sched_rank, ())
    for key in ("finite", "replicas_identical", "bucket_steps_identical", "moved"):
        assert res[key] == [True, True], res
    assert res["per_bucket"] == [False, True, False, True], res
    assert res["words"] == [(3, 3, 1.0)] * 4, res                        # step 2 of W = 2 is the first at full rate
