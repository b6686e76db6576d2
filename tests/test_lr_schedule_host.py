"""Learning-rate schedules, the part that needs no GPU: the host twin ``optim.LRSchedule.scale_at`` against torch's own schedulers
and against exact rational arithmetic, the planted defects of tests/util_lr_schedule.py that the tests' grid must tell apart,
``LstcLrSchedule`` against the C compiler's layout, the refusals ``lstc_lr_schedule`` and ``lstc_adagrad_multi_scaled`` make before
any launch, ``optim.LRSchedule``'s argument checks and state dict on CPU tensors, and the command-line flags."""
import ctypes as C
import os
import subprocess
import warnings
from argparse import Namespace
from fractions import Fraction

import numpy as np
import pytest
import torch

import util_lr_schedule as ul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_NULL, E_SHAPE, E_RANGE = -1, -2, -5
TRAIN_SCRIPTS = ("temporal_transformer_shanghaitech", "temporal_transformer_UCF", "temporal_transformer_UBnormal",
                 "spatio_transformer_shanghaitech", "spatio_transformer_UCF", "spatio_transformer_UBnormal", "spatio_transformer_MIL_CE")


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _scale_at(t, **kw):
    from lstc_vad_amd.optim import LRSchedule
    return LRSchedule.scale_at(t, **kw)


# ------------------------------------------------------------------------------------------- the host twin against torch
# relative 1e-6: one f32 rounding is at most 2^-24 = 6e-8, torch's recursive forms drift by less than 1e-12 over these step counts
# (the absolute term below, for the steps at which the value itself is 0), and an off-by-one in t moves a value by 1e-2 or more
REL, DRIFT = 1e-6, 1e-12
STEP_SIZE, GAMMA = 3, 0.5


def _torch_curve(kind, W, T, m, ws, steps):
    """The rate of a one-parameter optimizer with base rate 1.0 over ``steps`` steps: LinearLR as the warm-up, the decay behind it,
    SequentialLR at milestone W."""
    S = torch.optim.lr_scheduler
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    decay = {"linear": lambda: S.LinearLR(opt, start_factor=1.0, end_factor=m, total_iters=T - W),
             "cosine": lambda: S.CosineAnnealingLR(opt, T_max=T - W, eta_min=m),
             "step": lambda: S.StepLR(opt, step_size=STEP_SIZE, gamma=GAMMA)}[kind]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if W > 0:
            sched = S.SequentialLR(opt, [S.LinearLR(opt, start_factor=ws, end_factor=1.0, total_iters=W), decay()], milestones=[W])
        else:
            sched = decay()
        out = []
        for _ in range(steps):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sched.step()
    return out


@pytest.mark.parametrize("kind", ["linear", "cosine", "step"])
@pytest.mark.parametrize("W,T", ul.HOST_GRID)
def test_host_twin_is_torchs_chained_schedulers(kind, W, T):
    for m in (0.0, 0.1):
        for ws in (0.25, 1.0):
            kw = dict(kind=kind, warmup_steps=W, total_steps=T, min_scale=m, warmup_start=ws)
            if kind == "step":
                kw.update(step_size=STEP_SIZE, gamma=GAMMA)
            theirs = _torch_curve(kind, W, T, m, ws, T + 5)
            for t in range(T + 5):
                ours = float(_scale_at(t, **kw))
                where = (kind, W, T, m, ws, t)
                if kind == "cosine" and t > T:
                    # the steps T + 1 .. T + 4: CosineAnnealingLR is periodic and climbs again behind T_max; the schedule here
                    # stays at min_scale (u = min(t - W, D)), the closed form the header states
                    assert ours == ul.f32(m) and theirs[t] > m + 1e-3, where
                    continue
                want = theirs[t]
                if kind == "step" and want < m:
                    # StepLR has no floor: from the step at which gamma^k falls below min_scale the schedule here holds min_scale
                    assert ours == ul.f32(m), where
                    continue
                assert abs(ours - want) <= REL * abs(want) + DRIFT, where + (ours, want)


def _configs(grid):
    return [c for c in ul.configs(grid)]


def test_host_twin_is_the_restated_twin_bit_for_bit():
    """optim.LRSchedule.scale_at and tests/util_lr_schedule.twin are two statements of one arithmetic: equal on every
    configuration and step both tests use, warm-up of zero steps and steps behind T included."""
    n = 0
    for grid in (ul.HOST_GRID, ul.GPU_GRID):
        for kw in _configs(grid):
            for t in range(kw["total_steps"] + 5):
                a, b = _scale_at(t, **kw), ul.twin(t, **kw)
                assert isinstance(a, np.float32) and a == b, (kw, t, a, b)
                n += 1
    assert n > 2000


def test_constant_inv_sqrt_step_linear_and_the_warm_up_against_exact_rational_arithmetic():
    """Every kind but cosine has a rational value (inv_sqrt: a rational square): the twin is that value rounded once to float32 -
    within 2^-24 relative, plus 2^-50 for the float64 evaluation in front of the rounding."""
    one = Fraction(1, 2 ** 24) + Fraction(1, 2 ** 50)
    seen = set()
    for kw in _configs(ul.HOST_GRID) + _configs(ul.GPU_GRID):
        if kw["kind"] == "cosine":
            continue
        for t in range(kw["total_steps"] + 5):
            got, want = Fraction(float(ul.twin(t, **kw))), ul.exact(t, **kw)
            if isinstance(want, tuple):
                assert abs(got * got - want[1]) <= want[1] * (2 * one + one * one), (kw, t)
                seen.add("sq")
            else:
                assert abs(got - want) <= want * one, (kw, t)
                seen.add(kw["kind"] if t >= kw["warmup_steps"] else "warmup")
    assert seen == {"sq", "warmup", "constant", "linear", "step"}          # inv_sqrt stays above both floors at these step counts
    # a few by hand: the zero-based step index, the warm-up's first and last step, the decay's end points
    lin = dict(kind="linear", warmup_steps=4, total_steps=12, min_scale=0.25, warmup_start=0.5)
    assert [float(_scale_at(t, **lin)) for t in (0, 1, 3, 4, 8, 12, 100)] == [0.5, 0.625, 0.875, 1.0, 0.625, 0.25, 0.25]
    assert [float(_scale_at(t, kind="inv_sqrt", warmup_steps=4)) for t in (0, 2, 4, 16, 64)] == [0.0, 0.5, 1.0, 0.5, 0.25]
    assert [float(_scale_at(t, kind="inv_sqrt")) for t in (0, 1, 4)] == [1.0, 1.0, 0.5]                    # W = 0: W' = 1
    assert [float(_scale_at(t, kind="inv_sqrt", warmup_steps=1, min_scale=0.5)) for t in (1, 4, 16)] == [1.0, 0.5, 0.5]   # ... and its floor
    assert [float(_scale_at(t, kind="step", step_size=2, gamma=0.5, min_scale=0.125)) for t in range(9)] == [1, 1, .5, .5, .25, .25, .125, .125, .125]
    assert [float(_scale_at(t, kind="cosine", total_steps=4)) for t in (0, 2, 4, 5)] == [1.0, 0.5, 0.0, 0.0]
    assert all(float(_scale_at(t, kind="constant", warmup_steps=2, warmup_start=1.0)) == 1.0 for t in range(5))


@pytest.mark.parametrize("defect", ul.DEFECTS)
def test_the_grid_tells_every_planted_defect_from_the_true_twin(defect):
    """On the (kind, W, T, m) grid of the GPU test - every kind, its three (W, T), both floors, T + 4 steps - each wrong schedule
    differs from the true one by more than the bar somewhere; so does it on the grid run against torch."""
    for grid, extra in ((ul.GPU_GRID, 4), (ul.HOST_GRID, 5)):
        worst, where = 0.0, None
        for kw in _configs(grid):
            for t in range(kw["total_steps"] + extra):
                good, bad = float(ul.twin(t, **kw)), float(ul.twin(t, defect=defect, **kw))
                miss = abs(bad - good) / max(abs(good), 1e-3)
                if miss > worst:
                    worst, where = miss, (kw, t)
        assert worst > 1e-2 >= 1e4 * REL, (defect, worst, where)


# ------------------------------------------------------------------------------------------- C ABI
def test_header_compiles_as_c_and_the_layouts_hold(lib, tmp_path):
    from lstc_vad_amd import _lib
    from lstc_vad_amd._lib import AdagradItem, AdamItem, EmaItem, LrSchedule
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lstc_hip.h"', 'int main(void) {',
             '(void)sizeof(lstc_lr_schedule((const LstcLrSchedule*)0, (int32_t*)0, (float*)0, (void*)0));',   # declared (unevaluated: nothing is linked)
             '(void)sizeof(lstc_adagrad_multi_scaled((const LstcAdagradItem*)0, (int32_t)0, (const float*)0, (void*)0));',
             'printf("kinds %d %d %d %d %d\\n", LSTC_LR_CONSTANT, LSTC_LR_LINEAR, LSTC_LR_COSINE, LSTC_LR_STEP, LSTC_LR_INV_SQRT);',
             'printf("version %d\\n", LSTC_VERSION);']
    for name in ("LstcLrSchedule", "LstcAdagradItem", "LstcAdamItem", "LstcEmaItem", "LstcLossDesc"):
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
    for fname, _ in LrSchedule._fields_:
        lines.append(f'printf("LstcLrSchedule.{fname} %zu %zu\\n", offsetof(LstcLrSchedule, {fname}), sizeof(((LstcLrSchedule*)0)->{fname}));')
    lines += ['return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert int(got["LstcLrSchedule"][0]) == C.sizeof(LrSchedule) == 28
    assert int(got["LstcAdagradItem"][0]) == C.sizeof(AdagradItem) == 48
    assert int(got["LstcAdamItem"][0]) == C.sizeof(AdamItem) == 88
    assert int(got["LstcEmaItem"][0]) == C.sizeof(EmaItem) == 40
    assert int(got["LstcLossDesc"][0]) == C.sizeof(_lib.LossDesc)
    assert int(got["version"][0]) == 112 == lib.lstc_version()
    assert [int(x) for x in got["kinds"]] == [0, 1, 2, 3, 4] == [_lib.LR_CONSTANT, _lib.LR_LINEAR, _lib.LR_COSINE, _lib.LR_STEP, _lib.LR_INV_SQRT]
    for fname, ctype in LrSchedule._fields_:
        off, size = (int(x) for x in got[f"LstcLrSchedule.{fname}"])
        assert off == getattr(LrSchedule, fname).offset and size == C.sizeof(ctype), fname
    assert [f for f, _ in LrSchedule._fields_] == ["kind", "warmup_steps", "total_steps", "step_size", "warmup_start", "min_scale", "gamma"]
    for call in ("lstc_lr_schedule", "lstc_adagrad_multi_scaled"):
        assert call in _lib.EXPORTS and callable(getattr(lib, call))
    assert "lstc_lr_schedule" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _sched(**kw):
    from lstc_vad_amd._lib import LrSchedule
    f = dict(kind=1, warmup_steps=2, total_steps=10, step_size=0, warmup_start=0.0, min_scale=0.0, gamma=0.1)
    f.update(kw)
    return LrSchedule(**f)


def test_lr_schedule_checks_its_arguments_before_any_launch(lib):
    """No call here passes its checks: nothing is launched and the pointers are never used."""
    inf, nan = float("inf"), float("nan")
    call = lambda s, step=4096, scale=8192: lib.lstc_lr_schedule(C.byref(s) if s is not None else None, step, scale, None)
    assert call(None) == E_NULL and call(_sched(), step=None) == E_NULL and call(_sched(), scale=None) == E_NULL
    for kind in (-1, 5, 100):
        assert call(_sched(kind=kind)) == E_SHAPE, kind
    for kind in range(5):
        assert call(_sched(kind=kind, warmup_steps=-1, total_steps=10, step_size=1)) == E_SHAPE, kind
    for kind in (1, 2):
        for W, T in ((0, 0), (2, 2), (3, 2), (0, -1)):
            assert call(_sched(kind=kind, warmup_steps=W, total_steps=T)) == E_SHAPE, (kind, W, T)
    for size in (0, -1):
        assert call(_sched(kind=3, step_size=size, gamma=0.5)) == E_SHAPE, size
    for kind in range(5):
        for field in ("warmup_start", "min_scale"):
            for bad in (-0.001, 1.001, nan, inf, -inf):
                assert call(_sched(kind=kind, step_size=1, gamma=0.5, **{field: bad})) == E_RANGE, (kind, field, bad)
    for bad in (0.0, -0.5, 1.001, nan, inf):
        assert call(_sched(kind=3, step_size=1, gamma=bad)) == E_RANGE, bad
    # a shape error is reported ahead of a range error, a NULL ahead of both
    assert call(_sched(kind=9, min_scale=2.0)) == E_SHAPE and call(_sched(kind=9, min_scale=2.0), step=None) == E_NULL


def test_adagrad_multi_scaled_checks_its_arguments_before_any_launch(lib):
    from lstc_vad_amd._lib import AdagradItem
    ok = lambda: AdagradItem(w=4096, grad=8192, state=12288, n=8, lr=0.1, weight_decay=0.0, eps=1e-10, grad_scale=1.0)
    arr = lambda *items: (AdagradItem * len(items))(*items)
    assert lib.lstc_adagrad_multi_scaled(arr(ok()), 1, None, None) == E_NULL                 # no scale word
    assert lib.lstc_adagrad_multi_scaled(None, 1, 16384, None) == E_NULL
    assert lib.lstc_adagrad_multi_scaled(arr(ok()), 0, 16384, None) == E_SHAPE
    for f in ("w", "grad", "state"):
        bad = ok()
        setattr(bad, f, None)
        assert lib.lstc_adagrad_multi_scaled(arr(ok(), bad), 2, 16384, None) == E_NULL, f
    bad = ok()
    bad.n = 0
    assert lib.lstc_adagrad_multi_scaled(arr(ok(), bad), 2, 16384, None) == E_SHAPE
    assert lib.lstc_adagrad_multi_scaled(arr(*[ok() for _ in range(49)], bad), 50, 16384, None) == E_SHAPE   # past the first launch's 48


# ------------------------------------------------------------------------------------------- optim.LRSchedule on CPU tensors
def _cpu_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3, 7), (5,), (2, 2, 3))]


def test_lrschedule_refuses_what_the_kernel_refuses():
    from lstc_vad_amd import optim
    nan, inf = float("nan"), float("inf")
    bad = [dict(kind="exponential"), dict(kind="constant", warmup_steps=-1), dict(kind="linear"), dict(kind="cosine", total_steps=0),
           dict(kind="linear", warmup_steps=5, total_steps=5), dict(kind="cosine", warmup_steps=6, total_steps=5),
           dict(kind="step"), dict(kind="step", step_size=0, gamma=0.5), dict(kind="step", step_size=2, gamma=0.0),
           dict(kind="step", step_size=2, gamma=1.5), dict(kind="step", step_size=2, gamma=nan),
           dict(kind="constant", warmup_steps=2.5), dict(kind="constant", warmup_steps=2 ** 31)]
    for field in ("min_scale", "warmup_start"):
        bad += [dict(kind="constant", **{field: x}) for x in (-0.1, 1.5, nan, inf)]
    for kw in bad:
        with pytest.raises(ValueError):
            optim.LRSchedule(optim.Adagrad(_cpu_params(), lr=1e-2), **kw)
        with pytest.raises(ValueError):
            optim.LRSchedule.scale_at(0, **kw)
    with pytest.raises(TypeError):
        optim.LRSchedule(torch.optim.SGD(_cpu_params(), lr=0.1), "constant")
    # what it accepts, and what it keeps: the kernel's fields (f32 numbers, 0 for an integer the kind ignores)
    s = optim.LRSchedule(optim.AdamW(_cpu_params()), "step", warmup_steps=3, step_size=4, gamma=0.1, min_scale=0.01)
    assert s.config == dict(kind="step", warmup_steps=3, total_steps=0, step_size=4, min_scale=ul.f32(0.01), warmup_start=0.0, gamma=ul.f32(0.1))
    assert (s._desc.kind, s._desc.warmup_steps, s._desc.step_size, s._desc.gamma) == (3, 3, 4, ul.f32(0.1))
    assert optim.LRSchedule(optim.Adam(_cpu_params()), "constant", gamma=7.0).config["gamma"] == 7.0          # read by "step" only


@pytest.mark.parametrize("name", ["Adagrad", "Adam", "AdamW"])
def test_lrschedule_state_dict_host_count_and_last_lr(name):
    from lstc_vad_amd import optim
    ps = _cpu_params()
    groups = [{"params": ps[:2], "lr": 0.5}, {"params": ps[2:], "lr": 2.0}]
    opt = getattr(optim, name)(groups)
    if name == "Adagrad":
        assert opt._lr_scale is None                                        # nothing allocated without a schedule
    kw = dict(kind="linear", warmup_steps=2, total_steps=6, min_scale=0.25, warmup_start=0.5)
    s = optim.LRSchedule(opt, **kw)
    assert s._scale is opt._lr_scale and s._scale.dtype == torch.float32 and float(s._scale) == 1.0
    assert s._step.dtype == torch.int32 and int(s._step) == 0 == s.host_step()
    assert s.get_last_lr() == [0.25, 1.0]                                   # before the first step: the rates of step 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.step()
    assert s.host_step() == 0 and int(s._step) == 0
    sd = s.state_dict()
    assert sd == dict(kind="linear", warmup_steps=2, total_steps=6, step_size=0, min_scale=0.25, warmup_start=0.5, gamma=ul.f32(0.1), step=0)
    other = optim.LRSchedule(getattr(optim, name)(_cpu_params(1)), **kw)
    other.load_state_dict(dict(sd, step=5))
    assert other.host_step() == 5 == int(other._step) and other.state_dict()["step"] == 5
    assert other.get_last_lr() == [float(other.scale(4)) * g["lr"] for g in other.optimizer.param_groups]
    assert float(other.scale(4)) == float(ul.twin(4, **kw)) == 0.625
    other.set_host_step(7)
    assert other.host_step() == 7 and int(other._step) == 5                 # the host's mirror alone
    for change in (dict(kind="cosine"), dict(warmup_steps=3), dict(total_steps=7), dict(min_scale=0.5), dict(warmup_start=0.0)):
        with pytest.raises(ValueError):
            other.load_state_dict(dict(sd, **change))
    for n in (-1, 2 ** 31):
        with pytest.raises(ValueError):
            other.load_state_dict(dict(sd, step=n))
    with pytest.raises(ValueError):
        other.load_state_dict(dict(sd, bogus=1))
    assert other.host_step() == 7 and int(other._step) == 5                 # a refused dict changes nothing


class _Stub:
    """Stands in for the loaded library: counts the calls by name and launches nothing."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append(name)
            return 0
        return call


def _tiny_trainstep(**kw):
    from lstc_vad_amd.engine import TrainStep
    from lstc_vad_amd.models import Classifier, Encoder
    enc = Encoder(n_layers=1, n_head=2, d_k=4, d_v=4, d_model=8, d_inner=16, weight_init=False)
    args = Namespace(batch_size=1, part_num=2, part_len=1, n_patch=4, lambda_1=0.01, lambda_MIL=1.0, lambda_CE=0.8, temporal_only=False,
                     clip_grad=False)
    return TrainStep(args, "LTN", enc, Classifier(8, 0.0), 1e-4, 1e-2, 1e-3, fuse_qkv="off", **kw)


def test_no_schedule_allocates_nothing_and_adagrad_keeps_its_entry_point(monkeypatch):
    import inspect
    from lstc_vad_amd import engine, optim
    sig = inspect.signature(engine.TrainStep.__init__).parameters
    assert sig["lr_schedule"].default is None
    monkeypatch.setattr(optim, "stream_ptr", lambda: 0)
    monkeypatch.setattr(optim, "dev_ptr", lambda t: 4096)
    item = [(4096, 8192, 12288, 8, 0.1, 0.0, 1e-10, 1.0)]
    ts = _tiny_trainstep()
    assert ts.schedule is None and ts.optimizer._lr_scale is None
    stub = _Stub()
    ts.optimizer._launch(stub, item)
    assert stub.calls == ["lstc_adagrad_multi"]
    ts = _tiny_trainstep(lr_schedule=dict(kind="cosine", warmup_steps=1, total_steps=3))
    assert isinstance(ts.schedule, optim.LRSchedule) and ts.schedule.optimizer is ts.optimizer
    assert ts.schedule._scale is ts.optimizer._lr_scale and ts.optimizer._lr_scale is not None
    stub = _Stub()
    ts.optimizer._launch(stub, item)
    assert stub.calls == ["lstc_adagrad_multi_scaled"]
    for name in ("adam", "adamw"):
        ts = _tiny_trainstep(optimizer=name, lr_schedule=dict(kind="inv_sqrt", warmup_steps=4))
        assert ts.schedule._scale is ts.optimizer._lr_scale
    with pytest.raises(ValueError):
        _tiny_trainstep(lr_schedule=dict(kind="linear"))
    # attached after construction (the command line learns the run's length from the feed it builds behind the TrainStep)
    ts = _tiny_trainstep()
    assert ts.set_lr_schedule(None) is None and ts.schedule is None and ts.optimizer._lr_scale is None
    sched = ts.set_lr_schedule(dict(kind="linear", total_steps=5))
    assert sched is ts.schedule and isinstance(sched, optim.LRSchedule) and sched._scale is ts.optimizer._lr_scale
    with pytest.raises(RuntimeError):
        ts.set_lr_schedule(dict(kind="constant"))


# ------------------------------------------------------------------------------------------- the command line
@pytest.mark.parametrize("script", TRAIN_SCRIPTS)
def test_schedule_flags_parse_on_every_training_script(script):
    from lstc_vad_amd import cli
    a = cli.build_parser(script).parse_args([])
    assert (a.lr_schedule, a.lr_warmup_steps, a.lr_warmup_start, a.lr_total_steps, a.lr_min_scale, a.lr_step_size, a.lr_gamma) == \
        ("none", 0, 0.0, 0, 0.0, None, None)
    assert cli.lr_schedule_kw(a, 3, [0] * 10) is None
    a = cli.build_parser(script).parse_args("--lr_schedule cosine --lr_warmup_steps 5 --lr_warmup_start 0.1 --lr_total_steps 40 "
                                            "--lr_min_scale 0.05".split())
    assert cli.lr_schedule_kw(a, 3, [0] * 10) == dict(kind="cosine", warmup_steps=5, total_steps=40, min_scale=0.05, warmup_start=0.1)
    a = cli.build_parser(script).parse_args("--lr_schedule step --lr_step_size 7 --lr_gamma 0.5".split())
    assert cli.lr_schedule_kw(a, 3, [0] * 10) == dict(kind="step", warmup_steps=0, total_steps=None, min_scale=0.0, warmup_start=0.0,
                                                      step_size=7, gamma=0.5)
    with pytest.raises(SystemExit):
        cli.build_parser(script).parse_args(["--lr_schedule", "exponential"])


def test_a_decay_takes_the_runs_own_length_and_never_guesses_it():
    from lstc_vad_amd import cli
    from lstc_vad_amd.optim import LRSchedule
    parse = lambda text: cli.build_parser("temporal_transformer_shanghaitech").parse_args(text.split())

    class NoLength:                      # a feed that can be iterated but cannot tell how many batches an epoch has
        def __iter__(self):
            return iter(())
    for kind in ("linear", "cosine"):
        assert cli.lr_schedule_kw(parse(f"--lr_schedule {kind} --steps 12"), 3, NoLength())["total_steps"] == 12       # --steps given
        assert cli.lr_schedule_kw(parse(f"--lr_schedule {kind}"), 3, [0] * 10)["total_steps"] == 30                    # epochs x batches
        assert cli.lr_schedule_kw(parse(f"--lr_schedule {kind} --lr_total_steps 50 --steps 12"), 3, NoLength())["total_steps"] == 50
        with pytest.raises(SystemExit, match="cannot tell how many batches"):
            cli.lr_schedule_kw(parse(f"--lr_schedule {kind}"), 3, NoLength())
    # the kinds that need no length ask for none
    for kind in ("constant", "inv_sqrt"):
        kw = cli.lr_schedule_kw(parse(f"--lr_schedule {kind} --lr_warmup_steps 3"), 3, NoLength())
        assert kw["total_steps"] is None and LRSchedule._checked(**kw)["warmup_steps"] == 3
    with pytest.raises(SystemExit, match="--lr_step_size"):
        cli.lr_schedule_kw(parse("--lr_schedule step"), 3, NoLength())
