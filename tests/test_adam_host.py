"""Adam / AdamW, the part that needs no GPU: ``LstcAdamItem`` against the C compiler's layout, the refusals ``lstc_adam_multi``
makes before any launch, the optimizers' surface on CPU tensors (state_dict interoperation with torch.optim, amsgrad, no CPU
fallback, the command-line flags), and the reference twin of tests/util_adam.py: against torch.optim in float64, and - on the
GPU test's exact inputs - that the float32 restatement sits inside the bars while five planted defects do not."""
import copy
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import util_adam as ua

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_SHAPE, E_RANGE = -2, -5
TRAIN_SCRIPTS = ("temporal_transformer_shanghaitech", "temporal_transformer_UCF", "temporal_transformer_UBnormal",
                 "spatio_transformer_shanghaitech", "spatio_transformer_UCF", "spatio_transformer_UBnormal", "spatio_transformer_MIL_CE")


@pytest.fixture(scope="module")
def lib():
    from lstc_vad_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------- C ABI
def test_adam_item_layout_matches_header(lib, tmp_path):
    from lstc_vad_amd._lib import AdagradItem, AdamItem
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lstc_hip.h"', 'int main(void) {',
             '(void)sizeof(lstc_adam_multi((const LstcAdamItem*)0, (int32_t)0, (void*)0));',          # declared (unevaluated: nothing is linked)
             'printf("LstcAdamItem %zu\\n", sizeof(LstcAdamItem));', 'printf("LstcAdagradItem %zu\\n", sizeof(LstcAdagradItem));',
             'printf("version %d\\n", LSTC_VERSION);']
    for fname, _ in AdamItem._fields_:
        lines.append(f'printf("LstcAdamItem.{fname} %zu %zu\\n", offsetof(LstcAdamItem, {fname}), sizeof(((LstcAdamItem*)0)->{fname}));')
    lines += ['return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert int(got["LstcAdamItem"][0]) == C.sizeof(AdamItem) == 88
    assert int(got["LstcAdagradItem"][0]) == C.sizeof(AdagradItem) == 48
    assert int(got["version"][0]) == 112 == lib.lstc_version()
    for fname, ctype in AdamItem._fields_:
        off, size = (int(x) for x in got[f"LstcAdamItem.{fname}"])
        assert off == getattr(AdamItem, fname).offset and size == C.sizeof(ctype), fname
    assert [f for f, _ in AdamItem._fields_] == ["w", "grad", "m", "v", "n", "step", "lr_scale", "lr", "beta1", "beta2", "eps",
                                                 "weight_decay", "grad_scale", "decoupled"]


def test_header_declares_and_library_exports_lstc_adam_multi(lib):
    from lstc_vad_amd import _lib
    header = open(os.path.join(ROOT, "include", "lstc_hip.h")).read()
    assert re.search(r"\bint\s+lstc_adam_multi\s*\(\s*const\s+LstcAdamItem\s*\*\s*items\s*,\s*int32_t\s+count\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert "#define LSTC_VERSION 112" in header
    assert "lstc_adam_multi" in _lib.EXPORTS and callable(lib.lstc_adam_multi)
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = {l.split()[-1] for l in nm.splitlines() if l.split()[-1].startswith("lstc_")}
    assert syms == set(_lib.EXPORTS), syms ^ set(_lib.EXPORTS)          # lstc_adam_multi is the one name this entry point adds


def _item(**kw):
    """An item that passes every host check; the pointers are never dereferenced on the host and no call below launches."""
    from lstc_vad_amd._lib import AdamItem
    f = dict(w=4096, grad=8192, m=12288, v=16384, n=100, step=20480, lr_scale=None, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8,
             weight_decay=0.01, grad_scale=1.0, decoupled=1)
    f.update(kw)
    return AdamItem(**f)


def _call(lib, *items, count=None):
    from lstc_vad_amd._lib import AdamItem
    arr = (AdamItem * max(len(items), 1))(*items)
    return lib.lstc_adam_multi(arr, len(items) if count is None else count, None)


def test_adam_multi_checks_its_arguments_before_any_launch(lib):
    inf, nan = float("inf"), float("nan")
    assert lib.lstc_adam_multi(None, 1, None) == E_SHAPE
    assert lib.lstc_adam_multi(None, 0, None) == 0                       # nothing to do
    assert _call(lib, _item(), count=-1) == E_SHAPE
    for f in ("w", "grad", "m", "v", "step"):
        assert _call(lib, _item(**{f: None})) == E_SHAPE, f
    assert _call(lib, _item(n=-1)) == E_SHAPE
    assert _call(lib, _item(), _item()) == E_SHAPE                       # two items, one step word
    assert _call(lib, _item(), _item(step=20484), _item(n=0)) == E_SHAPE   # ... an empty item's word counts too
    for f in ("beta1", "beta2"):
        for bad in (-0.1, 1.0, 1.5, nan, inf):
            assert _call(lib, _item(**{f: bad})) == E_RANGE, (f, bad)
    for f in ("eps", "lr", "weight_decay"):
        for bad in (-1e-3, nan, inf, -inf):
            assert _call(lib, _item(**{f: bad})) == E_RANGE, (f, bad)
    # the bad item may sit anywhere in the list, also past the first launch's 48
    good = [_item(step=20480 + 4 * i) for i in range(50)]
    assert _call(lib, *good[:49], _item(step=40960, lr=-1.0)) == E_RANGE
    assert _call(lib, *good[:49], _item(step=20480)) == E_SHAPE
    # a shape error is reported ahead of a range error of the same item
    assert _call(lib, _item(w=None, lr=-1.0)) == E_SHAPE


# ------------------------------------------------------------------------------------------- the Python optimizers on CPU tensors
def _cpu_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3, 7), (5,), (2, 2, 3))]


def _grads(params, k):
    g = torch.Generator().manual_seed(100 + k)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)


def _same_state(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert a["state"].keys() == b["state"].keys()
    for k in a["state"]:
        assert a["state"][k].keys() == b["state"][k].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for name in a["state"][k]:
            x, y = a["state"][k][name], b["state"][k][name]
            assert x.shape == y.shape and x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), (k, name, x, y)


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_state_dict_round_trips_with_torch_optim_in_both_directions(name):
    from lstc_vad_amd import optim
    ours_cls, torch_cls = getattr(optim, name), getattr(torch.optim, name)
    kw = dict(betas=(0.8, 0.95), eps=1e-6, weight_decay=0.05)
    pt = _cpu_params()
    groups = lambda ps: [{"params": ps[:2], "lr": 3e-3}, {"params": ps[2:], "lr": 1e-2}]
    t_opt = torch_cls(groups(pt), **kw)
    for k in range(3):
        _grads(pt, k)
        if k == 2:
            pt[1].grad = None                 # steps 3, 2, 3: every parameter keeps its own count
        t_opt.step()
    saved = copy.deepcopy(t_opt.state_dict())          # (torch's load_state_dict keeps the tensors it is given: no two optimizers may share them)
    # torch -> ours: keys, shapes, values and `step` come back out as torch wrote them
    po = _cpu_params()
    ours = ours_cls(groups(po), **kw)
    assert ours.state_dict()["state"] == {}                                   # nothing stepped yet: torch emits no state either
    assert ours.state_dict()["param_groups"] == torch_cls(groups(_cpu_params()), **kw).state_dict()["param_groups"]
    ours.load_state_dict(saved)
    _same_state(ours.state_dict(), saved)
    assert [int(ours.state[p]["step"]) for p in po] == [3, 2, 3] == [ours.host_step(p) for p in po]
    assert all(ours.state[p]["step"].dtype == torch.int32 and ours.state[p]["step"].dim() == 0 for p in po)
    words = ours.state[po[0]]["step"]._base
    assert words is not None and all(ours.state[p]["step"]._base is words for p in po)       # views of ONE tensor
    # ours -> torch: a fresh torch optimizer loaded from OUR dict continues exactly like the uninterrupted one
    pc = [torch.nn.Parameter(p.detach().clone()) for p in pt]
    cont = torch_cls(groups(pc), **kw)
    cont.load_state_dict(copy.deepcopy(ours.state_dict()))
    _grads(pt, 7), _grads(pc, 7)
    t_opt.step(), cont.step()
    for a, b in zip(pt, pc):
        assert torch.equal(a, b)
    _same_state(cont.state_dict(), t_opt.state_dict())
    # ours -> ours, and a dict without state (a fresh torch optimizer's) resets ours
    again = ours_cls(groups(_cpu_params()), **kw)
    again.load_state_dict(copy.deepcopy(ours.state_dict()))
    _same_state(again.state_dict(), saved)
    again.load_state_dict(torch_cls(groups(_cpu_params()), **kw).state_dict())
    assert again.state_dict()["state"] == {} and all(int(again.state[p]["step"]) == 0 for g in again.param_groups for p in g["params"])


def test_adam_state_loads_into_adamw_and_back():
    from lstc_vad_amd import optim
    pt = _cpu_params()
    t_opt = torch.optim.Adam(pt, lr=1e-2)
    _grads(pt, 0)
    t_opt.step()
    for cls in (optim.AdamW, optim.Adam):
        o = cls(_cpu_params(), lr=1e-2)
        o.load_state_dict(copy.deepcopy(t_opt.state_dict()))
        sd = o.state_dict()
        assert all(torch.equal(sd["state"][k]["exp_avg"], t_opt.state_dict()["state"][k]["exp_avg"]) and float(sd["state"][k]["step"]) == 1.0
                   for k in range(3))


def test_defaults_amsgrad_and_no_cpu_fallback():
    from lstc_vad_amd import optim
    a, w = optim.Adam(_cpu_params()), optim.AdamW(_cpu_params())
    for o, wd in ((a, 0), (w, 1e-2)):
        g = o.param_groups[0]
        assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (1e-3, (0.9, 0.999), 1e-8, wd)
    for cls in (optim.Adam, optim.AdamW):
        with pytest.raises(NotImplementedError):
            cls(_cpu_params(), amsgrad=True)
        with pytest.raises(ValueError):
            cls(_cpu_params(), betas=(1.0, 0.999))
        ps = _cpu_params()
        o = cls(ps)
        _grads(ps, 0)
        before = [p.detach().clone() for p in ps]
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            o.step()
        assert all(torch.equal(p, b) for p, b in zip(ps, before)) and all(o.host_step(p) == 0 for p in ps)
        assert o.state_dict()["state"] == {}
        o.set_lr_scale(0.25)
        assert float(o._lr_scale) == 0.25 and o._lr_scale.dtype == torch.float32


def test_adagrad_keeps_its_state_keys_and_surface():
    from lstc_vad_amd import optim
    ps = _cpu_params()
    o = optim.Adagrad(ps, lr=1e-2, weight_decay=1e-3)
    assert all(set(o.state[p]) == {"sum", "step"} and o.state[p]["step"] == 0 for p in ps)
    assert isinstance(o, torch.optim.Optimizer) and optim.Adagrad.__mro__[1] is optim.Adam.__mro__[1]      # one shared base
    assert "step" not in {k for k, f in vars(optim.Adagrad).items() if not getattr(f, "hooked", False)}
    _grads(ps, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        o.step()


def test_trainstep_rejects_unknown_optimizers():
    import inspect
    from lstc_vad_amd.engine import TrainStep
    names = list(inspect.signature(TrainStep.__init__).parameters)
    assert names[-2:] == ["optimizer", "optimizer_kw"] and names[1:8] == ["args", "mode", "encoder", "head", "lr_encoder", "lr_head", "weight_decay"]
    assert inspect.signature(TrainStep.__init__).parameters["optimizer"].default == "adagrad"


@pytest.mark.parametrize("script", TRAIN_SCRIPTS)
def test_optimizer_flags_parse_on_every_training_script(script):
    from lstc_vad_amd import cli
    a = cli.build_parser(script).parse_args([])
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_eps) == ("adagrad", 0.9, 0.999, 1e-8)
    a = cli.build_parser(script).parse_args("--optimizer adamw --adam_beta1 0.8 --adam_beta2 0.95 --adam_eps 1e-6".split())
    assert (a.optimizer, a.adam_beta1, a.adam_beta2, a.adam_eps) == ("adamw", 0.8, 0.95, 1e-6)
    assert cli.build_parser(script).parse_args(["--optimizer", "adam"]).optimizer == "adam"
    with pytest.raises(SystemExit):
        cli.build_parser(script).parse_args(["--optimizer", "sgd"])


def test_cli_flag_table_is_untouched():
    import json
    table = json.load(open(os.path.join(ROOT, "lstc_vad_amd", "cli_flags.json")))
    assert "--optimizer" not in json.dumps(table) and "--adam_beta1" not in json.dumps(table)


# ------------------------------------------------------------------------------------------- the reference twin
@pytest.mark.parametrize("name,decoupled", [("Adam", 0), ("AdamW", 1)])
def test_float64_reference_is_torch_optim_in_float64(name, decoupled):
    """Three steps of util_adam.adam_step (float64) against torch.optim.Adam / AdamW on float64 parameters, to 1e-12 relative.
    The hyper-parameters are float32 numbers, so that the widening inside adam_step changes nothing."""
    h = ua.Hyper(ua.f32(1e-2), ua.f32(0.9), ua.f32(0.999), ua.f32(1e-8), ua.f32(0.1), 1.0, decoupled)
    g = torch.Generator().manual_seed(1)
    w0 = torch.randn(1000, generator=g, dtype=torch.float64)
    p = torch.nn.Parameter(w0.clone())
    opt = getattr(torch.optim, name)([p], lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps, weight_decay=h.weight_decay)
    w, m, v = w0, torch.zeros_like(w0), torch.zeros_like(w0)
    for t in (1, 2, 3):
        grad = torch.randn(1000, generator=g, dtype=torch.float64)
        p.grad = grad.clone()
        opt.step()
        w, m, v = ua.adam_step(w, grad, m, v, t, h)
        st = opt.state[p]
        for ours, theirs in ((w, p.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert float(((ours - theirs).abs() / theirs.abs().clamp_min(1e-300)).max()) < 1e-12, t
        assert float(st["step"]) == t


@pytest.fixture(scope="module")
def gpu_case():
    items = ua.gpu_items()
    arenas, offs = ua.gpu_inputs(items)
    return items, arenas, offs


def _chain(items, arenas, offs):
    """Per item: the before-values of steps t = 1, 2, 3 - step 1 from the GPU test's inputs, the later ones from the float32
    restatement of the step before (the GPU test takes them from the device; they differ by rounding only)."""
    for i, (it, o) in enumerate(zip(items, offs)):
        if it.n == 0:
            continue
        w, grad, m, v = (a[o:o + it.n].clone() for a in arenas)
        for t in (1, 2, 3):
            yield i, it, t, (w, grad, m, v)
            w, m, v = ua.adam_step(w, grad, m, v, t, it.hyper, dtype=ua.F32)


def test_float32_restatement_stays_within_half_of_every_bar(gpu_case):
    items, arenas, offs = gpu_case
    assert len(items) == 60 and items[ua.EMPTY_AT].n == 0 and items[ua.UNALIGNED_AT].misaligned
    assert offs[ua.UNALIGNED_AT] % 4 == 1 and all(o % 4 == 0 for i, o in enumerate(offs) if i != ua.UNALIGNED_AT)
    assert {it.n for it in items} >= {1, 3, 4, 5, 8191, 8192, 8193, 21, 2048 * 513}
    assert {it.hyper.decoupled for it in items} == {0, 1}
    for i, it, t, before in _chain(items, arenas, offs):
        ref, bar = ua.bars(*before, t, it.hyper)
        r32 = ua.adam_step(*before, t, it.hyper, dtype=ua.F32)
        for name, r, x, b in zip("wmv", ref, r32, bar):
            assert torch.isfinite(r).all() and b > 0
            assert float((x.double() - r).abs().max()) <= 0.5 * b, (i, t, name)


@pytest.mark.parametrize("defect", ua.DEFECTS)
def test_planted_defects_land_beyond_four_bars(gpu_case, defect):
    """Each wrong formula misses at least one tensor of at least one item by more than FOUR bars at EVERY step t = 1, 2, 3: the bars
    of the GPU test are tight enough to tell the update they pin from its usual mistakes."""
    items, arenas, offs = gpu_case
    worst = {1: 0.0, 2: 0.0, 3: 0.0}
    for i, it, t, before in _chain(items, arenas, offs):
        if it.n < 1000:
            continue                       # the large items decide; the small ones only cost time here
        ref, bar = ua.bars(*before, t, it.hyper)
        bad = ua.adam_step(*before, t, it.hyper, defect=defect)
        for r, x, b in zip(ref, bad, bar):
            worst[t] = max(worst[t], float((x - r).abs().max()) / b)
    assert all(x > 4.0 for x in worst.values()), worst


@pytest.mark.parametrize("beta2", [0.5, 0.75])
@pytest.mark.parametrize("decoupled", [0, 1])
def test_integer_family_is_exactly_representable(beta2, decoupled):
    """The family the GPU test requires to EQUAL float64.  beta1 = beta2 = 0.5 at t = 1: every intermediate of m and v is a float32
    number, but 1 / sqrt(1 - beta2^t) = sqrt(2) is not, so w cannot be exact there; with beta2 = 0.75 the correction is 2 and the
    whole chain, w included, is exact."""
    w, grad, m, v, h = ua.int_family(beta2, decoupled)
    ex = ua.exact_chain(w, grad, m, v, h)
    need = {"1-b1", "1-b2", "step", "keep", "g", "g-m", "(1-b1)(g-m)", "m", "g*g", "(1-b2)g*g", "b2*v", "v", "step*m"}
    assert all(ex[k] for k in need), ex
    if beta2 == 0.75:
        assert all(ex.values()) and {"denominator", "quotient", "w"} <= set(ex), ex
    else:
        assert not ex["rsb2"] and "w" not in ex
    ref = ua.adam_step(w, grad, m, v, 1, h)
    r32 = ua.adam_step(w, grad, m, v, 1, h, dtype=ua.F32)
    assert torch.equal(r32[1].double(), ref[1]) and torch.equal(r32[2].double(), ref[2])
    assert len(torch.unique(ref[0])) > 50                      # not a degenerate family
