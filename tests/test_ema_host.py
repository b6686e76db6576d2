"""EMA weights, the part that needs no GPU: ``LstcEmaItem`` / ``LstcSwapItem`` against the C compiler's layout, the refusals
``lstc_ema_multi`` and ``lstc_swap_multi`` make before any launch, ``optim.EMA``'s argument checks and the command-line flags, and
the reference twin of tests/util_ema.py: against torch's own EMA definition, and - on the GPU test's exact inputs - that the
float32 restatement sits inside the bars while four planted defects do not."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import util_ema as ue

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
def test_item_layouts_match_header(lib, tmp_path):
    from lstc_vad_amd._lib import EmaItem, SwapItem
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lstc_hip.h"', 'int main(void) {',
             '(void)sizeof(lstc_ema_multi((const LstcEmaItem*)0, (int32_t)0, (void*)0));',           # declared (unevaluated: nothing is linked)
             '(void)sizeof(lstc_swap_multi((const LstcSwapItem*)0, (int32_t)0, (void*)0));',
             'printf("LstcEmaItem %zu\\n", sizeof(LstcEmaItem));', 'printf("LstcSwapItem %zu\\n", sizeof(LstcSwapItem));']
    for name, cls in (("LstcEmaItem", EmaItem), ("LstcSwapItem", SwapItem)):
        for fname, _ in cls._fields_:
            lines.append(f'printf("{name}.{fname} %zu %zu\\n", offsetof({name}, {fname}), sizeof((({name}*)0)->{fname}));')
    lines += ['return 0; }']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {l.split()[0]: l.split()[1:] for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert int(got["LstcEmaItem"][0]) == C.sizeof(EmaItem) == 40
    assert int(got["LstcSwapItem"][0]) == C.sizeof(SwapItem) == 24
    for name, cls in (("LstcEmaItem", EmaItem), ("LstcSwapItem", SwapItem)):
        for fname, ctype in cls._fields_:
            off, size = (int(x) for x in got[f"{name}.{fname}"])
            assert off == getattr(cls, fname).offset and size == C.sizeof(ctype), (name, fname)
    assert [f for f, _ in EmaItem._fields_] == ["avg", "w", "n", "count", "decay", "warmup"]
    assert [f for f, _ in SwapItem._fields_] == ["a", "b", "n"]


def test_header_declares_and_library_exports_both_calls(lib):
    from lstc_vad_amd import _lib
    header = open(os.path.join(ROOT, "include", "lstc_hip.h")).read()
    for call, item in (("lstc_ema_multi", "LstcEmaItem"), ("lstc_swap_multi", "LstcSwapItem")):
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+%s\s*\*\s*items\s*,\s*int32_t\s+count\s*,\s*void\s*\*\s*stream\s*\)\s*;" % (call, item), header)
        assert call in _lib.EXPORTS and callable(getattr(lib, call))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {"lstc_ema_multi", "lstc_swap_multi"} <= {l.split()[-1] for l in nm.splitlines()}


def _item(**kw):
    """An item that passes every host check; the pointers are never dereferenced on the host and no call below launches."""
    from lstc_vad_amd._lib import EmaItem
    f = dict(avg=4096, w=8192, n=100, count=20480, decay=0.999, warmup=0)
    f.update(kw)
    return EmaItem(**f)


def _call(lib, *items, count=None):
    from lstc_vad_amd._lib import EmaItem
    arr = (EmaItem * max(len(items), 1))(*items)
    return lib.lstc_ema_multi(arr, len(items) if count is None else count, None)


def test_ema_multi_checks_its_arguments_before_any_launch(lib):
    inf, nan = float("inf"), float("nan")
    assert lib.lstc_ema_multi(None, 1, None) == E_SHAPE
    assert lib.lstc_ema_multi(None, 0, None) == 0                        # nothing to do
    assert _call(lib, _item(), count=0) == 0
    assert _call(lib, _item(), count=-1) == E_SHAPE
    for f in ("avg", "w", "count"):
        assert _call(lib, _item(**{f: None})) == E_SHAPE, f
    assert _call(lib, _item(n=-1)) == E_SHAPE
    assert _call(lib, _item(), _item()) == E_SHAPE                       # two items, one word
    assert _call(lib, _item(), _item(count=20484), _item(n=0)) == E_SHAPE  # ... an empty item's word counts too
    assert _call(lib, _item(w=4096)) == E_SHAPE                          # the average of a weight is not the weight
    for bad in (-0.1, 1.0, 1.5, nan, inf, -inf):
        assert _call(lib, _item(decay=bad)) == E_RANGE, bad
    for bad in (2, -1):
        assert _call(lib, _item(warmup=bad)) == E_RANGE, bad
    # the bad item may sit anywhere in the list, also past the first launch's 48
    good = [_item(count=20480 + 4 * i) for i in range(50)]
    assert _call(lib, *good[:49], _item(count=40960, decay=1.0)) == E_RANGE
    assert _call(lib, *good[:49], _item(count=20480)) == E_SHAPE
    # a shape error is reported ahead of a range error of the same item
    assert _call(lib, _item(w=None, decay=2.0)) == E_SHAPE


def test_swap_multi_checks_its_arguments_before_any_launch(lib):
    from lstc_vad_amd._lib import SwapItem

    def call(*items, count=None):
        arr = (SwapItem * max(len(items), 1))(*items)
        return lib.lstc_swap_multi(arr, len(items) if count is None else count, None)
    ok = SwapItem(a=4096, b=8192, n=100)
    assert lib.lstc_swap_multi(None, 1, None) == E_SHAPE
    assert lib.lstc_swap_multi(None, 0, None) == 0
    assert call(ok, count=0) == 0
    assert call(ok, count=-1) == E_SHAPE
    assert call(SwapItem(a=None, b=8192, n=100)) == E_SHAPE and call(SwapItem(a=4096, b=None, n=100)) == E_SHAPE
    assert call(SwapItem(a=4096, b=8192, n=-1)) == E_SHAPE
    assert call(SwapItem(a=4096, b=4096, n=1)) == E_SHAPE
    assert call(*[ok] * 49, SwapItem(a=4096, b=4096, n=1)) == E_SHAPE      # past the first launch's 48: still before any launch


# ------------------------------------------------------------------------------------------- host-only Python
def _cpu_params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((3, 7), (5,), (2, 2, 3))]


def test_ema_checks_decay_and_warmup_and_has_no_cpu_path():
    from lstc_vad_amd.optim import EMA
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), 1.0 - 1e-9):           # the last one IS 1 as a float32
        with pytest.raises(ValueError):
            EMA(_cpu_params(), decay=bad)
    with pytest.raises(ValueError):
        EMA(_cpu_params(), warmup=2)
    ps = _cpu_params()
    e = EMA([{"params": ps[:2]}, {"params": ps[2:]}])
    assert (e.decay, e.warmup) == (0.999, False) and e.params == ps
    assert all(torch.equal(e.state[p]["avg"], p) and e.state[p]["avg"].data_ptr() != p.data_ptr() for p in ps)
    words = e.state[ps[0]]["count"]._base
    assert words is not None and words.dtype == torch.int32 and all(e.state[p]["count"]._base is words for p in ps)   # views of ONE tensor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e.update()
    sd = e.state_dict()
    assert sd["counts"] == [0, 0, 0] and (sd["decay"], sd["warmup"]) == (0.999, False) and len(sd["avg"]) == 3
    with pytest.raises(ValueError):
        EMA(ps[:2]).load_state_dict(sd)                                           # another number of parameters
    with pytest.raises(ValueError):
        EMA([ps[0], ps[2], ps[1]]).load_state_dict(sd)                            # other shapes
    f = EMA(_cpu_params(1), decay=0.5, warmup=True)
    f.load_state_dict(dict(sd, counts=[4, 5, 6]))
    assert (f.decay, f.warmup) == (0.999, False) and [f.host_count(p) for p in f.params] == [4, 5, 6]
    assert [int(f.state[p]["count"]) for p in f.params] == [4, 5, 6]
    assert all(torch.equal(f.state[q]["avg"], p) for p, q in zip(ps, f.params))


def test_trainstep_takes_ema_decay_and_defaults_to_none():
    import inspect
    from lstc_vad_amd.engine import TrainStep
    sig = inspect.signature(TrainStep.__init__).parameters
    assert sig["ema_decay"].default is None and sig["ema_warmup"].default is False


@pytest.mark.parametrize("script", TRAIN_SCRIPTS)
def test_ema_flags_parse_on_every_training_script(script):
    from lstc_vad_amd import cli
    a = cli.build_parser(script).parse_args([])
    assert (a.ema_decay, a.ema_warmup) == (0.0, False)
    a = cli.build_parser(script).parse_args("--ema_decay 0.99 --ema_warmup".split())
    assert (a.ema_decay, a.ema_warmup) == (0.99, True)
    for bad in ("1.0", "-0.5", "nan"):
        with pytest.raises(SystemExit):
            cli.build_parser(script).parse_args(["--ema_decay", bad])


# ------------------------------------------------------------------------------------------- the reference twin
def test_float32_reference_is_torchs_own_ema_within_the_bar():
    """Five updates of a small CPU model with decay 0.999, no warm-up: util_ema.ema_step in float32, from torch's own average in
    front of each update, against ``AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.999))`` within the bar."""
    swa = torch.optim.swa_utils
    if not hasattr(swa, "get_ema_multi_avg_fn"):
        pytest.skip("this torch has no torch.optim.swa_utils.get_ema_multi_avg_fn")
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    theirs = swa.AveragedModel(model, multi_avg_fn=swa.get_ema_multi_avg_fn(0.999))
    g = torch.Generator().manual_seed(1)
    for t in range(1, 6):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=g))
        before = [p.detach().clone() for p in theirs.module.parameters()]
        theirs.update_parameters(model)
        for b, p, q in zip(before, model.parameters(), theirs.module.parameters()):
            ref, bar = ue.bar(b, p.detach(), t, 0.999, False)
            ours = ue.ema_step(b, p.detach(), t, 0.999, False, dtype=ue.F32)
            assert float((ours.double() - q.detach().double()).abs().max()) <= bar, t
            assert float((q.detach().double() - ref).abs().max()) <= bar, t
            if t == 1:
                assert torch.equal(ours, q.detach())


@pytest.fixture(scope="module")
def gpu_case():
    items = ue.gpu_items()
    avg0, offs = ue.first_average(items)
    return items, avg0, offs


def _chain(items, avg0, offs, min_n=0):
    """Per item: (the average in front of update t, the weights of update t) for t = 1 .. 12 - update 1 from the GPU test's
    inputs, the later ones from the float32 restatement of the update before (the GPU test takes them from the device; they
    differ by rounding only)."""
    ws = {t: ue.weights(items, t) for t in ue.UPDATES}
    for i, (it, o) in enumerate(zip(items, offs)):
        if it.n == 0 or it.n < min_n:
            continue
        avg = avg0[o:o + it.n].clone()
        for t in ue.UPDATES:
            w_arena, offs_w = ws[t]
            w = w_arena[offs_w[i]:offs_w[i] + it.n]
            yield i, it, t, avg, w
            avg = ue.ema_step(avg, w, t, ue.DECAY, it.warmup, dtype=ue.F32)


def test_float32_restatement_stays_within_one_bar(gpu_case):
    items, avg0, offs = gpu_case
    assert len(items) == 60 and items[ue.EMPTY_AT].n == 0 and items[ue.UNALIGNED_AT].misaligned
    offs_w = ue.layout(items, misalign=True)[0]
    assert offs_w[ue.UNALIGNED_AT] % 4 == 1 and all(o % 4 == 0 for i, o in enumerate(offs_w) if i != ue.UNALIGNED_AT)
    assert all(o % 4 == 0 for o in offs)
    assert {it.n for it in items} >= {1, 3, 4, 5, 8191, 8192, 8193, 21, 7, 44}
    assert {it.warmup for it in items} == {0, 1} and items[ue.ALIGNED_TWIN_AT][:2] == items[ue.UNALIGNED_AT][:2]
    # the ramp crosses the decay exactly: either arm of the min is the same number
    assert (1.0 + 8) / (10.0 + 8) == ue.DECAY == ue.f32(ue.DECAY) and ue.ema_a(9, ue.DECAY, 1) == ue.ema_a(9, ue.DECAY, 0) == 0.5
    assert ue.ema_a(8, ue.DECAY, 1) > 0.5 and ue.ema_a(12, ue.DECAY, 1) == 0.5
    for i, it, t, avg, w in _chain(items, avg0, offs):
        ref, bar = ue.bar(avg, w, t, ue.DECAY, it.warmup)
        r32 = ue.ema_step(avg, w, t, ue.DECAY, it.warmup, dtype=ue.F32)
        assert torch.isfinite(ref).all() and bar > 0
        assert float((r32.double() - ref).abs().max()) <= bar, (i, t)
        if t > 1 and it.n >= 1000:
            assert float((avg.double() - w.double()).abs().mean()) > 0.3            # the average is an order of 1 away from the weight


@pytest.mark.parametrize("defect", ue.DEFECTS)
def test_planted_defects_land_beyond_four_bars(gpu_case, defect):
    """Each wrong formula misses at least one item at at least one update by more than FOUR bars: the bars of the GPU test are
    tight enough to tell the update they pin from its usual mistakes.  (With decay 0.5 the last three are visible on the ramp of
    the warmed-up items only: on the plateau a = decay = 0.5 whatever u is.)"""
    items, avg0, offs = gpu_case
    worst, where = 0.0, None
    for i, it, t, avg, w in _chain(items, avg0, offs, min_n=1000):
        ref, bar = ue.bar(avg, w, t, ue.DECAY, it.warmup)
        miss = float((ue.ema_step(avg, w, t, ue.DECAY, it.warmup, defect=defect) - ref).abs().max()) / bar
        if miss > worst:
            worst, where = miss, (i, t)
    assert worst > 4.0, (worst, where)
    if defect == "first_update_blends":
        assert where[1] == 1


def test_integer_family_is_exactly_representable():
    """The family the GPU test requires to EQUAL float64: three updates in float32 are the three updates in float64."""
    avg, ws = ue.int_family()
    a64, a32 = avg.double(), avg.clone()
    for t, w in enumerate(ws, 1):
        a64 = ue.ema_step(a64, w, t, 0.5, False)
        a32 = ue.ema_step(a32, w, t, 0.5, False, dtype=ue.F32)
        assert torch.equal(a32.double(), a64), t
    assert len(torch.unique(a64)) > 50 and not torch.equal(a64, ws[-1].double())      # neither degenerate nor a copy
