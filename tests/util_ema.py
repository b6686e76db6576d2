"""What the EMA tests share (tests/test_ema_host.py, tests/test_ema_gpu.py): the float64 reference of ONE update of
``lstc_ema_multi`` with its float32 restatement and the ``terms_abs`` of the project's tolerance rule (util_rowops.tol), the
planted defects the host test shows that rule to catch, and the item lists the GPU test runs - so that the host test proves its
claims on the GPU test's exact inputs.  No project kernel is called here.

One update, from the average in front of it (include/lstc_hip.h, lstc_ema_multi; the f32 decay widened to float64):

    t == 1:  avg = w                                                                (a bit copy)
    t >  1:  decay_t = warmup ? min(decay, (1 + u) / (10 + u)) : decay,  u = t - 1
             avg = avg + (1 - decay_t) * (w - avg)

The weights of a test CHANGE from update to update (``weights(t)``), as a training step would change them: with a fixed weight
the first update's copy would make every later update a no-op and no formula after it could be told from another.
"""
from collections import namedtuple

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
DEFECTS = ("first_update_blends", "u_is_t", "a_and_decay_swapped", "warmup_ignored")
DECAY = 0.5                                            # the ramp (1 + u) / (10 + u) crosses it exactly at u = 8: 9 / 18
UPDATES = tuple(range(1, 13))                          # the copy, the ramp up to its crossing (t = 9), three updates of the plateau


def f32(x):
    """The value the f32 field of LstcEmaItem holds for the Python number ``x``."""
    return float(np.float32(x))


def ema_a(t, decay, warmup, defect=None):
    """a = 1 - decay_t of update ``t`` (1-based, t > 1 unless the defect blends the first update too), in float64."""
    d = f32(decay)
    u = t if defect == "u_is_t" else t - 1
    if warmup and defect != "warmup_ignored":
        d = min(d, (1.0 + u) / (10.0 + u))
    return d if defect == "a_and_decay_swapped" else 1.0 - d


def ema_step(avg, w, t, decay, warmup, dtype=F64, defect=None):
    """The average after update ``t`` in ``dtype``: float64 is the reference, float32 the restatement of util_rowops.tol.
    ``defect``: one of DEFECTS, a wrong formula that the bars must refuse."""
    avg, w = avg.to(dtype), w.to(dtype)
    if t == 1 and defect != "first_update_blends":
        return w.clone()
    return avg + ema_a(t, decay, warmup, defect) * (w - avg)


def ema_terms(avg, w, t, decay, warmup):
    """terms_abs: |avg| + a (|w| + |avg|) in float64; the copy of the first update has the one term |w|."""
    avg, w = avg.to(F64), w.to(F64)
    if t == 1:
        return w.abs()
    return avg.abs() + ema_a(t, decay, warmup) * (w.abs() + avg.abs())


def bar(avg, w, t, decay, warmup):
    """(reference in float64, its bar) for one update from this average."""
    from util_rowops import tol
    ref = ema_step(avg, w, t, decay, warmup)
    return ref, tol(ref, ema_step(avg, w, t, decay, warmup, dtype=F32), ema_terms(avg, w, t, decay, warmup))


# ------------------------------------------------------------------------------------------- the GPU test's item lists
PER_WG = 8192                                          # elements one workgroup owns (csrc/rowops.hip, ADA_PER_WG)
# the sizes the issue names - one element each side of a workgroup slice, a 2-D weight, an empty item in the middle - then
# 7 + 37 i up to 60 items (two launches of 48 + 12)
NAMED_SIZES = (1, 3, 4, 5, PER_WG - 1, PER_WG, PER_WG + 1, 3 * 7)
EMPTY_AT, UNALIGNED_AT, ALIGNED_TWIN_AT = 20, 33, 34
N_ITEMS = 60
GUARD = 64          # NaN floats in front of, between and behind the items' regions

Item = namedtuple("Item", "n warmup misaligned")


def gpu_items():
    """The 60 items of the GPU test: decay 0.5 everywhere, the warm-up on every second item (the twin: as its misaligned item)."""
    sizes = list(NAMED_SIZES) + [7 + 37 * i for i in range(N_ITEMS - len(NAMED_SIZES))]
    sizes[EMPTY_AT] = 0
    sizes[UNALIGNED_AT] = sizes[ALIGNED_TWIN_AT] = PER_WG + 1
    return [Item(n, (UNALIGNED_AT if i == ALIGNED_TWIN_AT else i) % 2, i == UNALIGNED_AT) for i, n in enumerate(sizes)]


def layout(items, misalign):
    """(offset of every item in a flat float32 arena, arena length): regions start on 16-byte boundaries with GUARD floats
    between them; with ``misalign`` (the arena of the weights) the misaligned item starts one float (4 bytes) past one."""
    offs, at = [], GUARD
    for it in items:
        offs.append(at + (1 if it.misaligned and misalign else 0))
        at = (offs[-1] + it.n + GUARD + 3) // 4 * 4
    return offs, at


def _fill(items, offs, total, seed, like=None, shift=1.0):
    """|x| in [0.5, 1.5] with random signs (``like`` given: that arena's values plus a normal deviate of size ``shift``); NaN
    outside the items' regions; the aligned twin holds the misaligned item's values."""
    g = torch.Generator().manual_seed(seed)
    arena = torch.full((total,), float("nan"), dtype=F32)
    for i, (it, o) in enumerate(zip(items, offs)):
        if i == ALIGNED_TWIN_AT:
            src = offs[UNALIGNED_AT]
            arena[o:o + it.n] = arena[src:src + it.n]
            continue
        sign = torch.randint(0, 2, (it.n,), generator=g).float() * 2 - 1
        x = sign * (0.5 + torch.rand(it.n, generator=g))
        if like is not None:
            arena_like, offs_like = like
            x = arena_like[offs_like[i]:offs_like[i] + it.n] + shift * torch.randn(it.n, generator=g)
        arena[o:o + it.n] = x
    return arena


def weights(items, t, seed=0):
    """(the weight arena in front of update ``t``, its offsets): |w| about 1, drawn afresh for every update."""
    offs, total = layout(items, misalign=True)
    return _fill(items, offs, total, 1000 * seed + t), offs


def first_average(items, seed=0):
    """(the average arena in front of update 1, its offsets): the first weights plus a normal deviate - what the first update
    must overwrite, not blend."""
    w, offs_w = weights(items, 1, seed)
    offs, total = layout(items, misalign=False)
    return _fill(items, offs, total, 1000 * seed + 500, like=(w, offs_w)), offs


def data_mask(items, offs, total):
    mask = torch.zeros(total, dtype=torch.bool)
    for it, o in zip(items, offs):
        mask[o:o + it.n] = True
    return mask


# ------------------------------------------------------------------------------------------- the integer-valued family
def int_family(n=PER_WG + 7, seed=3, updates=3):
    """(first average, the weights of updates 1 .. ``updates``): multiples of 8 below 2**10.  With decay 0.5 and no warm-up every
    difference, half and sum of three updates is an integer below 2**11 - a float32 number - so the kernel must EQUAL float64."""
    g = torch.Generator().manual_seed(seed)
    draw = lambda: 8.0 * torch.randint(-127, 128, (n,), generator=g).float()
    return draw(), [draw() for _ in range(updates)]
