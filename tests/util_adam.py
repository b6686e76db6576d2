"""What the Adam / AdamW tests share (tests/test_adam_host.py, tests/test_adam_gpu.py): the float64 reference of ONE step of
``lstc_adam_multi`` with its float32 restatement and the ``terms_abs`` of the project's tolerance rule (util_rowops.tol), the
planted defects the host test shows that rule to catch, and the item lists the GPU test runs - so that the host test proves its
claims on the GPU test's exact inputs.  No project kernel is called here.

One step, from the state in front of it (include/lstc_hip.h, lstc_adam_multi; f32 scalars widened to float64):

    g = grad * grad_scale  [+ wd * w  when not decoupled]          [w *= 1 - lr_t * wd  when decoupled],  lr_t = lr * lr_scale
    m += (1 - b1) * (g - m)          v = b2 * v + (1 - b2) * g * g
    w -= (lr_t / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
"""
import math
from collections import namedtuple

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
DEFECTS = ("no_bias_correction", "t_off_by_one", "decoupled_as_l2", "eps_inside_sqrt", "grad_scale_on_decay")

Hyper = namedtuple("Hyper", "lr beta1 beta2 eps weight_decay grad_scale decoupled")


def f32(x):
    """The value an f32 field of LstcAdamItem holds for the Python number ``x``."""
    return float(np.float32(x))


def adam_step(w, grad, m, v, t, h: Hyper, lr_scale=1.0, dtype=F64, defect=None):
    """(w, m, v) after step ``t`` (1-based) in ``dtype``: float64 is the reference, float32 the restatement of util_rowops.tol.
    ``defect``: one of DEFECTS, a wrong formula that the bars must refuse."""
    w, grad, m, v = (x.to(dtype) for x in (w, grad, m, v))
    lr_t = f32(h.lr) * f32(lr_scale)
    b1, b2, eps, wd, gs = f32(h.beta1), f32(h.beta2), f32(h.eps), f32(h.weight_decay), f32(h.grad_scale)
    decoupled = bool(h.decoupled) and defect != "decoupled_as_l2"
    if defect == "t_off_by_one":
        t = t + 1
    g = grad * gs
    if not decoupled:
        g = (grad + wd * w) * gs if defect == "grad_scale_on_decay" else g + wd * w
    else:
        w = w * (1.0 - lr_t * wd)
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    c1, c2 = (1.0, 1.0) if defect == "no_bias_correction" else (1.0 - b1 ** t, 1.0 - b2 ** t)
    if defect == "eps_inside_sqrt":
        denom = (v / c2 + eps).sqrt()
    else:
        denom = v.sqrt() / math.sqrt(c2) + eps
    return w - (lr_t / c1) * m / denom, m, v


def adam_terms(w, grad, m, v, t, h: Hyper, lr_scale=1.0):
    """terms_abs of (w, m, v): |w| (1 + lr_t wd) + |update|,  |m| + (1 - b1)(|g| + |m|),  b2 |v| + (1 - b2) g^2 - in float64, g's own
    two terms taken by absolute value."""
    w, grad, m, v = (x.to(F64) for x in (w, grad, m, v))
    lr_t = f32(h.lr) * f32(lr_scale)
    b1, b2, wd = f32(h.beta1), f32(h.beta2), f32(h.weight_decay)
    ga = grad.abs() * abs(f32(h.grad_scale)) + (0.0 if h.decoupled else wd * w.abs())
    w1, _, _ = adam_step(w, grad, m, v, t, h, lr_scale)
    w_dec = w * (1.0 - lr_t * wd) if h.decoupled else w
    return (w.abs() * (1.0 + lr_t * wd) + (w1 - w_dec).abs(), m.abs() + (1.0 - b1) * (ga + m.abs()), b2 * v.abs() + (1.0 - b2) * ga * ga)


def bars(w, grad, m, v, t, h: Hyper, lr_scale=1.0):
    """(reference (w, m, v) in float64, the bar of each) for one step from these before-values."""
    from util_rowops import tol
    ref = adam_step(w, grad, m, v, t, h, lr_scale)
    r32 = adam_step(w, grad, m, v, t, h, lr_scale, dtype=F32)
    terms = adam_terms(w, grad, m, v, t, h, lr_scale)
    return ref, tuple(tol(r, a, b) for r, a, b in zip(ref, r32, terms))


# ------------------------------------------------------------------------------------------- the GPU test's item lists
# Hyper-parameters chosen so that each planted defect lands beyond four bars somewhere (tests/test_adam_host.py proves it on
# these very inputs): lr = 1e-2 with wd = 0.1 and |w| about 1 makes the decay visible against the update, grad_scale = 0.25
# separates "scaled gradient + decay" from "scaled (gradient + decay)", and the family with gradients about 1e-3 and eps = 1e-3
# is the one where eps inside or outside the square root differ.
FAMILIES = (
    Hyper(1e-2, 0.9, 0.999, 1e-8, 0.1, 0.25, 0),       # Adam, L2 decay joins the scaled gradient
    Hyper(1e-2, 0.9, 0.999, 1e-8, 0.1, 0.25, 1),       # AdamW
    Hyper(1e-2, 0.9, 0.999, 1e-3, 0.1, 1.0, 1),        # AdamW, gradients about 1e-3 against eps = 1e-3
    Hyper(1e-2, 0.8, 0.99, 1e-3, 0.1, 0.25, 0),        # Adam, small gradients, other betas
)
GRAD_SIZE = (1.0, 1.0, 1e-3, 1e-3)                     # per family
PER_WG = 8192                                          # elements one workgroup owns (csrc/rowops.hip, ADA_PER_WG)
# the sizes the issue names - one element each side of a workgroup slice, a 2-D weight that ends inside a slice, an empty item in
# the middle - then small ones up to 60 items (two launches of 48 + 12)
NAMED_SIZES = (1, 3, 4, 5, PER_WG - 1, PER_WG, PER_WG + 1, 3 * 7, 2048 * 513)
EMPTY_AT, UNALIGNED_AT, ALIGNED_TWIN_AT = 20, 33, 34
N_ITEMS = 60

Item = namedtuple("Item", "n hyper misaligned")


def gpu_items(lr=None):
    """The 60 items of the GPU test.  ``lr``: one learning rate for every item (the lr_scale test needs a power of two)."""
    sizes = list(NAMED_SIZES) + [7 + 37 * i for i in range(N_ITEMS - len(NAMED_SIZES))]
    sizes[EMPTY_AT] = 0
    sizes[UNALIGNED_AT] = sizes[ALIGNED_TWIN_AT] = PER_WG + 1
    items = []
    for i, n in enumerate(sizes):
        h = FAMILIES[i % len(FAMILIES)]
        if i == ALIGNED_TWIN_AT:
            h = items[UNALIGNED_AT].hyper
        if lr is not None:
            h = h._replace(lr=lr)
        items.append(Item(n, h, i == UNALIGNED_AT))
    return items


GUARD = 64          # NaN floats in front of, between and behind the items' regions


def layout(items):
    """(offset of every item in a flat float32 arena, arena length): regions start on 16-byte boundaries - the misaligned item one
    float (4 bytes) past one - with GUARD floats between them."""
    offs, at = [], GUARD
    for it in items:
        offs.append(at + (1 if it.misaligned else 0))
        at = (offs[-1] + it.n + GUARD + 3) // 4 * 4
    return offs, at


def gpu_inputs(items, seed=0):
    """Four flat arenas (w, grad, m, v), NaN outside the items' regions: |w| in [0.5, 1.5] with random signs, gradients normal
    at the family's size, a state as some steps would have left it (m about a tenth of a gradient, v > 0).  The aligned twin
    holds the misaligned item's values."""
    offs, total = layout(items)
    g = torch.Generator().manual_seed(seed)
    arenas = [torch.full((total,), float("nan"), dtype=F32) for _ in range(4)]
    for i, (it, o) in enumerate(zip(items, offs)):
        if i == ALIGNED_TWIN_AT:
            src = offs[UNALIGNED_AT]
            for a in arenas:
                a[o:o + it.n] = a[src:src + it.n]
            continue
        size = GRAD_SIZE[i % len(FAMILIES)]
        sign = torch.randint(0, 2, (it.n,), generator=g).float() * 2 - 1
        arenas[0][o:o + it.n] = sign * (0.5 + torch.rand(it.n, generator=g))
        arenas[1][o:o + it.n] = size * torch.randn(it.n, generator=g)
        arenas[2][o:o + it.n] = 0.1 * size * torch.randn(it.n, generator=g)
        arenas[3][o:o + it.n] = size * size * (0.01 + torch.rand(it.n, generator=g))
    return arenas, offs


def data_mask(items, offs, total):
    mask = torch.zeros(total, dtype=torch.bool)
    for it, o in zip(items, offs):
        mask[o:o + it.n] = True
    return mask


# ------------------------------------------------------------------------------------------- the integer-valued family
def int_family(beta2, decoupled, n=PER_WG + 7, seed=3):
    """Inputs on which every intermediate of one step at t = 1 is a float32 number, so the kernel must EQUAL float64: w, m small
    integers, grad a signed power of two with grad - m even, v = 0, beta1 = 0.5, eps = 0, lr = 2**-3, grad_scale = 2, and
    weight decay 0.5 when decoupled (1 - lr wd = 15/16) else 0.  With beta2 = 0.75 the second-moment correction is
    1 / sqrt(1 - 0.75) = 2 and the whole chain is exact; with beta2 = 0.5 it is sqrt(2): m and v are still exact, w is not
    (``exact_chain`` says which intermediates are)."""
    g = torch.Generator().manual_seed(seed)
    grad = (2.0 ** torch.randint(0, 4, (n,), generator=g).float()) * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1)
    m = 2.0 * grad + 2.0 * torch.randint(-3, 4, (n,), generator=g).float()          # grad * grad_scale - m is even
    w = torch.randint(-8, 9, (n,), generator=g).float()
    h = Hyper(2.0 ** -3, 0.5, beta2, 0.0, 0.5 if decoupled else 0.0, 2.0, int(decoupled))
    return w, grad, m, torch.zeros(n), h


def exact_chain(w, grad, m, v, h: Hyper):
    """{intermediate: is every element (or the scalar) exactly a float32 number} for the kernel's chain at t = 1, evaluated in
    float64."""
    def ok(x):
        x = torch.as_tensor(x, dtype=F64)
        return bool(torch.equal(x.to(F32).to(F64), x))
    w, grad, m, v = (x.to(F64) for x in (w, grad, m, v))
    lr_t = f32(h.lr)
    out = {"1-b1": ok(1.0 - h.beta1), "1-b2": ok(1.0 - h.beta2), "step": ok(lr_t / (1.0 - h.beta1)),
           "rsb2": ok(1.0 / math.sqrt(1.0 - h.beta2)), "keep": ok(1.0 - lr_t * h.weight_decay)}
    g = grad * h.grad_scale
    out["g"] = ok(g)
    if h.decoupled:
        w = w * (1.0 - lr_t * h.weight_decay)
        out["w*keep"] = ok(w)
    else:
        out["wd*w"] = ok(h.weight_decay * w)
        g = g + h.weight_decay * w
        out["g+wd*w"] = ok(g)
    out["g-m"] = ok(g - m)
    out["(1-b1)(g-m)"] = ok((1.0 - h.beta1) * (g - m))
    m1 = m + (1.0 - h.beta1) * (g - m)
    out["m"] = ok(m1)
    out["g*g"], out["(1-b2)g*g"], out["b2*v"] = ok(g * g), ok((1.0 - h.beta2) * g * g), ok(h.beta2 * v)
    v1 = h.beta2 * v + (1.0 - h.beta2) * g * g
    out["v"] = ok(v1)
    out["sqrt(v)"] = ok(v1.sqrt())
    step = lr_t / (1.0 - h.beta1)
    out["step*m"] = ok(step * m1)
    if out["rsb2"] and out["sqrt(v)"]:
        den = v1.sqrt() * (1.0 / math.sqrt(1.0 - h.beta2))
        out["denominator"], out["quotient"], out["w"] = ok(den), ok(step * m1 / den), ok(w - step * m1 / den)
    return out
