"""What the learning-rate schedule tests share (tests/test_lr_schedule_host.py, tests/test_lr_schedule_gpu.py): an independent
restatement of ``lstc_lr_schedule``'s arithmetic (include/lstc_hip.h) with planted defects, the exact rational value of the
kinds that have one, the grids both tests walk, and the float64-stated chain of one scaled Adagrad step.  No project kernel is
called here.

    t <  W:  f = ws + (1 - ws) t / W
    t >= W:  u = min(t - W, D),  D = T - W
             constant 1 | linear 1 - (1 - m) u / D | cosine m + (1 - m) (1 + cos(pi u / D)) / 2
             step max(m, gamma^((t - W) // step_size)) | inv_sqrt max(m, sqrt(W' / max(t, W'))),  W' = max(W, 1)
"""
import math
from fractions import Fraction

import numpy as np
import torch

KINDS = ("constant", "linear", "cosine", "step", "inv_sqrt")
DEFECTS = ("t_off_by_one", "warmup_ignored", "no_clamp_after_T", "min_scale_ignored", "scale_squared")


def f32(x):
    """The value an f32 field of LstcLrSchedule holds for the Python number ``x``."""
    return float(np.float32(x))


def twin(t, kind, warmup_steps=0, total_steps=None, min_scale=0.0, warmup_start=0.0, step_size=None, gamma=0.1, defect=None):
    """f(t) in float64 from the f32 fields widened, rounded once to float32.  ``defect``: one of DEFECTS, a wrong schedule that
    the grid of the tests must tell from the true one."""
    W, T = int(warmup_steps), int(total_steps or 0)
    m, ws, g = f32(min_scale), f32(warmup_start), f32(gamma)
    if defect == "t_off_by_one":
        t = t + 1
    if defect == "min_scale_ignored":
        m = 0.0
    if t < W and defect != "warmup_ignored":
        f = ws + (1.0 - ws) * float(t) / float(W)
    else:
        D = float(T - W)
        u = float(max(t - W, 0))
        if defect != "no_clamp_after_T":
            u = min(u, D)
        if kind == "linear":
            f = 1.0 - (1.0 - m) * u / D
        elif kind == "cosine":
            f = m + (1.0 - m) * 0.5 * (1.0 + math.cos(math.pi * u / D))
        elif kind == "step":
            r, b, e = 1.0, g, max(t - W, 0) // int(step_size)
            while e:                                          # gamma^e by repeated squaring, as the kernel's pow_f64
                if e & 1:
                    r = r * b
                b, e = b * b, e >> 1
            f = max(m, r)
        elif kind == "inv_sqrt":
            Wp = max(float(W), 1.0)
            f = max(m, math.sqrt(Wp / max(float(t), Wp)))
        else:
            f = 1.0
    if defect == "scale_squared":
        f = f * f
    return np.float32(f)


def exact(t, kind, warmup_steps=0, total_steps=None, min_scale=0.0, warmup_start=0.0, step_size=None, gamma=0.1):
    """f(t) as a Fraction (the SQUARE of it for inv_sqrt above its floor, as ``("sq", Fraction)``), from the f32 fields taken
    exactly; None for cosine, which has no rational value."""
    W, T = int(warmup_steps), int(total_steps or 0)
    m, ws, g = (Fraction(f32(x)) for x in (min_scale, warmup_start, gamma))
    if t < W:
        return ws + (1 - ws) * t / W
    if kind == "constant":
        return Fraction(1)
    if kind == "linear":
        return 1 - (1 - m) * min(t - W, T - W) / (T - W)
    if kind == "step":
        return max(m, g ** ((t - W) // int(step_size)))
    if kind == "inv_sqrt":
        Wp = max(W, 1)
        sq = Fraction(Wp, max(t, Wp))
        return m if sq <= m * m else ("sq", sq)
    return None


def configs(grid, ms=(0.0, 0.1), wss=(0.25, 1.0)):
    """Every kind on every (W, T) of ``grid``; "step" with step_size 1 and 3 at gamma 0.5."""
    out = []
    for W, T in grid:
        for m in ms:
            for ws in wss:
                base = dict(warmup_steps=W, total_steps=T, min_scale=m, warmup_start=ws)
                for kind in ("constant", "linear", "cosine", "inv_sqrt"):
                    out.append(dict(base, kind=kind))
                for size in (1, 3):
                    out.append(dict(base, kind="step", step_size=size, gamma=0.5))
    return out


HOST_GRID = ((0, 20), (1, 7), (5, 20))          # against torch's schedulers, T + 5 steps each
GPU_GRID = ((0, 1), (1, 2), (3, 8))             # on the device, T + 4 launches each


# ------------------------------------------------------------------------------------------- scaled Adagrad
def adagrad_scaled_step(w, grad, s, lr, wd, eps, gscale, lr_scale):
    """One element-wise step of lstc_adagrad_multi_scaled on float32 numpy arrays (torch tensors are converted), every operation
    rounded once in the kernel's order; lr_t = (float)((double)lr * (double)lr_scale) is formed in float64 from the f32 numbers and
    rounded once.  numpy's float32 ``+ - * /`` and ``sqrt`` are IEEE's correctly rounded operations (torch's vectorised CPU
    ``sqrt`` is not on every build, so it is not used here).  Returns (w, s) as float32 tensors."""
    F = np.float32
    w, grad, s = (np.asarray(x, dtype=F) for x in (w, grad, s))
    lr_t = F(f32(lr) * f32(lr_scale))          # a product of two f32 numbers is exact in float64: one rounding
    wd, eps, gscale = F(wd), F(eps), F(gscale)
    gg = grad * gscale + wd * w
    s = s + gg * gg
    w = w - lr_t * gg / (np.sqrt(s) + eps)
    assert w.dtype == F and s.dtype == F
    return torch.from_numpy(w), torch.from_numpy(s)
