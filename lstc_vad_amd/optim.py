"""The optimizers of the training step, each stepped by ONE fused multi-tensor HIP launch.

``Adagrad`` is the reference's: it builds ``torch.optim.Adagrad([{params: encoder, lr: lr_encoder}, {params: head, lr: lr_head}],
weight_decay=wd)`` (Train/temporal_transformer_shanghaitech.py:83-85) and calls ``zero_grad / backward /
[clip_grad_norm_] / step`` (:137-142).  This class keeps that surface (param groups, ``zero_grad``, ``step``,
``state_dict``) and the exact update ``g += wd*w; s += g*g; w -= lr*g/(sqrt(s)+1e-10)``; parameters whose
``grad`` is None are skipped exactly like upstream (unused LayerNorms never get a gradient).

``Adam`` and ``AdamW`` are ``torch.optim.Adam`` / ``torch.optim.AdamW`` (amsgrad off) on ``lstc_adam_multi``: the step count and
the learning-rate multiplier live on the device, so a captured step (engine.GraphedStep) replays as step 2, 3, ... and follows
a schedule set through ``set_lr_scale``.  All three share ``step(closure, grad_scales, only)`` and what follows the launch.

``EMA`` is their companion: an exponential moving average of every weight, one ``lstc_ema_multi`` launch behind the optimizer's,
and ``lstc_swap_multi`` to evaluate and save the averaged model out of the live parameter storage.

``LRSchedule`` moves the one device float all three read through ``set_lr_scale``: warm-up and decay as one ``lstc_lr_schedule``
launch in front of the step.  Adagrad allocates that float, and switches to ``lstc_adagrad_multi_scaled``, only when asked to.
"""
from __future__ import annotations

import contextlib
import ctypes
import math

import torch

from . import _lib
from ._lib import check, dev_ptr, stream_ptr


class _MultiTensorOptimizer(torch.optim.Optimizer):
    """What every optimizer here shares: the selection of the parameters of a step, one launch over all of them, and the
    packed-weight bookkeeping behind it.  A subclass gives ``_item`` (one parameter's entry of the launch; it advances that
    parameter's host step count), ``_launch``, and the host step count itself (``host_step`` / ``set_host_step``)."""

    @torch.no_grad()
    def step(self, closure=None, grad_scales=None, only=None):
        """``grad_scales``: optional {group index: device-or-host scale} from ``clip_grad_norm_`` below.  ``only``: step just these
        parameters (one gradient bucket of a data-parallel job whose all-reduce has landed - engine.TrainStep steps bucket k while
        the backward of the layers below it is still running); the element arithmetic does not depend on how the parameters are
        grouped into launches, so any partition into ``only`` sets gives the weights of ONE whole step bit for bit."""
        lib = _lib.load()
        items, keep, updated = [], [], []
        sel = None if only is None else {id(p) for p in only}
        for gi, group in enumerate(self.param_groups):
            gs = 1.0 if not grad_scales else float(grad_scales.get(gi, 1.0))
            for p in group["params"]:
                if p.grad is None or (sel is not None and id(p) not in sel):
                    continue
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(g)
                updated.append(p)
                items.append(self._item(group, p, g, gs))
        if items:           # every parameter in ONE launch
            self._launch(lib, items)
        from .functional import bump_weight_epoch, repack_weights
        bump_weight_epoch(updated)   # THESE weights changed through raw pointers: their packed copies (f32x3 / bf16 GEMM) are stale
        if items and not torch.cuda.is_current_stream_capturing():
            # bf16 mode: every packed weight copy of the finished step rebuilt in one launch (a captured step keeps the
            # lazily issued packs of its forward instead: the graph replays those)
            repack_weights(updated)
        return None

    def host_step(self, p) -> int:
        """Steps taken on ``p`` as the host counts them (what ``state_dict`` reports).  engine.GraphedStep reads it, puts it back
        after its warm-up and capture, and adds 1 per replay."""
        return self.state[p]["step"]

    def set_host_step(self, p, n: int):
        self.state[p]["step"] = n


class Adagrad(_MultiTensorOptimizer):
    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0, initial_accumulator_value=0, eps=1e-10):
        if lr_decay != 0:
            raise NotImplementedError("lr_decay is 0 everywhere on the LSTC_VAD path")
        defaults = dict(lr=lr, weight_decay=weight_decay, eps=eps, initial_accumulator_value=initial_accumulator_value)
        super().__init__(params, defaults)
        self._lr_scale = None          # the device float of a schedule: allocated by the first set_lr_scale, never without one
        for group in self.param_groups:
            for p in group["params"]:
                self.state[p]["sum"] = torch.full_like(p, float(group["initial_accumulator_value"]),
                                                       memory_format=torch.preserve_format)
                self.state[p]["step"] = 0

    def set_lr_scale(self, x: float):
        """lr_t = lr * x from the next step on, eager or captured (a schedule's hook, as Adam's).  The first call allocates the
        device float; from then on every launch is ``lstc_adagrad_multi_scaled`` and reads it (x = 1 gives the same bits)."""
        if self._lr_scale is None:
            dev = self.param_groups[0]["params"][0].device
            self._lr_scale = torch.ones(1, dtype=torch.float32, device=dev)
        self._lr_scale.fill_(float(x))

    def _item(self, group, p, g, gs):
        state = self.state[p]
        state["step"] += 1
        return (dev_ptr(p.data), dev_ptr(g), dev_ptr(state["sum"]), p.numel(), float(group["lr"]),
                float(group["weight_decay"]), float(group["eps"]), gs)

    def _launch(self, lib, items):          # lstc_adagrad_multi; element arithmetic of lstc_adagrad_step
        arr = (_lib.AdagradItem * len(items))(*items)
        if self._lr_scale is None:
            check(lib.lstc_adagrad_multi(arr, len(items), stream_ptr()), "lstc_adagrad_multi")
        else:
            check(lib.lstc_adagrad_multi_scaled(arr, len(items), dev_ptr(self._lr_scale), stream_ptr()), "lstc_adagrad_multi_scaled")


class Adam(_MultiTensorOptimizer):
    """``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` with ``amsgrad=False, maximize=False`` (include/lstc_hip.h,
    lstc_adam_multi, states the arithmetic).  State per parameter, under torch's keys: ``exp_avg``, ``exp_avg_sq`` and ``step`` -
    here a 0-dim view of ONE int32 device tensor holding every parameter's count, which the launch itself increments.  The host
    keeps its own count per parameter (``host_step``) so that ``state_dict()`` needs no device read; ``state_dict()`` emits and
    ``load_state_dict()`` accepts ``step`` the way torch writes it (a 0-dim float tensor), parameters that were never stepped
    have no entry, as in torch: a state saved by either optimizer loads into the other."""
    _torch_twin = torch.optim.Adam

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False):
        if amsgrad:
            raise NotImplementedError("amsgrad is not implemented (lstc_adam_multi keeps no running maximum)")
        # torch's own argument checks and its param-group keys (foreach, capturable, ...): a state_dict passes either way
        defaults = dict(self._torch_twin([torch.empty(0)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults)
        self._words = None
        super().__init__(params, defaults)
        plist = [p for group in self.param_groups for p in group["params"]]
        dev = plist[0].device
        self._words = torch.zeros(len(plist), dtype=torch.int32, device=dev)
        self._lr_scale = torch.ones(1, dtype=torch.float32, device=dev)
        self._host_step = {}
        for i, p in enumerate(plist):
            self._host_step[p] = 0
            self.state[p] = {"step": self._words[i], "exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                             "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}

    def add_param_group(self, param_group):
        if getattr(self, "_words", None) is not None:
            raise NotImplementedError("param groups are fixed at construction: the step words are one device tensor")
        super().add_param_group(param_group)

    def set_lr_scale(self, x: float):
        """lr_t = lr * x from the next step on, eager or captured: every launch reads this one device word (a schedule's hook)."""
        self._lr_scale.fill_(float(x))

    def host_step(self, p) -> int:
        return self._host_step[p]

    def set_host_step(self, p, n: int):
        self._host_step[p] = n

    def _item(self, group, p, g, gs):
        st = self.state[p]
        b1, b2 = group["betas"]
        decoupled = bool(group.get("decoupled_weight_decay", self._torch_twin is torch.optim.AdamW))
        item = (dev_ptr(p.data), dev_ptr(g), dev_ptr(st["exp_avg"]), dev_ptr(st["exp_avg_sq"]), p.numel(), dev_ptr(st["step"]),
                dev_ptr(self._lr_scale), float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                float(group["weight_decay"]), gs, int(decoupled))
        self._host_step[p] += 1
        return item

    def _launch(self, lib, items):
        arr = (_lib.AdamItem * len(items))(*items)
        check(lib.lstc_adam_multi(arr, len(items), stream_ptr()), "lstc_adam_multi")

    def _ordered(self):
        return [p for group in self.param_groups for p in group["params"]]

    def state_dict(self):
        sd = super().state_dict()
        dt = torch.float64 if torch.get_default_dtype() == torch.float64 else torch.float32       # torch's scalar dtype for `step`
        for k, p in enumerate(self._ordered()):
            t = self._host_step[p]
            if t == 0:
                sd["state"].pop(k, None)
            else:
                sd["state"][k] = dict(sd["state"][k], step=torch.tensor(float(t), dtype=dt))
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)          # deep copies, cast to each parameter's device and dtype; `step` as saved
        for i, p in enumerate(self._ordered()):
            st = self.state[p]
            t = int(st["step"]) if "step" in st else 0
            self._words[i] = t
            self._host_step[p] = t
            st["step"] = self._words[i]
            for key in ("exp_avg", "exp_avg_sq"):
                st[key] = (st[key].contiguous() if key in st else torch.zeros_like(p, memory_format=torch.contiguous_format))


class AdamW(Adam):
    """``torch.optim.AdamW``: the weight is shrunk by ``1 - lr_t * weight_decay`` before the Adam update instead of the decay
    joining the gradient."""
    _torch_twin = torch.optim.AdamW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)


class EMA:
    """``avg = avg + (1 - decay_t) * (w - avg)`` for every parameter in ONE launch (include/lstc_hip.h, lstc_ema_multi, states the
    arithmetic): Polyak averaging of the weights an optimizer above steps.  The first update copies the weights
    (``torch.optim.swa_utils.AveragedModel`` at ``n_averaged == 0``); ``warmup`` ramps the decay up as TensorFlow's
    ``num_updates`` does, ``decay_t = min(decay, (1 + u) / (10 + u))``.  The update counts are ONE int32 device tensor that the
    launch itself increments (``state[p]["count"]`` is its 0-dim view), so a captured update (engine.GraphedStep) replays as
    update 2, 3, ...; the host keeps its own count per parameter and ``state_dict()`` needs no device read.

    ``swap()`` exchanges parameters and averages in place (``lstc_swap_multi``), so fused Q|K|V views and raw pointers held
    elsewhere see the averaged weights; ``averaged()`` is the context manager around an evaluation or a checkpoint."""

    def __init__(self, params, decay=0.999, warmup=False):
        self.decay, self.warmup = self._checked(decay, warmup)
        params = list(params)
        if params and isinstance(params[0], dict):
            params = [p for group in params for p in group["params"]]
        if not params:
            raise ValueError("EMA: no parameters")
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError("EMA: parameters must be contiguous float32 tensors")
        self.params = params
        self._words = torch.zeros(len(params), dtype=torch.int32, device=params[0].device)
        self._host_count = {p: 0 for p in params}
        self.state = {p: {"count": self._words[i], "avg": p.detach().clone(memory_format=torch.contiguous_format)}
                      for i, p in enumerate(params)}
        self._swapped = self._inside = False

    @staticmethod
    def _checked(decay, warmup):
        """The kernel's rules, on the host: decay in [0, 1) as a float32, warmup 0 / 1."""
        d = float(decay)
        if not math.isfinite(d) or not 0.0 <= d or not float(torch.tensor(d, dtype=torch.float32)) < 1.0:
            raise ValueError(f"EMA: decay must be in [0, 1), not {decay!r}")
        if warmup not in (False, True, 0, 1):
            raise ValueError(f"EMA: warmup must be False or True, not {warmup!r}")
        return d, bool(warmup)

    def host_count(self, p) -> int:
        """Updates of ``p`` as the host counts them (the mirror of its device word; engine.GraphedStep adds 1 per replay)."""
        return self._host_count[p]

    def set_host_count(self, p, n: int):
        self._host_count[p] = n

    @torch.no_grad()
    def update(self, only=None):
        """One update of every parameter - with or without ``.grad`` - or of the ``only`` subset (one gradient bucket, behind
        ``optimizer.step(only=...)``): the element arithmetic does not depend on how the parameters are grouped into launches,
        so any partition into ``only`` sets gives ONE whole update bit for bit."""
        if self._swapped:
            raise RuntimeError("EMA.update: the parameters hold the averages (inside averaged(), or after an odd number of swap())")
        sel = None if only is None else {id(p) for p in only}
        items = []
        for p in self.params:
            if sel is not None and id(p) not in sel:
                continue
            st = self.state[p]
            items.append((dev_ptr(st["avg"]), dev_ptr(p.data), p.numel(), dev_ptr(st["count"]), self.decay, int(self.warmup)))
            self._host_count[p] += 1
        if items:
            arr = (_lib.EmaItem * len(items))(*items)
            check(_lib.load().lstc_ema_multi(arr, len(items), stream_ptr()), "lstc_ema_multi")

    @torch.no_grad()
    def swap(self):
        """Parameters <-> averages, bit for bit, in one launch; then what follows every raw-pointer write to the weights."""
        items = [(dev_ptr(p.data), dev_ptr(self.state[p]["avg"]), p.numel()) for p in self.params]
        arr = (_lib.SwapItem * len(items))(*items)
        check(_lib.load().lstc_swap_multi(arr, len(items), stream_ptr()), "lstc_swap_multi")
        self._swapped = not self._swapped
        from .functional import bump_weight_epoch, repack_weights
        bump_weight_epoch(self.params)
        if not torch.cuda.is_current_stream_capturing():
            repack_weights(self.params)

    @contextlib.contextmanager
    def averaged(self):
        """The model holds its averaged weights inside the block and its training weights again behind it."""
        if self._inside or self._swapped:
            raise RuntimeError("EMA.averaged: the parameters already hold the averages")
        self._inside = True
        try:
            self.swap()
            try:
                yield self
            finally:
                self.swap()
        finally:
            self._inside = False

    def state_dict(self):
        if self._swapped:
            raise RuntimeError("EMA.state_dict: the parameters hold the averages; leave averaged() first")
        return {"decay": self.decay, "warmup": self.warmup, "counts": [self._host_count[p] for p in self.params],
                "avg": [self.state[p]["avg"] for p in self.params]}

    @torch.no_grad()
    def load_state_dict(self, sd):
        if self._swapped:
            raise RuntimeError("EMA.load_state_dict: the parameters hold the averages; leave averaged() first")
        avg, counts = list(sd["avg"]), [int(n) for n in sd["counts"]]
        if len(avg) != len(self.params) or len(counts) != len(self.params):
            raise ValueError(f"EMA.load_state_dict: {len(avg)} averages and {len(counts)} counts for {len(self.params)} parameters")
        for k, (p, a) in enumerate(zip(self.params, avg)):
            if tuple(a.shape) != tuple(p.shape):
                raise ValueError(f"EMA.load_state_dict: average {k} has shape {tuple(a.shape)}, its parameter {tuple(p.shape)}")
        if any(n < 0 for n in counts):
            raise ValueError("EMA.load_state_dict: negative count")
        self.decay, self.warmup = self._checked(sd["decay"], sd["warmup"])
        for p, a, n in zip(self.params, avg, counts):
            self.state[p]["avg"].copy_(a)
            self._host_count[p] = n
        self._words.copy_(torch.tensor(counts, dtype=torch.int32))


class LRSchedule:
    """Warm-up and decay of the learning rates of an optimizer above, evaluated on the device: ONE ``lstc_lr_schedule`` launch per
    training step reads this schedule's step word, writes ``f(t)`` into the optimizer's ``_lr_scale`` float - the multiplier every
    ``lstc_adam_multi`` / ``lstc_adagrad_multi_scaled`` launch reads - and adds 1 to the word (include/lstc_hip.h states ``f``).
    ``t`` is the zero-based index of the optimizer step about to be taken (torch's ``last_epoch``): call ``step()`` IN FRONT of
    ``optimizer.step()``, once per training step however many ``step(only=...)`` bucket launches that step is made of.  Nothing
    that changes from step to step is passed by value, so a captured step (engine.GraphedStep) replays as step t + 1, t + 2, ...

    ``kind``: "constant", "linear", "cosine", "step" or "inv_sqrt".  The first ``warmup_steps`` steps ramp linearly from
    ``warmup_start`` to 1 for every kind; "linear" and "cosine" then reach ``min_scale`` at ``total_steps`` and stay there, "step"
    multiplies by ``gamma`` every ``step_size`` steps and "inv_sqrt" decays as sqrt(W / t), both floored at ``min_scale``.  The
    host keeps its own count (``host_step``) and its own float64 twin of ``f`` (``scale_at``): nothing here reads the device."""
    KINDS = ("constant", "linear", "cosine", "step", "inv_sqrt")
    INT32_MAX = 2 ** 31 - 1

    def __init__(self, optimizer, kind, warmup_steps=0, total_steps=None, min_scale=0.0, warmup_start=0.0, step_size=None,
                 gamma=0.1):
        self.config = self._checked(kind, warmup_steps, total_steps, min_scale, warmup_start, step_size, gamma)
        if not hasattr(optimizer, "set_lr_scale"):
            raise TypeError("LRSchedule: the optimizer has no set_lr_scale (optim.Adagrad, optim.Adam and optim.AdamW do)")
        self.optimizer = optimizer
        if getattr(optimizer, "_lr_scale", None) is None:
            optimizer.set_lr_scale(1.0)          # Adagrad: the device float exists from here on, and its launches read it
        self._scale = optimizer._lr_scale
        self._step = torch.zeros(1, dtype=torch.int32, device=self._scale.device)
        self._host = 0
        c = self.config
        self._desc = _lib.LrSchedule(self.KINDS.index(c["kind"]), c["warmup_steps"], c["total_steps"], c["step_size"],
                                     c["warmup_start"], c["min_scale"], c["gamma"])

    @classmethod
    def _checked(cls, kind, warmup_steps=0, total_steps=None, min_scale=0.0, warmup_start=0.0, step_size=None, gamma=0.1):
        """The kernel's rules, on the host; returns the configuration as the kernel's fields hold it (f32 numbers, 0 for the
        integers a kind ignores and the caller left out)."""
        if kind not in cls.KINDS:
            raise ValueError(f"LRSchedule: kind must be one of {cls.KINDS}, not {kind!r}")
        ints = {}
        for name, v in (("warmup_steps", warmup_steps), ("total_steps", total_steps), ("step_size", step_size)):
            v = 0 if v is None else v
            if isinstance(v, bool) or int(v) != v or abs(int(v)) > cls.INT32_MAX:
                raise ValueError(f"LRSchedule: {name} must be a 32-bit integer, not {v!r}")
            ints[name] = int(v)
        if ints["warmup_steps"] < 0:
            raise ValueError("LRSchedule: warmup_steps must be >= 0")
        if kind in ("linear", "cosine") and ints["total_steps"] <= ints["warmup_steps"]:
            raise ValueError(f"LRSchedule: kind {kind!r} needs total_steps > warmup_steps, not {total_steps!r} and {warmup_steps!r}")
        if kind == "step" and ints["step_size"] < 1:
            raise ValueError(f"LRSchedule: kind 'step' needs step_size >= 1, not {step_size!r}")
        f32 = lambda x: ctypes.c_float(float(x)).value          # the number the kernel's f32 field holds
        ws, m, g = f32(warmup_start), f32(min_scale), f32(gamma)
        if not 0.0 <= ws <= 1.0 or not 0.0 <= m <= 1.0:          # NaN fails both
            raise ValueError(f"LRSchedule: warmup_start and min_scale must be in [0, 1], not {warmup_start!r} and {min_scale!r}")
        if kind == "step" and not 0.0 < g <= 1.0:
            raise ValueError(f"LRSchedule: kind 'step' needs gamma in (0, 1], not {gamma!r}")
        return dict(kind=kind, **ints, min_scale=m, warmup_start=ws, gamma=g)

    @classmethod
    def scale_at(cls, t, kind, warmup_steps=0, total_steps=None, min_scale=0.0, warmup_start=0.0, step_size=None, gamma=0.1):
        """The host twin of the kernel: ``f(t)`` by the same float64 expressions in the same order, rounded once, as ``np.float32``."""
        return cls._f(cls._checked(kind, warmup_steps, total_steps, min_scale, warmup_start, step_size, gamma), t)

    @staticmethod
    def _f(c, t):
        """``f(t)`` of a configuration ``_checked`` returned."""
        import numpy as np
        kind, W, T, m, ws, t = c["kind"], c["warmup_steps"], c["total_steps"], c["min_scale"], c["warmup_start"], int(t)
        if t < W:
            return np.float32(ws + (1.0 - ws) * float(t) / float(W))
        D = float(T - W)
        u = min(float(t - W), D)
        if kind == "linear":
            f = 1.0 - (1.0 - m) * u / D
        elif kind == "cosine":
            f = m + (1.0 - m) * 0.5 * (1.0 + math.cos(3.141592653589793 * u / D))
        elif kind == "step":
            b, e, r = c["gamma"], (t - W) // c["step_size"], 1.0
            while e:                        # the kernel's pow_f64: repeated squaring in float64
                if e & 1:
                    r *= b
                e >>= 1
                b *= b
            f = max(m, r)
        elif kind == "inv_sqrt":
            Wp = max(float(W), 1.0)
            f = max(m, math.sqrt(Wp / max(float(t), Wp)))
        else:
            f = 1.0
        return np.float32(f)

    def scale(self, t):
        """``scale_at(t)`` of this schedule (its configuration was checked at construction)."""
        return self._f(self.config, t)

    def step(self):
        """The one launch, on the current stream: *scale = f(*step), *step += 1.  The host count follows without a device read."""
        check(_lib.load().lstc_lr_schedule(ctypes.byref(self._desc), dev_ptr(self._step), dev_ptr(self._scale), stream_ptr()),
              "lstc_lr_schedule")
        self._host = min(self._host + 1, self.INT32_MAX)

    def host_step(self) -> int:
        """Ticks so far as the host counts them: the index of the NEXT optimizer step (the mirror of the device word;
        engine.GraphedStep reads it, puts it back after its warm-up and capture, and adds 1 per replay)."""
        return self._host

    def set_host_step(self, n: int):
        self._host = int(n)

    def get_last_lr(self):
        """The rate of every param group at the last step taken (before the first: at step 0), as torch's schedulers report it."""
        s = float(self.scale(max(self._host - 1, 0)))
        return [float(group["lr"]) * s for group in self.optimizer.param_groups]

    def state_dict(self):
        return dict(self.config, step=self._host)

    def load_state_dict(self, sd):
        """Continue at ``sd["step"]``: sets the device word and the host count.  The configuration must be this schedule's."""
        theirs = {k: v for k, v in sd.items() if k != "step"}
        try:
            theirs = self._checked(**theirs)
        except TypeError as e:
            raise ValueError(f"LRSchedule.load_state_dict: {e}") from None
        if theirs != self.config:
            raise ValueError(f"LRSchedule.load_state_dict: the saved schedule {theirs} is not this one {self.config}")
        n = int(sd["step"])
        if not 0 <= n <= self.INT32_MAX:
            raise ValueError(f"LRSchedule.load_state_dict: step {n} is no step count")
        self._step.fill_(n)
        self._host = n


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_(params, 10)`` (Train/temporal_transformer_shanghaitech.py:139-141): total L2 norm over
    the given parameters' grads and an in-place scale by ``max_norm / (total + 1e-6)`` clamped to 1 (torch semantics) - as TWO
    launches over the whole list (``lstc_sqnorm_multi`` + ``lstc_clip_scale_multi``, the coefficient formed on the device)
    instead of upstream's kernel per tensor and host comparison.  No host sync, so a captured step may contain it.  Returns
    the total norm as a 0-dim device tensor (torch returns a device tensor too)."""
    if norm_type != 2.0:
        raise NotImplementedError("clip_grad_norm_: only the L2 norm the LSTC_VAD scripts use")
    params = [p for p in parameters if p.grad is not None and p.grad.numel() > 0]       # torch accepts empty tensors: nothing to scale
    if not params:
        return torch.zeros(())
    for p in params:
        if not p.grad.is_contiguous() or p.grad.dtype != torch.float32:
            raise RuntimeError("clip_grad_norm_: gradients must be contiguous float32 tensors")
    lib = _lib.load()
    dev = params[0].grad.device
    items = (_lib.VecItem * len(params))(*[(dev_ptr(p.grad), p.grad.numel()) for p in params])
    need = int(lib.lstc_sqnorm_multi_scratch(items, len(params)))
    scratch = torch.empty((need + 2,), device=dev, dtype=torch.float32)       # [partials..., sum of squares, total norm]
    sq = scratch[need:]
    check(lib.lstc_sqnorm_multi(items, len(params), dev_ptr(scratch), need, dev_ptr(sq), stream_ptr()), "lstc_sqnorm_multi")
    check(lib.lstc_clip_scale_multi(items, len(params), dev_ptr(sq), float(max_norm), stream_ptr()), "lstc_clip_scale_multi")
    return sq[1]
