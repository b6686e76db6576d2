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
"""
from __future__ import annotations

import contextlib
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
        for group in self.param_groups:
            for p in group["params"]:
                self.state[p]["sum"] = torch.full_like(p, float(group["initial_accumulator_value"]),
                                                       memory_format=torch.preserve_format)
                self.state[p]["step"] = 0

    def _item(self, group, p, g, gs):
        state = self.state[p]
        state["step"] += 1
        return (dev_ptr(p.data), dev_ptr(g), dev_ptr(state["sum"]), p.numel(), float(group["lr"]),
                float(group["weight_decay"]), float(group["eps"]), gs)

    def _launch(self, lib, items):          # lstc_adagrad_multi; element arithmetic of lstc_adagrad_step
        arr = (_lib.AdagradItem * len(items))(*items)
        check(lib.lstc_adagrad_multi(arr, len(items), stream_ptr()), "lstc_adagrad_multi")


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
