"""Flat-buffer parameters and fused optimizers.

All parameters of the site's model(s) are re-homed into ONE contiguous fp32 buffer (16-byte
aligned per tensor) and their ``.grad`` into a matching flat gradient buffer.  Consequences:

* the dSGD all-reduce is one collective on one buffer (or a few buckets) with zero packing;
* Adam is a single fused HIP launch over the whole model (``csrc/kernels/optim.hip``);
* checkpoints still save per-module ``state_dict``s with the reference key names.

Semantics match ``torch.optim.Adam`` / ``torch.optim.SGD`` (checked against them in tests).
"""
from __future__ import annotations

import ctypes
import math
import os
import struct
from dataclasses import asdict, dataclass
from typing import Dict, Iterable, List, Optional, Union

import torch
import torch.nn as nn

from . import _lib

_P, _I, _L, _F, _D = _lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_float, _lib.c_double
# the device-feed arguments X ... B of the gathering launchers (DeviceSource.feed_args)
_FEED = [_P, _I, _L, _P, _P, _L, _P, _I]

_lib.register("dn_adam", [_P, _I, _P])  # (block, bump, stream)
_lib.register("dn_grad_sqnorm", [_lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_void_p])
_lib.register("dn_step_gather", _FEED + [_P, _P, _P, _L, _P, _P])
_lib.register("dn_step_prologue", [_lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_void_p,
                                   _lib.c_long, _lib.c_void_p, _lib.c_void_p, _lib.c_long,
                                   _lib.c_void_p, _lib.c_void_p])
_lib.register("dn_sgd", [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_long,
                         _lib.c_float, _lib.c_float, _lib.c_float, _lib.c_float, _lib.c_int,
                         _lib.c_void_p])
_lib.register("dn_cast_f32_bf16", [_lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_float,
                                   _lib.c_void_p])
_lib.register("dn_cast_bf16_f32", [_lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_float,
                                   _lib.c_void_p])

# (block, update, zero_grad, segs, cnt, I, Hd, HD, feed, xb, yd, sd, gofs, record, srcs, stream)
_lib.register("dn_adam_pack", [_P, _I, _I, _P, _I, _I, _I, _I] + _FEED + [_P, _P, _P, _I, _P, _P, _P])
_lib.register("dn_swap_f32", [_lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_void_p])
_lib.register("dn_step_record", [_lib.c_void_p, _lib.c_int, _lib.c_void_p])


ctypes_addr = ctypes.addressof


# host mirrors of the optim.hip structs, each checked against the library where it is filled
class _AdamArgs(ctypes.Structure):
    _fields_ = ([(k, _P) for k in ("p", "g", "m", "v", "ema")] + [("n", _L)]
                + [(k, _F) for k in ("lr", "b1", "b2", "eps", "wd", "grad_scale", "bc1",
                                     "inv_sqrt_bc2")]
                + [("b1d", _D), ("b2d", _D), ("tdev", _P), ("tofs", _I), ("pad", _I)]
                + [(k, _P) for k in ("cursor", "cs", "ls", "es")])


class _Seg(ctypes.Structure):  # PackSeg
    _fields_ = [("off", _L), ("n", _I), ("kind", _I), ("d", _I), ("dst", _P), ("dst2", _P)]


class _Src(ctypes.Structure):  # SlabSrc
    _fields_ = [("slab", _P), ("elems", _L), ("M", _I), ("N", _I), ("splits", _I), ("mode", _I),
                ("alpha", _F), ("beta", _F)]


class _Rec(ctypes.Structure):  # StepRecord
    _fields_ = [("out", _P), ("ld", _L), ("col", _I), ("B", _I), ("loss", _P), ("rs", _P),
                ("rl", _P), ("n", _L), ("cursor", _P), ("pred", _P)]


ALIGN = 4  # elements (16 bytes)

# fp64 partial sums of optim.hip ClipState (checked against the library on a GPU)
CLIP_PARTS = 256


class FlatParams:
    """Re-home ``params`` into one flat buffer; ``.grad`` of each becomes a view of ``self.grad``."""

    def __init__(self, params: Iterable[nn.Parameter], device=None):
        self.params: List[nn.Parameter] = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        device = device or self.params[0].device
        self.offsets: List[int] = []
        off = 0
        for p in self.params:
            self.offsets.append(off)
            off += (p.numel() + ALIGN - 1) // ALIGN * ALIGN
        self.numel = off
        self.data = torch.zeros(off, dtype=torch.float32, device=device)
        self.grad = torch.zeros(off, dtype=torch.float32, device=device)
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            self.data[o:o + n].copy_(p.detach().reshape(-1).float())
            p.data = self.data[o:o + n].view_as(p)
            p.grad = self.grad[o:o + n].view_as(p)

    def zero_grad(self):
        self.grad.zero_()

    def rebind_grads(self):
        """Autograd may replace ``.grad`` with a fresh tensor when it was None; keep views."""
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self.grad[o:o + n].data_ptr():
                g = p.grad
                p.grad = self.grad[o:o + n].view_as(p)
                if g is not None:
                    p.grad.copy_(g)

    def segments(self):
        for p, o in zip(self.params, self.offsets):
            yield p, o, p.numel()

    def numel_of(self, ps) -> int:
        return sum(p.numel() for p in ps)


def _check_max_norm(value) -> float:
    c = float(value)
    if not (0.0 <= c <= 3.4e38):  # (an fp32 word on the device)
        raise ValueError(f"max_grad_norm must be a finite fp32 number >= 0 (0 = off), got {value!r}")
    return c


def clip_coef(grad: torch.Tensor, grad_scale: float, max_norm: float):
    """``(coef, G)`` of global-norm clipping as the kernels compute it (optim.hip clip_coef):
    ``G = grad_scale * ||grad||_2`` from an fp64 sum of squares, ``coef = grad_scale * min(1,
    max_norm / (G + 1e-6))`` rounded to fp32 once; ``G`` rounded to fp32 (non-finite: skip)."""
    c = float(torch.tensor(float(max_norm), dtype=torch.float32))  # the device word
    gs = float(torch.tensor(float(grad_scale), dtype=torch.float32))
    Gd = gs * math.sqrt(float(grad.double().square().sum())) if grad.numel() else 0.0
    G = float(torch.tensor(Gd, dtype=torch.float32))
    coef = gs * min(1.0, c / (Gd + 1e-6)) if math.isfinite(Gd) else float("nan")
    return float(torch.tensor(coef, dtype=torch.float32)), G


# optim.hip LrState: 8 four-byte words {fp32 base, fp32 scale, fp32 lr_min, int32 kind, int32
# warmup, int32 decay_steps, fp32 applied, pad} (size checked against the library on a GPU)
LR_KINDS = {"constant": 0, "linear": 1, "cosine": 2}
_LR_BASE, _LR_SCALE, _LR_MIN, _LR_KIND, _LR_WARMUP, _LR_DECAY, _LR_APPLIED = range(7)
LR_WORDS = 8


def _f32(x: float) -> float:
    """``x`` rounded to fp32 (what a device word holds), as a Python double."""
    return struct.unpack("f", struct.pack("f", float(x)))[0]


# optim.hip EmaState: 4 four-byte words {fp32 decay, int32 warmup, fp32 applied, pad} (size
# checked against the library on a GPU)
_EMA_DECAY, _EMA_WARMUP, _EMA_APPLIED = range(3)
EMA_WORDS = 4


def _check_ema_decay(value) -> float:
    d = float(value)
    if not (d == 0.0 or (0.0 < d < 1.0 and _f32(d) < 1.0)):  # (an fp32 word on the device)
        raise ValueError(f"ema_decay must be 0 (off) or a number in (0, 1), got {value!r}")
    return d


@dataclass
class LrSchedule:
    """A learning rate as a function of the update number ``t`` (:meth:`FusedAdam.lr_at`):
    ``warmup_steps`` updates of linear warmup, then ``kind`` (``constant`` / ``linear`` /
    ``cosine``) decay to ``lr_min`` at update ``decay_steps``.  ``decay_steps=None``: not known
    yet (no decay until :meth:`FusedAdam.set_decay_steps`)."""
    kind: str = "constant"
    warmup_steps: int = 0
    decay_steps: Optional[int] = None
    lr_min: float = 0.0

    @staticmethod
    def of(spec: Union["LrSchedule", Dict, str]) -> "LrSchedule":
        if isinstance(spec, LrSchedule):
            return LrSchedule(**asdict(spec))
        if isinstance(spec, str):
            return LrSchedule(kind=spec)
        if isinstance(spec, dict):
            unknown = set(spec) - {"kind", "warmup_steps", "decay_steps", "lr_min"}
            if unknown:
                raise ValueError(f"lr_schedule: unknown entries {sorted(unknown)}")
            return LrSchedule(**spec)
        raise ValueError(f"lr_schedule must be an LrSchedule, a dict or a kind name, got {spec!r}")

    def check(self, lr: float) -> "LrSchedule":
        if self.kind not in LR_KINDS:
            raise ValueError(f"lr_schedule kind must be one of {sorted(LR_KINDS)}, got {self.kind!r}")
        for name in ("warmup_steps", "decay_steps"):
            v = getattr(self, name)
            if v is None and name == "decay_steps":
                continue
            if isinstance(v, bool) or not isinstance(v, int) or not (0 <= v < 2 ** 31):
                raise ValueError(f"lr_schedule {name} must be an integer >= 0, got {v!r}")
        if isinstance(self.lr_min, bool) or not (0.0 <= float(self.lr_min) <= float(lr)):
            raise ValueError(f"lr_schedule lr_min must lie in [0, lr = {lr!r}], got {self.lr_min!r}")
        if (self.kind != "constant" and self.decay_steps is not None
                and self.decay_steps <= self.warmup_steps):
            raise ValueError(f"lr_schedule decay_steps ({self.decay_steps}) must exceed "
                             f"warmup_steps ({self.warmup_steps}) for a {self.kind} decay")
        return self


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class FusedAdam:
    """``torch.optim.Adam`` on a :class:`FlatParams` buffer in one kernel launch per step.

    ``max_grad_norm = c > 0``: global-norm clipping on the device, the same on every step form.
    ``G = grad_scale * ||flat.grad||_2`` (fp64 sum of squares in a fixed order) and the gradient
    scale becomes ``grad_scale * min(1, c / (G + 1e-6))`` (``torch.nn.utils.clip_grad_norm_``),
    rounded to fp32 once, so ``G <= c`` leaves the update bit-identical to the unclipped one.  A
    non-finite ``G`` skips the update -- parameters and both moments untouched, ``skipped_steps``
    advanced -- while everything else the launch does (gradient zeroed, images rewritten, next
    batch gathered, cursor and step number advanced) still happens.  ``None``: the
    ``DINUNET_MAX_GRAD_NORM`` switch, else off; ``0``: off.  On / off is fixed here (it changes
    what is launched); the threshold itself lives on the device and may change between replays of
    a captured graph.

    ``lr_schedule`` (an :class:`LrSchedule`, a dict of its fields or a kind name): the rate of
    update ``t`` is :meth:`lr_at` -- warmup, decay and the plateau multiplier ``lr_scale`` --
    evaluated on the device in the prologue of the Adam launch from the same update number as the
    bias corrections, the same on every step form; ``applied_lr`` holds the rate the last update
    used.  An update skipped by the clipping still consumes its number, so the schedule advances.
    ``None``: the ``DINUNET_LR_SCHEDULE`` switch (``constant|linear|cosine``; the decaying kinds
    run to ``DINUNET_LR_DECAY_STEPS``, default 10000), else off.  On / off is fixed here (it
    changes what is launched); ``lr``, ``lr_scale`` and the schedule's numbers live on the device,
    so they may change between replays of a captured graph.  ``constant`` with no warmup and
    ``lr_scale`` 1 is bit-identical to the schedule being off.

    ``ema_decay = d`` in (0, 1): ``ema``, an exponential moving average of the parameters
    (``e_0 = p_0``), follows every update inside the same launch, ``e += (1 - d_t) (p - e)`` from
    the registers that hold the new ``p``, with ``d_t`` = :meth:`ema_decay_at` of the update number
    the bias corrections use (``ema_warmup``: ``min(d, (1 + t) / (10 + t))``), the same on every
    step form; ``applied_ema_decay`` holds the decay the last average used.  A skipped update and
    a priming launch leave ``ema`` alone (the skipped update still consumes its number).
    :meth:`swap_ema` / :meth:`ema_weights` exchange parameters and average in place, which is how
    an evaluation reads the average.  ``None``: the ``DINUNET_EMA_DECAY`` switch, else off; ``0``:
    off.  On / off is fixed here (it changes what is launched); the decay lives on the device and
    may change between replays of a captured graph."""

    def __init__(self, flat: FlatParams, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, max_grad_norm: Optional[float] = None,
                 lr_schedule: Union[LrSchedule, Dict, str, None] = None,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True):
        self.flat = flat
        self._lrs: Optional[torch.Tensor] = None  # schedule state (optim.hip LrState)
        self._lr = float(lr)
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(flat.data)
        self.exp_avg_sq = torch.zeros_like(flat.data)
        self.step_count = 0
        self._tdev: Optional[torch.Tensor] = None  # device step counter (graph-captured steps)
        # device-fed batches (ops.DeviceSource): the update advances the source's cursor
        self.cursor: Optional[torch.Tensor] = None
        self.drop_slabs()
        if max_grad_norm is None:
            env = os.environ.get("DINUNET_MAX_GRAD_NORM", "")
            max_grad_norm = float(env) if env else 0.0
        c = _check_max_norm(max_grad_norm)
        # clip state (optim.hip ClipState): [CLIP_PARTS] fp64 partials, then the words
        # {fp32 threshold, fp32 last norm, int32 skipped, pad}
        self._clip: Optional[torch.Tensor] = None
        self._max_grad_norm = c if c > 0 else None
        if c > 0:
            self._clip = self._state_block(CLIP_PARTS + 2, "dn_clip_state_size", torch.float64,
                                           "clip state", dn_clip_parts=CLIP_PARTS)
            self._clip_f = self._clip[CLIP_PARTS:].view(torch.float32)
            self._clip_i = self._clip[CLIP_PARTS:].view(torch.int32)
            self._clip_f[0] = c
        if lr_schedule is None:
            env = os.environ.get("DINUNET_LR_SCHEDULE", "")
            if env:
                lr_schedule = LrSchedule(kind=env)
                if env != "constant":
                    lr_schedule.decay_steps = int(os.environ.get("DINUNET_LR_DECAY_STEPS", "")
                                                  or 10000)
        self._sched: Optional[LrSchedule] = None
        self._lr_scale = 1.0
        self.plateau_wait = 0  # validations without improvement (plateau_step)
        if lr_schedule is not None:
            self._sched = LrSchedule.of(lr_schedule).check(self._lr)
            self._lrs = self._state_block(LR_WORDS, "dn_lr_state_size", torch.int32, "lr state")
            self._lrs_f = self._lrs.view(torch.float32)
            self._write_lr_state()
        if ema_decay is None:
            env = os.environ.get("DINUNET_EMA_DECAY", "")
            ema_decay = float(env) if env else 0.0
        d = _check_ema_decay(ema_decay)
        self.ema: Optional[torch.Tensor] = None  # the average (fp32, like flat.data)
        self._emas: Optional[torch.Tensor] = None  # its device block (optim.hip EmaState)
        self._ema_decay = d if d > 0 else None
        self._ema_warmup = bool(ema_warmup)
        self._swapped = False  # flat.data holds the average, ema the raw parameters
        if d > 0:
            self._emas = self._state_block(EMA_WORDS, "dn_ema_state_size", torch.int32,
                                           "ema state")
            self.ema = flat.data.detach().clone()
            self._emas_f = self._emas.view(torch.float32)
            self._write_ema_state()

    def _state_block(self, words: int, size_symbol: str, dtype, what: str,
                     **counts) -> torch.Tensor:
        """A zeroed device state block of ``words`` ``dtype`` words (optim.hip ClipState / LrState
        / EmaState), its layout checked against the library (``_lib.checked_struct``)."""
        block = torch.zeros(words, dtype=dtype, device=self.flat.data.device)
        if block.is_cuda:
            _lib.checked_struct(words * block.element_size(), size_symbol, what, **counts)
        return block

    # weight average -----------------------------------------------------------------------------
    def _write_ema_state(self):
        """The host-written words of the device block (one small copy)."""
        w = struct.pack("fi", self._ema_decay, int(self._ema_warmup))
        self._emas[:_EMA_APPLIED].copy_(torch.tensor(struct.unpack("2i", w), dtype=torch.int32))

    def _need_ema(self, what: str):
        if self.ema is None:
            raise ValueError(f"FusedAdam.{what}: the weight average is switched on or off when "
                             "the optimizer is built (it changes what is launched)")

    @property
    def ema_decay(self) -> Optional[float]:
        """The configured decay (None with the average off)."""
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value: Optional[float]):
        on = value is not None and _check_ema_decay(value) > 0
        if on != (self.ema is not None):
            raise ValueError("FusedAdam.ema_decay: the weight average is switched on or off when "
                             "the optimizer is built (it changes what is launched)")
        if not on:
            return
        self._refuse_in_capture("ema_decay")
        self._ema_decay = float(value)
        self._write_ema_state()

    @property
    def ema_warmup(self) -> bool:
        return self._ema_warmup

    @property
    def applied_ema_decay(self) -> Optional[torch.Tensor]:
        """fp32 [] on the optimizer's device: the decay the last average used (None with the
        average off)."""
        return None if self._emas is None else self._emas_f[_EMA_APPLIED]

    def ema_decay_at(self, t: int) -> float:
        """The decay of update number ``t`` (1-based) as the kernels compute it (optim.hip
        ema_omd), in double from the fp32 device word: ``min(d, (1 + t) / (10 + t))`` with the
        warmup on, else ``d``.  The kernels multiply by ``fp32(1 - d_t)``."""
        self._need_ema("ema_decay_at")
        d, t = _f32(self._ema_decay), float(int(t))
        return min(d, (1.0 + t) / (10.0 + t)) if self._ema_warmup else d

    def swap_ema(self):
        """Exchange the parameters and their average in place (``dn_swap_f32``, no third
        buffer): after it the model computes with the average and ``ema`` holds the raw
        parameters; twice restores both bit for bit.  No ``step*`` while swapped."""
        self._need_ema("swap_ema")
        if _capturing():
            # the exchange would become a graph node that swaps again at every replay
            raise RuntimeError("FusedAdam.swap_ema inside a HIP graph capture")
        d = self.flat.data
        if d.is_cuda:
            _lib.call("dn_swap_f32", d.data_ptr(), self.ema.data_ptr(), d.numel(), _lib.stream())
        else:
            tmp = d.clone()
            d.copy_(self.ema)
            self.ema.copy_(tmp)
        self._swapped = not self._swapped

    def ema_weights(self):
        """``with opt.ema_weights():`` -- the parameters are the average inside the scope and
        are swapped back when it ends, however it ends."""
        import contextlib
        self._need_ema("ema_weights")

        @contextlib.contextmanager
        def scope():
            self.swap_ema()
            try:
                yield self
            finally:
                self.swap_ema()
        return scope()

    def _refuse_swapped(self):
        if self._swapped:
            raise RuntimeError("FusedAdam: no update while the parameters are swapped with "
                               "their average (swap_ema / ema_weights)")

    # learning-rate schedule ---------------------------------------------------------------------
    def _write_lr_state(self):
        """All host-written words of the device block from the host values (one small copy)."""
        sc = self._sched
        w = struct.pack("fffiii", self._lr, self._lr_scale, sc.lr_min, LR_KINDS[sc.kind],
                        sc.warmup_steps, sc.decay_steps or 0)
        self._lrs[:_LR_APPLIED].copy_(torch.tensor(struct.unpack("6i", w), dtype=torch.int32))

    def _refuse_in_capture(self, what: str):
        if (self._lrs is not None or self._emas is not None) and _capturing():
            # the write would become a graph node that resets the value at every replay
            raise RuntimeError(f"FusedAdam.{what} set inside a HIP graph capture")

    @property
    def lr(self) -> float:
        return self._lr

    @lr.setter
    def lr(self, value: float):
        value = float(value)
        if self._lrs is None:
            self._lr = value
            return
        self._refuse_in_capture("lr")
        if not (self._sched.lr_min <= value):
            raise ValueError(f"FusedAdam.lr {value!r} is below the schedule's lr_min "
                             f"{self._sched.lr_min!r}")
        self._lr = value
        self._write_lr_state()

    @property
    def lr_schedule(self) -> Optional[LrSchedule]:
        """The schedule as built (a copy), None with the schedule off."""
        return None if self._sched is None else LrSchedule.of(self._sched)

    def _need_schedule(self, what: str):
        if self._lrs is None:
            raise ValueError(f"FusedAdam.{what}: the schedule is switched on or off when the "
                             "optimizer is built (it changes what is launched)")

    @property
    def lr_scale(self) -> float:
        """The plateau multiplier on the scheduled rate (1 with the schedule off)."""
        return self._lr_scale

    @lr_scale.setter
    def lr_scale(self, value: float):
        self._need_schedule("lr_scale")
        value = float(value)
        if not (0.0 < value <= 3.4e38):
            raise ValueError(f"FusedAdam.lr_scale must be a finite number > 0, got {value!r}")
        self._refuse_in_capture("lr_scale")
        self._lr_scale = value
        self._write_lr_state()

    def set_decay_steps(self, steps: int):
        """The update number at which the decay reaches ``lr_min``."""
        self._need_schedule("set_decay_steps")
        sc = LrSchedule.of(self._sched)
        sc.decay_steps = steps if steps is None else int(steps)
        sc.check(self._lr)
        self._refuse_in_capture("decay_steps")
        self._sched = sc
        self._write_lr_state()

    @property
    def applied_lr(self) -> Optional[torch.Tensor]:
        """fp32 [] on the optimizer's device: the rate the last update used (None with the
        schedule off)."""
        return None if self._lrs is None else self._lrs_f[_LR_APPLIED]

    def lr_at(self, t: int) -> float:
        """The rate of update number ``t`` (1-based) as the kernels compute it (optim.hip
        sched_lr): from the fp32 device words, in double, rounded to fp32 once::

            w = t / W if t < W else 1
            u = clamp((t - W) / (T - W), 0, 1)
            d = 1 | 1 - (1 - r) u | r + (1 - r) 0.5 (1 + cos(pi u)),  r = lr_min / base
            lr = fp32(((base * scale) * w) * d)

        With the schedule off this is ``lr``."""
        if self._sched is None:
            return self._lr
        sc = self._sched
        base, scale, t = _f32(self._lr), _f32(self._lr_scale), int(t)
        W, T = sc.warmup_steps, sc.decay_steps or 0
        w = t / W if t < W else 1.0
        d = 1.0
        if sc.kind != "constant" and T > W:
            u = min(max((t - W) / (T - W), 0.0), 1.0)
            r = _f32(sc.lr_min) / base if base > 0.0 else 1.0
            d = (1.0 - (1.0 - r) * u if sc.kind == "linear"
                 else r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * u)))
        return _f32(((base * scale) * w) * d)

    def plateau_step(self, improved: bool, factor: float, patience: int) -> bool:
        """Reduce-on-plateau bookkeeping for one validation result: an improvement resets the
        counter, anything else advances it, and once it exceeds ``patience`` the multiplier
        becomes ``max(lr_scale * factor, lr_min / lr)`` and the counter restarts.  True when
        this call reduced (or tried to: at the floor the multiplier stays)."""
        self._need_schedule("plateau_step")
        if improved:
            self.plateau_wait = 0
            return False
        self.plateau_wait += 1
        if self.plateau_wait <= int(patience):
            return False
        self.plateau_wait = 0
        floor = self._sched.lr_min / self._lr if self._lr > 0 else 0.0
        self.lr_scale = max(self._lr_scale * float(factor), floor)
        return True

    # global-norm clipping ----------------------------------------------------------------------
    @property
    def max_grad_norm(self) -> Optional[float]:
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value: Optional[float]):
        on = value is not None and _check_max_norm(value) > 0
        if on != (self._clip is not None):
            raise ValueError("FusedAdam.max_grad_norm: clipping is switched on or off when the "
                             "optimizer is built (it changes what is launched)")
        if not on:
            return
        if _capturing():
            # the write would become a graph node that resets the threshold at every replay
            raise RuntimeError("FusedAdam.max_grad_norm set inside a HIP graph capture")
        self._max_grad_norm = float(value)
        self._clip_f[0] = float(value)

    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """fp32 [] on the optimizer's device: ``G`` of the last update (None with clipping off)."""
        return None if self._clip is None else self._clip_f[1]

    @property
    def skipped_steps(self) -> Optional[torch.Tensor]:
        """int32 [] on the optimizer's device: updates skipped for a non-finite ``G``."""
        return None if self._clip is None else self._clip_i[2]

    def _sqnorm(self) -> Optional[int]:
        """Launch the squared-norm partials of the gradient; the clip state for the Adam launch."""
        if self._clip is None:
            return None
        _lib.call("dn_grad_sqnorm", self.flat.grad.data_ptr(), self.flat.grad.numel(),
                  self._clip.data_ptr(), _lib.stream())
        return self._clip.data_ptr()

    def zero_grad(self, set_to_none: bool = False):
        self.flat.zero_grad()

    def _adam_args(self, grad_scale: float, clip: Optional[int], tofs: int,
                   bc=None) -> _AdamArgs:
        """The launch's argument block (optim.hip AdamArgs).  ``clip``: what :meth:`_sqnorm`
        returned.  The update number is ``tofs`` past the device counter -- or, with ``bc`` (the
        host's ``(bc1, 1 / sqrt(bc2))``), ``tofs`` itself."""
        f, (b1, b2) = self.flat, self.betas
        tdev, bc = (None, bc) if bc else (self._tdev.data_ptr(), (1.0, 1.0))
        return _lib.checked_struct(_AdamArgs, "dn_adam_args_size", "adam argument block")(
            f.data.data_ptr(), f.grad.data_ptr(), self.exp_avg.data_ptr(),
            self.exp_avg_sq.data_ptr(), _lib.ptr(self.ema), f.data.numel(), self.lr, b1, b2,
            self.eps, self.weight_decay, grad_scale, *bc, b1, b2, tdev, tofs, 0,
            _lib.ptr(self.cursor), clip, _lib.ptr(self._lrs), _lib.ptr(self._emas))

    def step(self, grad_scale: float = 1.0):
        self._refuse_swapped()
        self.step_count += 1
        b1, b2 = self.betas
        bc1 = 1 - b1 ** self.step_count
        bc2 = 1 - b2 ** self.step_count
        d = self.flat.data
        if d.is_cuda:
            # (the number only matters to the schedule and the average)
            tofs = self.step_count if (self._lrs is not None or self._emas is not None) else 1
            args = self._adam_args(grad_scale, self._sqnorm(), tofs,
                                   bc=(bc1, 1.0 / math.sqrt(bc2)))
            _lib.call("dn_adam", ctypes_addr(args), 0, _lib.stream())
            return
        lr = self.lr_at(self.step_count)
        if self._lrs is not None:  # (recorded for a skipped update too: it consumed its number)
            self._lrs_f[_LR_APPLIED] = lr
        if self._clip is not None:
            grad_scale, G = clip_coef(self.flat.grad, grad_scale, self._max_grad_norm)
            self._clip_f[1] = G
            if not math.isfinite(G):
                self._clip_i[2] += 1
                return
        g = self.flat.grad * grad_scale
        if self.weight_decay:
            g = g + self.weight_decay * d
        self.exp_avg.mul_(b1).add_(g, alpha=1 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
        denom = (self.exp_avg_sq.sqrt() / math.sqrt(bc2)).add_(self.eps)
        d.addcdiv_(self.exp_avg, denom, value=-lr / bc1)
        if self.ema is not None:  # (not reached by a skipped update)
            dt = self.ema_decay_at(self.step_count)
            self._emas_f[_EMA_APPLIED] = dt
            self.ema.add_((d - self.ema) * _f32(1.0 - dt))

    # HIP-graph form --------------------------------------------------------------------------
    def sync_device_step(self):
        """Copy the host step count to the device counter :meth:`step_graphable` reads."""
        if _capturing():
            # inside a capture the fill (and a first allocation) would become graph nodes that
            # reset the counter at every replay
            raise RuntimeError("FusedAdam.sync_device_step inside a HIP graph capture")
        if self._tdev is None:
            self._tdev = torch.zeros(1, dtype=torch.int32, device=self.flat.data.device)
        self._tdev.fill_(self.step_count)

    def step_graphable(self, grad_scale: float = 1.0, prebumped: bool = False):
        """One Adam step whose bias corrections come from the device step counter (advanced by
        the same launch), so it can be captured once and replayed every step.  The caller keeps
        ``step_count`` in sync (one increment per replay).  ``prebumped``: the caller advances
        the counter in its step prologue instead (it passes :meth:`device_step` to the
        prologue launch before each replay), so the update is ONE graph node, not Adam + a
        one-thread bump kernel."""
        self._refuse_swapped()
        if self._tdev is None:
            self.sync_device_step()
        args = self._adam_args(grad_scale, self._sqnorm(), 0 if prebumped else 1)
        _lib.call("dn_adam", ctypes_addr(args), int(not prebumped), _lib.stream())

    # Adam that also emits the next step's operands (optim.hip adam_pack_kernel) ------------------
    def attach_pack(self, pack, src=None, xb: Optional[torch.Tensor] = None,
                    yd: Optional[torch.Tensor] = None, sd: Optional[torch.Tensor] = None,
                    copy_x: bool = True):
        """Keep ``pack`` (``ops.lstm.PersistentPack``) current from every :meth:`step_pack`, and
        gather the next batch of ``src`` (``DeviceSource``) into ``xb`` / ``yd`` there too.
        ``sd`` (int64 [B + 1]): the next batch's dataset rows go there as well; ``copy_x=False``
        then skips the batch copy (the GEMMs read the rows in place: ``ops.gemm.rows_from``)."""
        rows = pack.rows(self.flat)
        _lib.checked_struct(_Seg, "dn_pack_seg_size", "pack segment")
        tab = (_Seg * max(1, len(rows)))()
        for i, (off, n, kind, d, dst, dst2) in enumerate(rows):
            tab[i] = _Seg(off, n, kind, d, dst, dst2 or None)
        if not copy_x and sd is None:
            raise ValueError("attach_pack: without the batch copy the step needs its row indices")
        self._pack = (pack, tab, len(rows), src, xb, yd, sd, copy_x)
        self._pack_rows = rows
        self.drop_slabs()

    # split-K slab sources: the update sums the weight-gradient partials itself -------------------
    def slab_sink(self):
        """The ``ops._grad.arm_slabs`` sink of a step that ends in :meth:`step_pack`: a split
        weight-gradient launch whose every problem writes exactly one pack segment's gradient
        (``ops.slabsrc.match``) skips its ``gemm_splitk_reduce``; :meth:`step_pack` then builds
        those segments' gradients from the slabs (``optim.hip slab_grad``: the reduce's sums and
        epilogue, operation for operation) instead of reading ``flat.grad``, which for them still
        holds the zero the previous update wrote.  Anything else -- clipping (the norm needs the
        finished gradient first), a descriptor that fits no segment, the 128 / 256 tiles -- is
        refused and keeps the reduce launch.  The step calls :meth:`drop_slabs` when it ends."""
        return self._accept_slabs

    def _accept_slabs(self, descs, slab) -> bool:
        if self._clip is not None or getattr(self, "_pack", None) is None:
            return False
        from . import slabsrc
        from .lstm import _row_map
        pack = self._pack[0]
        dev = self.flat.grad.device
        got = slabsrc.match(descs, self._pack_rows, self.flat.grad.data_ptr(), pack.I, pack.Hd,
                            pack.HD, _row_map(pack.Hd, pack.HD, dev).data_ptr(),
                            taken=self._slab_srcs)
        if got is None:
            return False
        self._slab_srcs.update(got)
        self._slab_keep.append(slab)  # alive, at its address, until step_pack has been issued
        return True

    def drop_slabs(self):
        """Forget accepted slab sources (:meth:`step_pack` consumed them, or the step failed)."""
        self._slab_srcs = {}
        self._slab_keep = []

    def _slab_table(self, cnt: int):
        """The ``optim.hip SlabSrc`` rows by segment for the accepted sources."""
        _lib.checked_struct(_Src, "dn_slab_src_size", "slab source")
        tab = (_Src * max(1, cnt))()
        for i, s in self._slab_srcs.items():
            tab[i] = _Src(s.slab, s.slab_elems, s.M, s.N, s.splits, s.mode, s.alpha, s.beta)
        return tab

    def step_pack(self, grad_scale: float = 1.0, update: bool = True, gofs: int = 1,
                  record=None):
        """ONE launch: the graph-capturable Adam step (bias corrections from the device counter,
        which the step's first GEMM advanced: ``dn_gemm_arm_bump``), the attached packed images
        rewritten from the updated parameters, the gradient zeroed, and the batch at
        ``cursor + gofs`` gathered.  ``update=False``: images + gather + zeroing only (priming).
        ``record``: a :meth:`StepRecorder.args` struct -- the step's score column and loss go to
        the recorder's rings at the cursor (one more workgroup of the same launch)."""
        self._refuse_swapped()
        pack, tab, cnt, src, xb, yd, sd, copy_x = self._pack
        if self._tdev is None:
            self.sync_device_step()
        if src is not None:
            gx = src.feed_args(xb) + [xb.data_ptr() if copy_x else None, yd.data_ptr(),
                                      _lib.ptr(sd)]
        else:
            gx = [None, 0, 0, None, None, 1, None, 0, None, None, None]
        clip = self._sqnorm() if update else None
        srcs = None
        if self._slab_srcs:
            if not update or clip is not None:
                raise RuntimeError("FusedAdam.step_pack: slab sources were accepted for a launch "
                                   "that cannot sum them (no update, or a clipped one)")
            srcs = self._slab_table(cnt)
        try:
            args = self._adam_args(grad_scale, clip, 0)
            _lib.call("dn_adam_pack", ctypes_addr(args), int(update), 1, ctypes_addr(tab), cnt,
                      pack.I, pack.Hd, pack.HD, *gx, int(gofs),
                      ctypes_addr(record) if (record is not None and update) else None,
                      ctypes_addr(srcs) if srcs is not None else None, _lib.stream())
        finally:
            self.drop_slabs()  # (the launch is in the stream: the slabs may be reused after it)

    def device_step(self) -> torch.Tensor:
        """The device step counter (int32[1]) the graph-captured update reads; a step prologue
        given it advances it once per launch."""
        if self._tdev is None:
            self.sync_device_step()  # (raises inside a capture: create it before)
        return self._tdev

    def state_dict(self) -> Dict:
        sd = {"lr": self.lr, "betas": self.betas, "eps": self.eps,
              "weight_decay": self.weight_decay, "step": self.step_count,
              "exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu()}
        if self._clip is not None:
            sd["max_grad_norm"] = self._max_grad_norm
            sd["skipped"] = int(self.skipped_steps.item())
        if self._sched is not None:
            sd["lr_schedule"] = asdict(self._sched)
            sd["lr_scale"] = self._lr_scale
            sd["plateau_wait"] = int(self.plateau_wait)
        if self.ema is not None:
            if self._swapped:
                raise RuntimeError("FusedAdam.state_dict while the parameters are swapped with "
                                   "their average")
            sd["ema"] = self.ema.detach().cpu()
            sd["ema_decay"] = self._ema_decay
            sd["ema_warmup"] = self._ema_warmup
        return sd

    def load_state_dict(self, sd: Dict):
        if self._sched is not None:  # (on / off stays as built; older checkpoints carry none)
            if sd.get("lr_schedule"):
                self._sched = LrSchedule.of(dict(sd["lr_schedule"])).check(
                    float(sd.get("lr", self._lr)))
            self._lr_scale = float(sd.get("lr_scale", self._lr_scale))
            self.plateau_wait = int(sd.get("plateau_wait", self.plateau_wait))
        self.lr = sd.get("lr", self.lr)
        self.betas = tuple(sd.get("betas", self.betas))
        self.eps = sd.get("eps", self.eps)
        self.weight_decay = sd.get("weight_decay", self.weight_decay)
        self.step_count = int(sd.get("step", 0))
        if "exp_avg" in sd:
            self.exp_avg.copy_(sd["exp_avg"].to(self.exp_avg.device))
            self.exp_avg_sq.copy_(sd["exp_avg_sq"].to(self.exp_avg_sq.device))
        if self._clip is not None:  # (on / off stays as built; older checkpoints carry neither)
            if sd.get("max_grad_norm"):
                self.max_grad_norm = float(sd["max_grad_norm"])
            if "skipped" in sd:
                self._clip_i[2] = int(sd["skipped"])
        if self.ema is not None:  # (on / off stays as built)
            self._refuse_swapped()
            if "ema" in sd:
                self.ema.copy_(sd["ema"].to(self.ema.device))
                self._ema_warmup = bool(sd.get("ema_warmup", self._ema_warmup))
                if sd.get("ema_decay"):
                    self._ema_decay = _check_ema_decay(sd["ema_decay"])
                self._write_ema_state()
            else:  # an older checkpoint: the built values, the average restarts at the parameters
                self.ema.copy_(self.flat.data)


def step_prologue(x: torch.Tensor, xb: Optional[torch.Tensor], y: torch.Tensor,
                  yd: torch.Tensor, grad: torch.Tensor, bump: Optional[torch.Tensor] = None):
    """ONE launch before a graph replay: ``xb <- bf16(x)`` (skipped when ``xb`` is None),
    ``yd <- y`` (int64), ``grad <- 0`` and, when given, ``bump += 1`` (the captured Adam's
    device step counter, :meth:`FusedAdam.device_step`)."""
    nx = x.numel() if xb is not None else 0
    if nx % 8 or grad.numel() % 4 or y.dtype != torch.int64 or yd.dtype != torch.int64:
        raise ValueError("step_prologue: x numel % 8, grad numel % 4 and int64 labels required")
    _lib.call("dn_step_prologue", x.data_ptr() if nx else None, nx,
              xb.data_ptr() if nx else None, y.data_ptr(), y.numel(), yd.data_ptr(),
              grad.data_ptr(), grad.numel(), _lib.ptr(bump), _lib.stream())


def cast_f32_to_bf16(src: torch.Tensor, dst: torch.Tensor, scale: float = 1.0):
    if src.is_cuda:
        _lib.call("dn_cast_f32_bf16", src.data_ptr(), dst.data_ptr(), src.numel(), scale,
                  _lib.stream())
    else:
        dst.copy_((src * scale).to(dst.dtype))


def cast_bf16_to_f32(src: torch.Tensor, dst: torch.Tensor, scale: float = 1.0):
    if src.is_cuda:
        _lib.call("dn_cast_bf16_f32", src.data_ptr(), dst.data_ptr(), src.numel(), scale,
                  _lib.stream())
    else:
        dst.copy_(src.float() * scale)


class DeviceSource:
    """Training batches resident in HBM (BASELINE config 5 sizing: a site's whole dataset fits one
    MI355X): ``X [N, *sample]`` (bf16, or fp32), labels ``Y [N]`` int64, an optional per-pass order
    ``[nb * B]`` of row indices, and a device batch cursor.  Step ``c`` trains on rows
    ``order[(c mod nb) * B : ... + B]``; the gather runs in the step's first launch and the cursor
    advances in its Adam launch, so a HIP graph can hold several whole steps
    (``runtime.step.TrainStep.run``)."""

    def __init__(self, X: torch.Tensor, Y: torch.Tensor, batch: int,
                 order: Optional[torch.Tensor] = None):
        if not X.is_cuda or X.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("DeviceSource: X must be a bf16 / fp32 GPU tensor")
        self.width = None  # the real feature count of a padded fp32 feature matrix
        if X.dtype == torch.float32 and X.dim() == 2 and X.shape[1] % 8:
            # fp32 feature rows (FS: 66 features) padded with zero columns to whole 16-B chunks
            # once; the step's static input keeps the padded width and the model reads the
            # first `width` columns (``view``)
            self.width = int(X.shape[1])
            Xp = torch.zeros(X.shape[0], -(-X.shape[1] // 8) * 8, dtype=X.dtype, device=X.device)
            Xp[:, :self.width] = X
            X = Xp
        self.X = X.contiguous()
        self.Y = Y.to(device=X.device, dtype=torch.int64).contiguous()
        self.B = int(batch)
        self.row = self.X[0].numel()
        if self.row % 8:
            raise ValueError("DeviceSource: sample size must be a multiple of 8 elements")
        self.order = None
        self.set_order(order)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=X.device)

    def set_order(self, order: Optional[torch.Tensor]):
        """A new pass order (e.g. the next epoch's shuffle) in place: captured graphs keep
        reading the same buffer."""
        n = self.X.shape[0] if order is None else order.numel()
        nb = n // self.B
        if nb < 1:
            raise ValueError("DeviceSource: fewer samples than one batch")
        if order is None:
            self.order = None
        else:
            o = order.to(device=self.X.device, dtype=torch.int64).reshape(-1)[:nb * self.B]
            if self.order is not None and self.order.numel() == o.numel():
                self.order.copy_(o)
            else:
                self.order = o.clone()
        self.nb = nb

    @property
    def sample_shape(self):
        return tuple(self.X.shape[1:])

    def batch(self, c: int):
        """Host-side view of batch ``c`` (tests / eager fallbacks): ``(x, y)``."""
        j = (c % self.nb) * self.B
        rows = (self.order[j:j + self.B] if self.order is not None
                else torch.arange(j, j + self.B, device=self.X.device))
        return self.X[rows], self.Y[rows]

    def view(self, xb: torch.Tensor) -> torch.Tensor:
        """What the model reads of a static input ``xb`` this source gathers into (the real
        columns of padded feature rows)."""
        return xb if self.width is None else xb[:, :self.width]

    def _mode(self, xb: torch.Tensor) -> int:
        # dn_step_gather's source / destination mode (prologue.h): 1 bf16 -> bf16, 0 fp32 ->
        # bf16 (rounded), 2 fp32 -> fp32 (exact)
        if self.X.dtype == torch.bfloat16:
            if xb.dtype != torch.bfloat16:
                raise ValueError("DeviceSource: a bf16 dataset gathers into a bf16 static input")
            return 1
        return 2 if xb.dtype == torch.float32 else 0

    def feed_args(self, xb: torch.Tensor) -> list:
        """The arguments ``X ... B`` every gathering launcher starts its device-feed tail with
        (``prologue.h prologue_gather``)."""
        return [self.X.data_ptr(), self._mode(xb), self.row, self.Y.data_ptr(),
                _lib.ptr(self.order), self.nb, self.cursor.data_ptr(), self.B]

    def gather(self, xb: torch.Tensor, yd: torch.Tensor, grad: torch.Tensor,
               bump: Optional[torch.Tensor] = None):
        """The standalone device-fed prologue launch (``dn_step_gather``)."""
        _lib.call("dn_step_gather", *self.prologue_args(xb, yd, grad, bump), _lib.stream())

    def labels_of(self, steps: int) -> torch.Tensor:
        """Labels of batches ``0 .. steps-1`` of the current order, flattened (what a
        :class:`StepRecorder`'s score ring pairs with)."""
        rows = (self.order[:steps * self.B] if self.order is not None
                else torch.arange(steps * self.B, device=self.X.device) % self.X.shape[0])
        return self.Y[rows]

    def prologue_args(self, xb, yd, grad, bump=None):
        """Argument tail of ``dn_lstm_pack_gather`` (the prologue riding in the weight pack)."""
        return self.feed_args(xb) + [xb.data_ptr(), yd.data_ptr(), grad.data_ptr(), grad.numel(),
                                     _lib.ptr(bump)]


class StepRecorder:
    """Per-step train records of device-fed steps (``runtime.feed.DeviceFeed``): ring slot
    ``c mod n`` of batch cursor ``c`` holds the step's score column ``out[:, col]`` (``[B]``; ICA:
    ``prob[:, 1]``, the reference's train-AUC input, ``comps/icalstm/__init__.py:64-65``; ``col``
    < 0: the predicted class, FS's hard-label scores, ``comps/fs/__init__.py:57-59``) and its
    loss (``:67-68``).  The write rides in the packing Adam launch (one more workgroup,
    ``optim.hip adam_pack_kernel``) or is a one-workgroup launch of its own (``dn_step_record``)
    after an update that already advanced the cursor; either way K-step graph replays keep exact
    per-sample train metrics with no host work between steps."""

    def __init__(self, n: int, B: int, cursor: torch.Tensor, col: int = 1):
        self.n, self.B, self.col = int(n), int(B), int(col)
        dev = cursor.device
        self.scores = torch.zeros(self.n, self.B, dtype=torch.float32, device=dev)
        self.losses = torch.zeros(self.n, dtype=torch.float32, device=dev)
        self.cursor = cursor
        self._cache: Dict[tuple, object] = {}

    def args(self, out: torch.Tensor, loss: torch.Tensor, pred: Optional[torch.Tensor] = None):
        """The ``StepRecord`` struct for a step whose outputs are ``out`` [B, C] / ``loss`` []
        (/ ``pred`` [B] int64, needed when ``col`` < 0).  Cached per output set: a multi-site
        step issued from the host every step asks for the same static buffers' struct each time
        (no per-step class or library query)."""
        if self.col < 0 and (pred is None or pred.dtype != torch.int64 or pred.numel() != self.B
                             or not pred.is_contiguous()):
            raise ValueError("StepRecorder(col < 0) records the predicted class: pass pred [B] int64")
        pp = pred.data_ptr() if (self.col < 0 and pred is not None) else None
        key = (out.data_ptr(), loss.data_ptr(), tuple(out.shape), pp)
        rec = self._cache.get(key)
        if rec is not None:
            return rec
        if (out.dim() != 2 or out.shape[0] != self.B or out.dtype != torch.float32
                or not out.is_contiguous() or loss.dtype != torch.float32 or loss.numel() != 1):
            raise ValueError("StepRecorder: out must be contiguous fp32 [B, C], loss fp32 scalar")
        rec = _lib.checked_struct(_Rec, "dn_step_record_size", "step record")(
            out.data_ptr(), out.shape[1], self.col, self.B, loss.data_ptr(),
            self.scores.data_ptr(), self.losses.data_ptr(), self.n, self.cursor.data_ptr(), pp)
        if len(self._cache) > 64:
            self._cache.clear()
        self._cache[key] = rec
        return rec

    def record(self, out: torch.Tensor, loss: torch.Tensor, cofs: int = -1,
               pred: Optional[torch.Tensor] = None):
        """Standalone record into slot ``(cursor + cofs) mod n``."""
        if out.is_cuda:
            rec = self.args(out, loss, pred)  # (held: the launcher reads it through its address)
            _lib.call("dn_step_record", ctypes_addr(rec), int(cofs), _lib.stream())
            return
        c = (int(self.cursor.item()) + cofs) % self.n
        self.scores[c].copy_((pred if self.col < 0 else out[:, self.col]).float())
        self.losses[c] = loss.detach().float()

    def reset(self):
        self.scores.zero_()
        self.losses.zero_()
