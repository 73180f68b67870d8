"""Fused MLP head + loss (``csrc/kernels/mlp_head.hip``).

Covers the two classifier heads of the reference:

* ICA  (``comps/icalstm/models.py:95-103`` + ``comps/icalstm/__init__.py:59-63``):
  ``Dropout(0.25) -> Linear -> BatchNorm1d(running stats) -> ReLU -> Linear -> ReLU -> Linear``
  then softmax cross-entropy; ``out`` = probabilities.
* FS   (``comps/fs/models.py:4-31`` + ``comps/fs/__init__.py:54-57``): the whole MSANNet,
  ``[Linear(no bias) -> BatchNorm1d(batch stats) -> ReLU (-> Dropout)] x L -> fc_out`` then
  log-softmax + NLL; ``out`` = log-probabilities.

A :class:`HeadSpec` is parsed from the module sequence itself, so the fused path always matches
what the modules would compute (parameters, BN eps/momentum/mode, dropout placement); anything the
kernels do not cover (> 16 classes, layers wider than 2048, unknown modules) runs the modules +
the loss op.

``norm_layer="layer"`` heads are fused too: an ``nn.LayerNorm`` (``ops.LayerNorm`` included) after
a ``Linear`` -- 1-D ``normalized_shape == out_features``, affine with a bias, ahead of the layer's
ReLU -- is the kernels' norm mode 3 (``flags & 3``; eps in ``_bnp``, weight / bias and their
gradient buffers in the BatchNorm pointer slots, no running state, the same math in training
and evaluation, legal on one row).  Batches <= 64 normalise in the single-workgroup launches
(a wave per row), larger batches with one extra launch per LayerNorm layer each way; a bias
ahead of the norm gets its real gradient.  The one-launch replicated head (``head_rep.hip``)
takes mode 3 on layer 0 (the ICA classifier), bitwise the three-launch result; a LayerNorm on a
later layer of a hinted step runs the three-launch path.  Any other LayerNorm (no affine, no
bias, after the ReLU, N-D shape) runs the modules.

Batches above 64 rows run ``csrc/kernels/head_big.hip`` behind the same C entry points: one
launch per layer forward (row blocks x 64-column blocks, the previous layer's BatchNorm + ReLU and
this layer's dropout applied while staging the input tile) + one loss launch, one launch per
layer backward (dA and dW jobs in one grid) + one per BatchNorm layer; BatchNorm statistics are
deterministic per-row-block partials merged in a fixed order (SURVEY K7 at the large batches of
the reference's pretrain config).

For batches <= 64 the forward is two launches (the wide first layer over many workgroups, then the narrow tail +
loss in one): loss, outputs, argmax, BatchNorm running-stat update and the dropout masks
(counter-based hash; the seed is a device counter the kernel bumps, so HIP-graph replays draw
fresh masks).  The backward is two launches (the output-gradient chain, then every dW slice and
dX over many workgroups); it scales by ``dloss`` on the device, accumulates every head parameter
gradient straight into its ``.grad`` (flat-buffer view) and returns ``d input``.  Dropout masks are not bit-identical to ``torch.nn.Dropout``'s generator
stream (same distribution, independent draws); everything else matches the module math with
bf16 MFMA operands and fp32 accumulation / statistics.

Loss options: ``HeadSpec(modules, class_weights=w, label_smoothing=eps)`` makes every path
compute ``F.cross_entropy(z, y, weight=w, label_smoothing=eps)`` (mean reduction) instead of the
plain mean cross-entropy; the FS head (log-softmax + NLL) applies the same formula to its logits
(torch's ``nll_loss`` has no smoothing argument).  Outputs, ``pred``, label clamping and dropout
draws do not change.  The normalisation is per batch, as in torch: each call divides by its own
``D = sum_i w[y_i]``, so micro-batches of an accumulated step and the shards of a multi-GPU site
each normalise by their own ``D`` (torch's behaviour under DataParallel too).  The kernels read
the options from a small fp32 device block the spec owns (``csrc/kernels/loss_opt.h``), so
:meth:`HeadSpec.set_loss` takes effect in already captured graphs; whether the options are on at
all is fixed when the spec is built.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from . import _grad
from . import _lib
from . import capture as _cap
from . import reference as ref

Tensor = torch.Tensor
_MAXL = 6

_P = _lib.c_void_p
_lib.register("dn_head_layout", [_P, _P, _P, _lib.c_int, _P])
_lib.register("dn_head_fwd", [_lib.c_int, _P, _P, _P, _P, _P, _P, _lib.c_long, _lib.c_int, _P, _P,
                              _P, _P, _P, _P, _lib.c_int, _lib.c_int, _P])
_lib.register("dn_head_bwd", [_lib.c_int, _P, _P, _P, _P, _P, _lib.c_int, _P, _P, _P, _lib.c_long,
                              _P])
_lib.register("dn_head_fwd_train", [_lib.c_int, _P, _P, _P, _P, _P, _P, _lib.c_long, _lib.c_int,
                                    _P, _P, _P, _P, _P, _P, _lib.c_int, _P, _P])
_lib.register("dn_head_bwd0", [_lib.c_int, _P, _P, _P, _P, _P, _lib.c_int, _P, _P, _lib.c_long,
                               _P])
_lib.register("dn_head_rep_sync_bytes", [])
_lib.register("dn_cast_bf16_group", [_P, _P, _P, _lib.c_int, _P])
_lib.register("dn_head_rep", [_lib.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _lib.c_long, _lib.c_int,
                              _P, _P, _P, _P, _P, _P, _lib.c_int, _P, _P, _lib.c_long, _P])
_lib.register("dn_head_rep_jobs", [_lib.c_int, _P, _P, _lib.c_int, _P, _lib.c_int])
# the same entry points with the loss-option block (null = off) ahead of the stream
_lib.register("dn_head_fwd_lw", [_lib.c_int, _P, _P, _P, _P, _P, _P, _lib.c_long, _lib.c_int, _P,
                                 _P, _P, _P, _P, _P, _lib.c_int, _lib.c_int, _P, _P])
_lib.register("dn_head_fwd_train_lw", [_lib.c_int, _P, _P, _P, _P, _P, _P, _lib.c_long, _lib.c_int,
                                       _P, _P, _P, _P, _P, _P, _lib.c_int, _P, _P, _P])
_lib.register("dn_head_bwd_lw", [_lib.c_int, _P, _P, _P, _P, _P, _lib.c_int, _P, _P, _P,
                                 _lib.c_long, _lib.c_int, _P])
_lib.register("dn_head_rep_lw", [_lib.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _lib.c_long,
                                 _lib.c_int, _P, _P, _P, _P, _P, _P, _lib.c_int, _P, _P,
                                 _lib.c_long, _P, _P])

# d(loss) tensor of the running training step, when the step will backpropagate exactly that
# tensor (runtime.step.TrainStep's persistent 1): the forward then runs the head's output-gradient
# chain in the same launch (dn_head_fwd_train).  DINUNET_FUSED_HEAD=0 disables.
_HINT: Optional[torch.Tensor] = None
import os as _os
_FUSED_HEAD = _os.environ.get("DINUNET_FUSED_HEAD", "1") == "1"
# the whole training step of the head in ONE launch when the d loss is known at forward time
# (csrc/kernels/head_rep.hip: the forward REPLICATED in every workgroup, no cross-workgroup
# hand-off), reading bf16 weight images: the ones the fused Adam keeps current
# (ops.lstm.PersistentPack, device-fed steps), else the spec's own images, cast from the fp32
# weights by one launch right before (HeadSpec.own_images).  DINUNET_HEAD_STEP=0 keeps the
# three-launch path.  (Round 5's hand-off head head_step.hip, the form for steps without the
# Adam-emitted pack, is folded into this: VERDICT r5 item 7.)
_HEAD_STEP = _os.environ.get("DINUNET_HEAD_STEP", "1") == "1"


REP_LAUNCHES = 0  # head_rep.hip launches issued (tests: the replicated head really ran)


def _bf16_images(spec: "HeadSpec"):
    """The bf16 weight images of every head layer from the active persistent operand pack
    (``ops.lstm.use_persistent``), or None when any is missing."""
    from . import lstm as _lstm
    pp = _lstm._PERSIST
    if pp is None or not hasattr(pp, "bf16_of"):
        return None
    imgs = [pp.bf16_of(L.linear.weight) for L in spec.layers]
    if any(t is None for t in imgs):
        return None
    pp.used = True
    return (ctypes.c_void_p * len(imgs))(*[t.data_ptr() for t in imgs])


class loss_grad_hint:
    """``with loss_grad_hint(one): out, loss, pred = head_loss(...)`` -- then
    ``loss.backward(one)``.  A backward with any other gradient tensor stays correct (it runs
    the unfused chain); it only loses the saving."""

    def __init__(self, t: Optional[torch.Tensor]):
        self.t = t

    def __enter__(self):
        global _HINT
        self.prev, _HINT = _HINT, self.t
        return self

    def __exit__(self, *a):
        global _HINT
        _HINT = self.prev
        return False


class _Layer:
    __slots__ = ("linear", "bn", "relu", "drop")

    def __init__(self, linear: nn.Linear, drop: float):
        self.linear = linear
        self.bn: Optional[nn.Module] = None  # the layer's norm: BatchNorm1d or LayerNorm
        self.relu = False
        self.drop = drop


class HeadSpec:
    """A fusable description of ``modules`` (run in order) followed by a loss."""

    def __init__(self, modules: Sequence[nn.Module], class_weights=None,
                 label_smoothing: float = 0.0):
        self.modules = list(modules)
        self.layers: List[_Layer] = []
        self.ok = True
        lins = [m for m in self.modules if isinstance(m, nn.Linear)]
        self.num_class = lins[-1].out_features if lins else 0
        # A/B switches, read only where the argument is unset (as DINUNET_MAX_GRAD_NORM is)
        if class_weights is None and _os.environ.get("DINUNET_CLASS_WEIGHTS"):
            class_weights = _env_numbers("DINUNET_CLASS_WEIGHTS")
        if not label_smoothing and _os.environ.get("DINUNET_LABEL_SMOOTHING"):
            label_smoothing = _env_numbers("DINUNET_LABEL_SMOOTHING")[0]
        self.class_weights, self.label_smoothing = check_loss_options(
            class_weights, label_smoothing or 0.0, self.num_class)
        # on / off is fixed here (a null block pointer runs the kernels' original code)
        self.loss_on = self.class_weights is not None or self.label_smoothing != 0.0
        self._lossblk = {}  # device -> the kernels' option block
        pending = 0.0
        for m in self.modules:
            if isinstance(m, nn.Dropout):
                if pending:
                    self.ok = False
                pending = float(m.p)
            elif isinstance(m, nn.Linear):
                self.layers.append(_Layer(m, pending))
                pending = 0.0
            elif isinstance(m, nn.BatchNorm1d):
                L = self.layers[-1] if self.layers else None
                if (L is None or L.bn is not None or L.relu or not m.affine
                        or (m.track_running_stats and m.momentum is None)):
                    self.ok = False
                else:
                    L.bn = m
            elif isinstance(m, nn.LayerNorm):
                L = self.layers[-1] if self.layers else None
                if (L is None or L.bn is not None or L.relu or not m.elementwise_affine
                        or m.bias is None or m.weight is None
                        or tuple(m.normalized_shape) != (L.linear.out_features,)):
                    self.ok = False
                else:
                    L.bn = m
            elif isinstance(m, nn.ReLU):
                if not self.layers or self.layers[-1].relu:
                    self.ok = False
                else:
                    self.layers[-1].relu = True
            else:
                self.ok = False
        if pending or not self.layers or len(self.layers) > _MAXL:
            self.ok = False
        if self.ok:
            self.dims = [self.layers[0].linear.in_features] + [L.linear.out_features for L in self.layers]
            for L, d in zip(self.layers, self.dims[:-1]):
                if L.linear.in_features != d:
                    self.ok = False
        if not self.ok:
            return
        n = len(self.layers)
        self.nl = n
        self._dims = (ctypes.c_int * (n + 1))(*self.dims)
        self._flags = (ctypes.c_int * n)(*[self._bn_mode(L) | (int(L.relu) << 2) for L in self.layers])
        self._drops = (ctypes.c_float * n)(*[L.drop for L in self.layers])
        bnp = []
        for L in self.layers:
            if L.bn is None:
                bnp += [1e-5, 0.1]
            else:  # (LayerNorm has no momentum: the kernels ignore the slot in mode 3)
                bnp += [L.bn.eps, getattr(L.bn, "momentum", None) or 0.0]
        self._bnp = (ctypes.c_float * (2 * n))(*bnp)
        self._layout = {}
        self._rng: Optional[Tensor] = None
        self._rep_jobs = {}
        self._sync: Optional[Tensor] = None
        self._own = None  # (device, [bf16 images], ctypes tables) of own_images

    @staticmethod
    def _bn_mode(L: _Layer) -> int:
        if L.bn is None:
            return 0
        if isinstance(L.bn, nn.LayerNorm):
            return 3
        return 2 if L.bn.track_running_stats and L.bn.running_mean is not None else 1

    # ---- parameters / pointers --------------------------------------------------------------
    def params(self) -> List[nn.Parameter]:
        ps = []
        for L in self.layers:
            ps.append(L.linear.weight)
            if L.linear.bias is not None:
                ps.append(L.linear.bias)
            if L.bn is not None:
                ps += [L.bn.weight, L.bn.bias]
        return ps

    @property
    def training(self) -> bool:
        return any(m.training for m in self.modules)

    def layout(self, B: int):
        lay = self._layout.get(B)
        if lay is None:
            buf = (ctypes.c_long * (1 + 4 * self.nl))()
            rc = _lib.lib().dn_head_layout(self.nl, self._dims, self._flags, B, buf)
            lay = list(buf) if rc == 0 else None
            self._layout[B] = lay
        return lay

    def supported(self, x: Tensor) -> bool:
        if not (self.ok and x.is_cuda and x.dim() == 2 and x.shape[1] == self.dims[0]):
            return False
        if not _lib.native_available():
            if _lib.require_native():
                raise RuntimeError("fused head on GPU needs the gfx950 kernel library")
            return False
        B = x.shape[0]
        if B < 2 and any(self._bn_mode(L) == 1 or (self._bn_mode(L) == 2 and self.training)
                         for L in self.layers):
            return False  # BatchNorm on one sample: let the modules raise like torch does
        if any(p.dtype != torch.float32 or not p.is_contiguous() for p in self.params()):
            return False
        return self.layout(B) is not None

    def rep_jobs(self, B: int, device) -> Optional[Tensor]:
        """head_rep.hip's dW job table of batch B on ``device`` (host-decoded once, so the kernel
        does no integer division), or None outside that kernel's envelope."""
        key = (B, str(device))
        if key not in self._rep_jobs:
            cap = 1 << 14
            buf = (ctypes.c_int * cap)()
            n = int(_lib.lib().dn_head_rep_jobs(self.nl, self._dims, self._flags, B, buf, cap))
            if n < 0:
                raise RuntimeError("dn_head_rep_jobs: job table larger than its buffer")
            self._rep_jobs[key] = (torch.tensor(list(buf[:n]), dtype=torch.int32, device=device)
                                   if n > 0 else None)
        return self._rep_jobs[key]

    def sync(self, device) -> Tensor:
        """The one-launch kernel's control block (zeroed once; its done counter -- the last
        workgroup advances the dropout seed -- resets itself every launch)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._sync is None or self._sync.device != device:
            n = int(_lib.lib().dn_head_rep_sync_bytes())
            self._sync = torch.zeros(n // 4, dtype=torch.int32, device=device)
        return self._sync

    def own_images(self, device):
        """bf16 images of every layer's weight, refreshed from the fp32 weights by ONE launch on
        the current stream (captured with the step when inside a capture): the replicated head's
        operands when no Adam-emitted pack keeps images current (host-fed steps, eager paths).
        Returns the pointer table ``dn_head_rep`` takes."""
        device = torch.device(device)
        if self._own is None or self._own[0] != device:
            imgs = [torch.empty(L.linear.weight.shape, dtype=torch.bfloat16, device=device)
                    for L in self.layers]
            n = len(imgs)
            tab = (ctypes.c_void_p * n)(*[t.data_ptr() for t in imgs])
            self._own = (device, imgs, tab, (ctypes.c_long * n)(*[t.numel() for t in imgs]))
        _, imgs, tab, cnt = self._own
        src = (ctypes.c_void_p * len(imgs))(*[L.linear.weight.data_ptr() for L in self.layers])
        _lib.call("dn_cast_bf16_group", src, tab, cnt, len(imgs), _lib.stream())
        return tab

    def rng(self, device) -> Tensor:
        if self._rng is None or self._rng.device != device:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            self._rng = torch.tensor([seed], dtype=torch.int64, device=device)
        return self._rng

    def ptrs(self, with_grads: bool):
        arr = (ctypes.c_void_p * (11 * self.nl))()
        grads = []
        for l, L in enumerate(self.layers):
            lin, bn = L.linear, L.bn
            v = [lin.weight, lin.bias]
            if bn is not None:
                v += [bn.weight, bn.bias]
                if self._bn_mode(L) == 2:
                    v += [bn.running_mean, bn.running_var, bn.num_batches_tracked]
                else:
                    v += [None, None, None]
            else:
                v += [None] * 5
            g = [None] * 4
            if with_grads:
                g = [_grad.grad_buffer(lin.weight),
                     _grad.grad_buffer(lin.bias) if lin.bias is not None else None,
                     _grad.grad_buffer(bn.weight) if bn is not None else None,
                     _grad.grad_buffer(bn.bias) if bn is not None else None]
                grads += [t for t in g if t is not None]
            for j, t in enumerate(v + g):
                arr[11 * l + j] = None if t is None else t.data_ptr()
        return arr

    # ---- loss options ------------------------------------------------------------------------
    def set_loss(self, class_weights=None, label_smoothing=None):
        """Rewrite the option values in place (None keeps the current one): every device block
        keeps its address, so captured graphs compute the new objective from their next replay.
        Raises if the spec was built with the options off."""
        if not self.loss_on:
            raise RuntimeError("HeadSpec.set_loss: the spec was built without loss options "
                               "(pass class_weights / label_smoothing to the constructor)")
        w, eps = check_loss_options(
            self.class_weights if class_weights is None else class_weights,
            self.label_smoothing if label_smoothing is None else label_smoothing, self.num_class)
        self.class_weights, self.label_smoothing = w, eps
        for blk in self._lossblk.values():
            blk.copy_(self._loss_values())

    def _loss_values(self) -> Tensor:
        from .heads import loss_block_values
        return loss_block_values(self.class_weights, self.label_smoothing, self.num_class)

    def loss_block(self, device) -> Optional[Tensor]:
        """The option block on ``device`` (created on first use), None with the options off."""
        if not self.loss_on:
            return None
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        blk = self._lossblk.get(device)
        if blk is None:
            blk = self._lossblk[device] = self._loss_values().to(device)
        return blk

    def loss_kwargs(self, device) -> dict:
        """``weight`` / ``label_smoothing`` / ``block`` for ``ops.softmax_ce`` and
        ``ops.log_softmax_nll`` on the module path (CPU: ``ops.reference``; GPU: the spec's own
        block, so nothing is rebuilt per call)."""
        if not self.loss_on:
            return {}
        from .heads import LOSS_W0
        blk = self.loss_block(device)
        return {"weight": blk[LOSS_W0:LOSS_W0 + self.num_class],
                "label_smoothing": self.label_smoothing, "block": blk}

    # ---- unfused path -----------------------------------------------------------------------
    def run_modules(self, x: Tensor) -> Tensor:
        for m in self.modules:
            x = m(x)
        return x


def _env_numbers(name: str) -> List[float]:
    try:
        return [float(v) for v in _os.environ[name].split(",")]
    except ValueError:
        raise ValueError(f"{name} must be a comma list of numbers, got {_os.environ[name]!r}")


def check_loss_options(class_weights, label_smoothing, num_class: int):
    """``(weights as a list of floats or None, eps)``; ValueError on anything else."""
    eps = 0.0 if label_smoothing is None else label_smoothing
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing {label_smoothing!r}: expected a number in [0, 1)")
    if class_weights is None:
        return None, float(eps)
    if isinstance(class_weights, Tensor):
        class_weights = class_weights.detach().cpu().tolist()
    if isinstance(class_weights, (str, bytes)) or not isinstance(class_weights, (list, tuple)):
        raise ValueError(f"class_weights {class_weights!r}: expected a list of {num_class} numbers")
    w = list(class_weights)
    if (len(w) != num_class or any(isinstance(v, bool) or not isinstance(v, (int, float))
                                   or not math.isfinite(v) or v <= 0 for v in w)):
        raise ValueError(f"class_weights {class_weights!r}: expected {num_class} finite numbers > 0")
    return [float(v) for v in w], float(eps)


class _HeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, spec: HeadSpec, log_out: bool, hint, *params):
        ctx.set_materialize_grads(False)  # no zero-filled grads for out / pred
        x = x.float()
        if x.stride(1) != 1:  # rows may be strided (a device-fed padded feature buffer)
            x = x.contiguous()
        y = y.long().contiguous()
        B = x.shape[0]
        C = spec.dims[-1]
        train = spec.training
        lay = spec.layout(B)
        ws = torch.empty(lay[0], dtype=torch.uint8, device=x.device)
        out = torch.empty(B, C, dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        pred = torch.empty(B, dtype=torch.long, device=x.device)
        rng = spec.rng(x.device)
        lossp = _lib.ptr(spec.loss_block(x.device))
        ctx.hint_ptr = None
        ctx.step_dx = None
        ctx.one_launch = False
        wbf = jt = None
        if train and hint is not None and _HEAD_STEP and _cap.active() is None:
            jt = spec.rep_jobs(B, x.device)
            if jt is not None:
                wbf = _bf16_images(spec) or spec.own_images(x.device)
        if wbf is not None:
            dx = (torch.empty(B, x.shape[1], dtype=torch.float32, device=x.device)
                  if ctx.needs_input_grad[0] else None)
            rc = _lib.lib().dn_head_rep_lw(
                spec.nl, spec._dims, spec._flags, spec._drops, spec._bnp, spec.ptrs(True), wbf,
                jt.data_ptr(), x.data_ptr(), x.stride(0), B, y.data_ptr(), out.data_ptr(), loss.data_ptr(),
                pred.data_ptr(), rng.data_ptr(), spec.sync(x.device).data_ptr(), int(log_out),
                hint.data_ptr(), _lib.ptr(dx), x.shape[1], lossp, _lib.stream())
            if rc == 0:
                global REP_LAUNCHES
                REP_LAUNCHES += 1
                ctx.one_launch = True
                ctx.hint_ptr = hint.data_ptr()
                ctx.step_dx = dx
                ctx.spec, ctx.B, ctx.D0, ctx.train = spec, B, x.shape[1], train
                ctx.ws = None
                ctx.mark_non_differentiable(out, pred)
                return out, loss, pred
            if rc != 3:
                raise RuntimeError(f"dn_head_rep failed with status {rc}")
        if train and hint is not None:
            rc = _lib.lib().dn_head_fwd_train_lw(
                spec.nl, spec._dims, spec._flags, spec._drops, spec._bnp, spec.ptrs(True),
                x.data_ptr(), x.stride(0), B, y.data_ptr(), out.data_ptr(), loss.data_ptr(),
                pred.data_ptr(), rng.data_ptr(), ws.data_ptr(), int(log_out), hint.data_ptr(),
                lossp, _lib.stream())
            if rc == 0:
                ctx.hint_ptr = hint.data_ptr()
            elif rc != 3:  # 3 = unsupported shape: the classic launches below
                raise RuntimeError(f"dn_head_fwd_train failed with status {rc}")
        if ctx.hint_ptr is None:
            _lib.call("dn_head_fwd_lw", spec.nl, spec._dims, spec._flags, spec._drops, spec._bnp,
                      spec.ptrs(False), x.data_ptr(), x.stride(0), B, y.data_ptr(),
                      out.data_ptr(), loss.data_ptr(), pred.data_ptr(), rng.data_ptr(),
                      ws.data_ptr(), int(train), int(log_out), lossp, _lib.stream())
        ctx.spec, ctx.B, ctx.D0, ctx.train = spec, B, x.shape[1], train
        ctx.ws = ws if train else None
        ctx.mark_non_differentiable(out, pred)
        return out, loss, pred

    @staticmethod
    def backward(ctx, dout, dloss, dpred):
        n_in = 5 + len(ctx.spec.params())
        if dloss is None:
            return (None,) * n_in
        if not ctx.train:
            raise RuntimeError("fused head: backward needs a training-mode forward")
        spec, B = ctx.spec, ctx.B
        if ctx.one_launch:
            # the forward launch already ran the whole backward for d loss == the hint tensor
            # and accumulated every head gradient; any other d loss cannot be honoured
            if dloss.data_ptr() != ctx.hint_ptr:
                raise RuntimeError("fused head step: backward must pass the loss_grad_hint tensor")
            _grad.notify(spec.params())
            dx, ctx.step_dx = ctx.step_dx, None
            return (dx,) + (None,) * (n_in - 1)
        dloss = dloss.float().contiguous()
        dx = torch.empty(B, ctx.D0, dtype=torch.float32, device=dloss.device) \
            if ctx.needs_input_grad[0] else None
        if ctx.hint_ptr is not None and dloss.data_ptr() == ctx.hint_ptr:
            # the forward already ran the output-gradient chain for exactly this d loss
            _lib.call("dn_head_bwd0", spec.nl, spec._dims, spec._flags, spec._drops, spec._bnp,
                      spec.ptrs(True), B, ctx.ws.data_ptr(), _lib.ptr(dx), ctx.D0,
                      _lib.stream())
        else:
            _lib.call("dn_head_bwd_lw", spec.nl, spec._dims, spec._flags, spec._drops, spec._bnp,
                      spec.ptrs(True), B, ctx.ws.data_ptr(), dloss.data_ptr(), _lib.ptr(dx),
                      ctx.D0, int(spec.loss_on), _lib.stream())
        params = spec.params()
        _grad.notify(params)
        if _cap.active() is not None:
            lay = spec.layout(B)
            for l, L in enumerate(spec.layers):
                a_off, s_a, dz_off, s_z = lay[1 + 4 * l: 5 + 4 * l]
                A = _ws_image(ctx.ws, a_off, B, s_a)[:, :L.linear.in_features]
                D = _ws_image(ctx.ws, dz_off, B, s_z)[:, :L.linear.out_features]
                _cap.record(L.linear, A.float(), D.float())
        ctx.ws = None
        return (dx,) + (None,) * (n_in - 1)


def _ws_image(ws: Tensor, off: int, rows: int, stride: int) -> Tensor:
    return ws[off: off + 2 * rows * stride].view(torch.bfloat16).view(rows, stride)


def head_loss(x: Tensor, spec: HeadSpec, y: Tensor, log_out: bool):
    """``(out, loss, pred)`` of ``loss(modules(x), y)``; fused on a GPU when supported."""
    if spec.supported(x):
        hint = _HINT
        if hint is not None and not (_FUSED_HEAD and torch.is_grad_enabled() and spec.training
                                     and hint.device == x.device and hint.numel() == 1
                                     and hint.dtype == torch.float32 and x.shape[0] <= 32):
            hint = None
        return _HeadFn.apply(x, y, spec, bool(log_out), hint, *spec.params())
    logits = spec.run_modules(x)
    from .heads import log_softmax_nll, softmax_ce  # (CPU logits: ops.reference)
    return (log_softmax_nll if log_out else softmax_ce)(
        logits, y, **spec.loss_kwargs(logits.device))
