"""Standalone loss heads (used when the classifier itself is not fused, see ``ops.head``).

``softmax_ce``  : ICA head, reference ``comps/icalstm/__init__.py:59-63``
``log_softmax_nll``: FS head, reference ``comps/fs/__init__.py:54-57``
Both return ``(out, loss, pred)`` where ``out`` is the probability (ICA) or log-probability (FS)
tensor, exactly what the reference trainers hand to their metrics.

``weight`` (one positive number per class) and ``label_smoothing`` are those of
``torch.nn.functional.cross_entropy`` with mean reduction: the batch's loss is divided by
``sum_i weight[y_i]`` of that batch.  The FS head applies the same formula to its logits
(``nll_loss(log_softmax(z)) == cross_entropy(z)``; torch's ``nll_loss`` has no smoothing argument).
On a GPU both run the fused ``dn_softmax_xent`` kernel, which reads the options from a small fp32
device block (:func:`loss_block`).
"""
from __future__ import annotations

import torch

from . import _lib
from . import reference as ref

_lib.register("dn_softmax_xent", [_lib.c_void_p, _lib.c_void_p, _lib.c_int, _lib.c_int,
                                  _lib.c_int, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p,
                                  _lib.c_void_p, _lib.c_void_p])
_lib.register("dn_softmax_xent_lw", [_lib.c_void_p, _lib.c_void_p, _lib.c_int, _lib.c_int,
                                     _lib.c_int, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p,
                                     _lib.c_void_p, _lib.c_void_p, _lib.c_void_p])

LOSS_W0 = 4  # first class weight in the block (csrc/kernels/loss_opt.h)


def loss_block_values(weight, label_smoothing: float, num_class: int) -> torch.Tensor:
    """The kernels' loss-option block as a CPU fp32 tensor (``csrc/kernels/loss_opt.h``):
    ``[1 - eps, eps / C, (eps / C) * sum(w), eps, w_0 .. w_{C-1}]``, padded to 16 weight slots."""
    C = int(num_class)
    eps = float(label_smoothing or 0.0)
    w = (torch.ones(C, dtype=torch.float32) if weight is None
         else torch.as_tensor(weight, dtype=torch.float32).detach().cpu().reshape(-1))
    if w.numel() != C:
        raise ValueError(f"class weights: {w.numel()} values for {C} classes")
    blk = torch.zeros(LOSS_W0 + max(C, 16), dtype=torch.float32)
    e = torch.tensor(eps / C, dtype=torch.float32)
    blk[0] = 1.0 - eps
    blk[1] = e
    blk[2] = e * w.sum()
    blk[3] = eps
    blk[LOSS_W0:LOSS_W0 + C] = w
    return blk


class _SoftmaxXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, y, log_out: bool, block=None):
        z = z.float().contiguous()
        y = y.long().contiguous()
        B, C = z.shape
        out = torch.empty_like(z)
        dz = torch.empty_like(z)
        loss = torch.empty((), dtype=torch.float32, device=z.device)
        pred = torch.empty(B, dtype=torch.long, device=z.device)
        _lib.call("dn_softmax_xent_lw", z.data_ptr(), y.data_ptr(), B, C, int(log_out),
                  out.data_ptr(), dz.data_ptr(), loss.data_ptr(), pred.data_ptr(),
                  _lib.ptr(block), _lib.stream())
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(out, pred)
        return out, loss, pred

    @staticmethod
    def backward(ctx, dout, dloss, dpred):
        (dz,) = ctx.saved_tensors
        if dloss is None:
            return None, None, None, None
        return dz * dloss, None, None, None


def _block(logits, weight, label_smoothing, block):
    """The device block of one call: the caller's (``ops.head.HeadSpec`` owns one, so captured
    graphs see later changes), else built from the arguments; None with the options off."""
    if block is not None:
        return block
    if weight is None and not label_smoothing:
        return None
    if not 0.0 <= float(label_smoothing) < 1.0:
        raise ValueError(f"label_smoothing {label_smoothing!r}: expected a number in [0, 1)")
    return loss_block_values(weight, label_smoothing, logits.shape[1]).to(logits.device)


def softmax_ce(logits: torch.Tensor, labels: torch.Tensor, weight=None,
               label_smoothing: float = 0.0, block=None):
    if logits.is_cuda:
        return _SoftmaxXent.apply(logits, labels, False,
                                  _block(logits, weight, label_smoothing, block))
    return ref.softmax_ce(logits, labels, weight, label_smoothing)


def log_softmax_nll(logits: torch.Tensor, labels: torch.Tensor, weight=None,
                    label_smoothing: float = 0.0, block=None):
    if logits.is_cuda:
        return _SoftmaxXent.apply(logits, labels, True,
                                  _block(logits, weight, label_smoothing, block))
    return ref.log_softmax_nll(logits, labels, weight, label_smoothing)
