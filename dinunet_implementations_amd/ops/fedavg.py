"""Federated averaging with local steps: the device side of one round.

Between rounds every site updates its own copy of the model.  A round turns the sites' copies
back into one, around ONE site mean (``parallel.engines.FedAvgEngine`` runs it).  With ``p`` the
parameters, ``a`` the anchor (the model every site held after the last round), ``w`` this site's
weight, ``eta`` the server learning rate and ``beta`` the server momentum, per element and every
fp32 operation rounded on its own (no fused multiply-add anywhere):

1. ``delta``:  ``d = (p - a) * w`` is written into the flat gradient buffer (all zero between
   updates: every Adam form zeroes what it consumes), and ``drift = sqrt(sum (p - a)^2)``
   (unweighted, summed in fp64 in a fixed order) describes how far the site moved;
2. the site mean ``m`` of ``d`` (not here);
3. ``adopt``:  with momentum ``u = beta * u + m; s = u``, else ``s = m``; then ``a = a + eta * s``,
   ``p = a`` and the gradient buffer is zero again.

Adam's moments, BatchNorm buffers and the device step counter are not touched: they stay local
to a site.  On a GPU each of 1 and 3 is one launch of ``csrc/kernels/fedavg.hip`` on the current
stream (16-byte accesses, a scalar tail, no host synchronisation); CPU tensors take the same
operations in the same order in torch.  ``tests/fedavg_ref.py`` is the numpy mirror (same bits).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib

_lib.register("dn_fedavg_delta", [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_long,
                                  _lib.c_float, _lib.c_void_p, _lib.c_void_p])
_lib.register("dn_fedavg_adopt", [_lib.c_void_p, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p,
                                  _lib.c_long, _lib.c_float, _lib.c_float, _lib.c_void_p,
                                  _lib.c_void_p])

PARTS = 2048  # drift partials of the delta launch (its grid cap), then the drift itself

WEIGHTINGS = ("uniform", "samples")


def site_weights(sizes: Sequence[int]) -> List[float]:
    """``fedavg_weighting="samples"``: ``w_s = fp32(W * n_s / sum n)`` evaluated in double, for
    every site from the same train-split sizes -- the plain mean of ``w_s d_s`` is then
    ``sum n_s d_s / sum n``."""
    sizes = [int(v) for v in sizes]
    W, tot = len(sizes), sum(sizes)
    if W < 1 or min(sizes) < 0 or tot <= 0:
        raise ValueError(f"fedavg_weighting='samples': the sites' train splits hold {sizes} "
                         f"samples (at least one sample overall is required)")
    return [float(np.float32(float(W * n) / float(tot))) for n in sizes]


def _f32(v: float) -> torch.Tensor:
    return torch.tensor(float(v), dtype=torch.float32)


class FedAvgState:
    """The anchor, the server momentum and the drift of one site's rounds over ``flat`` (anything
    with contiguous fp32 ``data`` and ``grad`` of one length, ``ops.FlatParams``).  ``momentum``
    > 0 allocates ``u`` (zero); else the adopt rule reads and writes none."""

    def __init__(self, flat, momentum: float = 0.0):
        p, g = flat.data, flat.grad
        if (p.dtype != torch.float32 or g.dtype != torch.float32 or p.dim() != 1
                or p.shape != g.shape or p.device != g.device or p.numel() < 1
                or not p.is_contiguous() or not g.is_contiguous()):
            raise ValueError("FedAvgState: flat.data and flat.grad must be contiguous fp32 "
                             "vectors of one length (>= 1) on one device")
        momentum = float(momentum)
        if not (0.0 <= momentum < 1.0):
            raise ValueError(f"FedAvgState: momentum must lie in [0, 1), got {momentum!r}")
        self.flat = flat
        self.n = int(p.numel())
        self.momentum = momentum
        self.anchor = torch.zeros_like(p)
        self.u: Optional[torch.Tensor] = torch.zeros_like(p) if momentum > 0 else None
        self._work = torch.zeros(PARTS + 1, dtype=torch.float64, device=p.device)
        if p.is_cuda:
            _lib.checked_struct(8 * (PARTS + 1), "dn_fedavg_work_size", "FedAvgState work block",
                                dn_fedavg_parts=PARTS)

    @property
    def drift(self) -> torch.Tensor:
        """``||p - a||_2`` of the last round's delta (fp64 device scalar, set by ``adopt``)."""
        return self._work[PARTS]

    def begin(self):
        """The anchor becomes the current parameters (every site holds the same ones)."""
        self.anchor.copy_(self.flat.data)

    def delta(self, w: float = 1.0) -> torch.Tensor:
        """``flat.grad = (p - a) * w``; the drift partials are left for :meth:`adopt`."""
        p, a, g = self.flat.data, self.anchor, self.flat.grad
        if p.is_cuda:
            _lib.call("dn_fedavg_delta", p.data_ptr(), a.data_ptr(), g.data_ptr(), self.n,
                      float(w), self._work.data_ptr(), _lib.stream())
            return g
        t = torch.sub(p, a)
        self._work[0] = t.double().pow(2).sum()
        torch.mul(t, _f32(w), out=g)
        return g

    def adopt(self, eta: float = 1.0, beta: Optional[float] = None) -> torch.Tensor:
        """The adopt rule on the site mean held in ``flat.grad``; ``beta`` defaults to the
        state's momentum."""
        p, a, g, u = self.flat.data, self.anchor, self.flat.grad, self.u
        beta = self.momentum if beta is None else float(beta)
        if p.is_cuda:
            _lib.call("dn_fedavg_adopt", p.data_ptr(), a.data_ptr(), g.data_ptr(),
                      None if u is None else u.data_ptr(), self.n, float(eta), beta,
                      self._work.data_ptr(), _lib.stream())
            return p
        self._work[PARTS] = self._work[0].sqrt()
        if u is not None:
            u.mul_(_f32(beta)).add_(g)
            s = u
        else:
            s = g
        a.add_(torch.mul(s, _f32(eta)))
        p.copy_(a)
        g.zero_()
        return p

    # resume --------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {} if self.u is None else {"u": self.u.detach().cpu().clone()}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        t = sd.get("u")
        if t is None or self.u is None:
            return
        if t.numel() != self.n:
            raise ValueError(f"fedAvg: a momentum buffer of {self.n} elements is required, got "
                             f"{t.numel()}")
        self.u.copy_(t.to(self.u.device, torch.float32).reshape(-1))
