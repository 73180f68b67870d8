"""Device state and batch-boundary launch of a device-fed evaluation pass (``eval.hip``).

:class:`EvalPass` owns what a pass over a resident split writes and reads on the device: the
static input a forward reads (``xb`` / ``yd``, ``cap`` rows), the pass-level results (``out_all
[N, C]``, ``pred_all [N]``, ``loss_b [nb]``, one allocation so the host reads them in one copy),
the cursor and the boundary kernel's ticket.  ``runtime.evalfeed.EvalFeed`` captures
``boundary`` launches between the forwards of a pass.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import torch

from . import _lib
from .optim import DeviceSource, ctypes_addr

_lib.register("dn_eval_boundary", [_lib.c_void_p, _lib.c_void_p])

_BOUNDARY = None


def _boundary_type():
    """The ctypes layout of ``eval.hip EvalBoundary``, checked against the library once."""
    global _BOUNDARY
    if _BOUNDARY is None:
        P, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int

        class _Eb(ctypes.Structure):
            _fields_ = [("out", P), ("pred", P), ("loss", P), ("out_all", P), ("pred_all", P),
                        ("loss_b", P), ("cursor", P), ("ticket", P), ("gx", P), ("gy", P),
                        ("xb", P), ("yd", P), ("N", L), ("nb", L), ("ld", L), ("C", I),
                        ("n_prev", I), ("cap", I), ("f8", I), ("mode", I)]
        _BOUNDARY = _lib.checked_struct(_Eb, "dn_eval_boundary_size", "evaluation boundary")
    return _BOUNDARY


class EvalPass:
    """``src``: the resident split (``DeviceSource``: bf16, or fp32 rows padded to 8 features);
    ``cap``: rows of the largest batch of the pass; ``nb``: its batches; ``C``: output columns."""

    def __init__(self, src: DeviceSource, cap: int, nb: int, C: int):
        X = src.X
        self.src = src
        self.N = int(X.shape[0])
        self.cap, self.nb, self.C = int(cap), int(nb), int(C)
        if not (0 < self.cap <= self.N and self.nb > 0 and self.C > 0):
            raise ValueError("EvalPass: empty pass")
        dev = X.device
        self.xb = torch.zeros((self.cap,) + src.sample_shape, dtype=X.dtype, device=dev)
        self.yd = torch.zeros(self.cap, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(2, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        # [out_all | loss_b | pad] as fp32 words of an int64 buffer, then pred_all
        self._nf64 = (self.N * self.C + self.nb + 1) // 2
        self.buf = torch.zeros(self._nf64 + self.N, dtype=torch.int64, device=dev)
        self.out_all, self.loss_b, self.pred_all = self.views(self.buf)

    def views(self, buf: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(out_all, loss_b, pred_all)`` of ``buf`` (the device buffer, or its host copy)."""
        fl = buf[:self._nf64].view(torch.float32)
        n = self.N * self.C
        return fl[:n].view(self.N, self.C), fl[n:n + self.nb], buf[self._nf64:]

    def reset(self):
        """Start of a pass: the cursor back at row 0 / batch 0."""
        self.cursor.zero_()

    def boundary(self, out: Optional[torch.Tensor] = None, loss: Optional[torch.Tensor] = None,
                 pred: Optional[torch.Tensor] = None, n_prev: int = 0):
        """ONE launch: file the finished batch (``out [n_prev, C]``, ``loss`` scalar, ``pred
        [n_prev]`` int64; none at the start of a pass), advance the cursor, gather the next batch
        into ``xb`` / ``yd``."""
        n_prev = int(n_prev)
        if n_prev:
            if (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != n_prev
                    or out.shape[1] != self.C or out.stride(1) != 1
                    or loss.dtype != torch.float32 or loss.numel() != 1
                    or pred.dtype != torch.int64 or pred.numel() != n_prev
                    or not pred.is_contiguous()):
                raise ValueError("EvalPass.boundary: out fp32 [n, C], loss fp32 scalar and pred "
                                 "int64 [n] required")
        src = self.src
        eb = _boundary_type()(
            out.data_ptr() if n_prev else None, pred.data_ptr() if n_prev else None,
            loss.data_ptr() if n_prev else None, self.out_all.data_ptr(),
            self.pred_all.data_ptr(), self.loss_b.data_ptr(), self.cursor.data_ptr(),
            self.ticket.data_ptr(), src.X.data_ptr(), src.Y.data_ptr(), self.xb.data_ptr(),
            self.yd.data_ptr(), self.N, self.nb, out.stride(0) if n_prev else self.C, self.C,
            n_prev, self.cap, src.row // 8, 1 if src.X.dtype == torch.bfloat16 else 2)
        _lib.call("dn_eval_boundary", ctypes_addr(eb), _lib.stream())
