"""Top-k sparsified gradient release with error feedback: of ``acc = grad + err`` the ``k`` entries
of largest magnitude leave the site as ``(index, value)`` pairs, the rest stay in ``err`` for the
next step; the gathered pairs of all ranks are summed back into a dense gradient.

The contract (``ops.reference.topk_select`` / ``topk_combine`` are its numpy mirror, same bits):
``key(i) = bits(acc[i]) & 0x7fffffff`` (NaN > inf > finite, +-0 tie); the ``k`` largest keys are
selected, the lower index winning among equal keys; the pairs come in ascending index order;
``err[i] = +0`` where selected, ``acc[i]`` elsewhere; ``out[i] = ((+0 + v_0) + v_1) + ...`` over
the ranks that selected ``i``, in rank order.

On a GPU a release is the launches of ``csrc/kernels/topk.hip`` (an exact radix select, an
ordered compaction, a per-range sum: integer logic, no float atomics, no host synchronisation, so
a captured HIP graph replays it on fresh gradients); on CPU tensors the same contract in torch.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib

_lib.register("dn_topk_select", [_lib.c_void_p, _lib.c_void_p, _lib.c_long, _lib.c_int,
                                 _lib.c_void_p, _lib.c_int, _lib.c_void_p, _lib.c_void_p])
_lib.register("dn_topk_combine", [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_int, _lib.c_int,
                                  _lib.c_void_p, _lib.c_long, _lib.c_void_p])

# topk.hip scratch: hist[4][256], sel[4][2], cnt[1024][2] int32 words (checked against the
# library on a GPU)
SCRATCH_WORDS = 4 * 256 + 8 + 2 * 1024
FLOAT_INDEX_MAX = 1 << 24  # indices up to here are exact as fp32 values


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class TopKState:
    """The buffers of one rank's releases of an ``n``-element gradient at ``k`` pairs per step.

    ``send`` holds a release as ``2k`` 32-bit words, ``k`` indices then ``k`` values: what a rank
    puts on the wire.  With ``idx_float`` the index words are fp32 VALUES (``float(i)``, exact for
    ``n <= 2^24``) so that an fp32 exchange may carry them; else int32.  ``select(grad)`` fills
    ``send`` and updates ``err``; ``combine(W, out)`` sums the ``W`` send blocks of ``gathered``
    (``send`` itself at ``W = 1`` when nothing was gathered) into all ``n`` elements of ``out``."""

    def __init__(self, device, n: int, k: int, idx_float: bool = False):
        self.device = torch.device(device)
        n, k = int(n), int(k)
        if not (0 < n < 2 ** 31):
            raise ValueError(f"top-k: the gradient must hold 1 to 2^31 - 1 elements (int32 "
                             f"indices), got {n}")
        if not (1 <= k <= n):
            raise ValueError(f"top-k: k must lie in [1, n = {n}], got {k}")
        if idx_float and n > FLOAT_INDEX_MAX:
            raise ValueError(f"top-k: fp32 index words are exact up to n = 2^24, got {n}")
        self.n, self.k, self.idx_float = n, k, bool(idx_float)
        dev = self.device
        if dev.type == "cuda":
            got = int(_lib.lib().dn_topk_scratch_words())
            if got != SCRATCH_WORDS:
                raise RuntimeError("top-k scratch layout mismatch with the kernel library")
        self.err = torch.zeros(n, dtype=torch.float32, device=dev)
        self.send = torch.zeros(2 * k, dtype=torch.float32, device=dev)
        self.scratch = torch.zeros(SCRATCH_WORDS, dtype=torch.int32, device=dev)
        self.gathered: Optional[torch.Tensor] = None  # [W * 2k] words, rank-major

    # the last release --------------------------------------------------------------------------
    @property
    def idx(self) -> torch.Tensor:
        """The selected indices, ascending (int32 ``[k]``)."""
        w = self.send[:self.k]
        return w.to(torch.int32) if self.idx_float else w.view(torch.int32)

    @property
    def val(self) -> torch.Tensor:
        """``acc`` at the selected indices (fp32 ``[k]``)."""
        return self.send[self.k:]

    def gather_buffer(self, W: int) -> torch.Tensor:
        if self.gathered is None or self.gathered.numel() != int(W) * 2 * self.k:
            if self.device.type == "cuda" and _capturing():
                raise RuntimeError("TopKState: the gather buffer is built outside a capture")
            self.gathered = torch.zeros(int(W) * 2 * self.k, dtype=torch.float32,
                                        device=self.device)
        return self.gathered

    def _check(self, t: torch.Tensor, what: str):
        if (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.n
                or t.device.type != self.device.type):
            raise ValueError(f"TopKState.{what}: {self.n} contiguous fp32 elements on the state's "
                             "device are required")

    def select(self, grad: torch.Tensor) -> None:
        """One release of ``grad``: ``send`` <- the ``k`` pairs, ``err`` <- the residual."""
        self._check(grad, "select")
        if grad.is_cuda:
            _lib.call("dn_topk_select", grad.data_ptr(), self.err.data_ptr(), self.n, self.k,
                      self.send.data_ptr(), int(self.idx_float), self.scratch.data_ptr(),
                      _lib.stream())
            return
        acc = grad + self.err
        key = acc.view(torch.int32) & 0x7FFFFFFF
        # a stable descending sort keeps equal keys in index order: the lower index wins
        order = torch.sort(key, descending=True, stable=True).indices[:self.k]
        idx = torch.sort(order).values
        self.send[self.k:] = acc[idx]
        if self.idx_float:
            self.send[:self.k] = idx.to(torch.float32)
        else:
            self.send[:self.k].view(torch.int32).copy_(idx.to(torch.int32))
        acc[idx] = 0.0
        self.err.copy_(acc)

    def combine(self, W: int, out: torch.Tensor,
                pairs: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``out`` (all ``n`` elements) <- the sum of the ``W`` send blocks of ``pairs`` (default:
        ``gathered``, or ``send`` at ``W = 1`` when nothing was gathered), in rank order."""
        self._check(out, "combine")
        W = int(W)
        if pairs is None:
            pairs = self.send if (W == 1 and self.gathered is None) else self.gathered
        fl, k = self.idx_float, self.k
        if (pairs is None or pairs.dtype != torch.float32 or not pairs.is_contiguous()
                or pairs.numel() < W * 2 * k or W < 1 or pairs.device != out.device):
            raise ValueError(f"TopKState.combine: {W} blocks of {2 * k} contiguous 32-bit words "
                             "are required")
        if out.is_cuda:
            _lib.call("dn_topk_combine", pairs.data_ptr(), W, 2 * k, k, int(fl), out.data_ptr(),
                      self.n, _lib.stream())
            return out
        out.zero_()
        blocks = pairs[:W * 2 * k].view(W, 2 * k)
        for w in range(W):
            iw = blocks[w, :k]
            idx = iw.to(torch.int64) if fl else iw.view(torch.int32).to(torch.int64)
            out[idx] = out[idx] + blocks[w, k:]
        return out

    # resume --------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"err": self.err.detach().cpu().clone()}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        if self.device.type == "cuda" and _capturing():
            raise RuntimeError("TopKState.load_state_dict inside a HIP graph capture")
        e = sd.get("err")
        if e is not None:
            if e.numel() != self.n:
                raise ValueError(f"top-k: a residual of {self.n} elements is required, got "
                                 f"{e.numel()}")
            self.err.copy_(e.to(self.device, torch.float32).reshape(-1))
