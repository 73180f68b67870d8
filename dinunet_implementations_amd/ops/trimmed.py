"""Coordinate-wise trimmed mean / median over the sites' gradients: of the ``W`` values a
coordinate has, one per site, the ``b`` smallest and the ``b`` largest are dropped and the rest
averaged; per site a cumulative count of the coordinates at which it was dropped.

The contract (``ops.reference.trimmed_mean`` is its numpy mirror, same bits): ``key(x) = bits(x) ^
0x80000000`` when the sign bit is clear, else ``~bits(x)`` (unsigned order = the IEEE total order,
-NaN first, +NaN last); a coordinate's entries are sorted ascending by ``(key, site)``; ``s =
v[b]; s = s + v[b+1]; ...; s = s + v[W-1-b]`` in fp32; ``out = s`` when ``W - 2b`` is 1, else ``s *
inv`` with ``inv = float32(1) / float32(W - 2b)`` made on the host; ``trimmed[w]`` grows by the
coordinates at which site ``w`` sat at a sorted position ``< b`` or ``>= W - b``.

On a GPU one combine is one launch of ``csrc/kernels/trimmed.hip`` (a register sorting network,
integer atomics for the counts, no host synchronisation, so a captured HIP graph replays it on
fresh rows); on CPU tensors the same contract in torch.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _lib

_lib.register("dn_trimmed_mean", [_lib.c_void_p, _lib.c_int, _lib.c_long, _lib.c_long, _lib.c_int,
                                  _lib.c_float, _lib.c_void_p, _lib.c_void_p, _lib.c_void_p])
_lib.register("dn_trimmed_set_max_blocks", [_lib.c_int])

MAX_SITES = 16  # the peer exchange's limit; the kernel is instantiated for 1 .. 16 sites


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def set_max_blocks(blocks: int) -> None:
    """Bound the combine launch's workgroups (0: the default, 4 per CU), so that its grid-stride
    loop wraps at a small ``n`` (tests)."""
    _lib.lib().dn_trimmed_set_max_blocks(int(blocks))


class TrimmedState:
    """The buffers of one rank's trimmed means of ``W`` sites' ``n``-element gradients with ``b``
    sites dropped at each end.

    ``gather_buffer()`` is ``[W, stride]`` fp32, ``stride`` = ``n`` rounded up to 4 (the kernel
    loads 16 bytes per row): row ``w`` receives site ``w``'s gradient.  ``combine(rows, out)``
    writes all ``n`` elements of ``out`` and advances the per-site counters; ``counts()`` reads
    them."""

    def __init__(self, device, n: int, W: int, b: int):
        self.device = torch.device(device)
        n, W, b = int(n), int(W), int(b)
        if not (0 < n < 2 ** 31):
            raise ValueError(f"trimmed mean: the gradient must hold 1 to 2^31 - 1 elements, got {n}")
        if not (1 <= W <= MAX_SITES):
            raise ValueError(f"trimmed mean: 1 to {MAX_SITES} sites, got {W}")
        if not (0 <= 2 * b < W):
            raise ValueError(f"trimmed mean: dropping b = {b} sites at each end leaves none of "
                             f"W = {W} (0 <= 2b < W is required)")
        self.n, self.W, self.b = n, W, b
        self.stride = -(-n // 4) * 4
        from .reference import trimmed_inv
        self.inv = float(trimmed_inv(W, b))
        if self.device.type == "cuda":
            got = int(_lib.lib().dn_trimmed_max_sites())
            if got != MAX_SITES:
                raise RuntimeError("trimmed mean: site limit mismatch with the kernel library")
        # 64-bit counters on the device (int64 words: the kernel adds to them as uint64)
        self.trimmed = torch.zeros(W, dtype=torch.int64, device=self.device)
        self.gathered: Optional[torch.Tensor] = None

    def gather_buffer(self) -> torch.Tensor:
        if self.gathered is None:
            if self.device.type == "cuda" and _capturing():
                raise RuntimeError("TrimmedState: the gather buffer is built outside a capture")
            self.gathered = torch.zeros(self.W, self.stride, dtype=torch.float32,
                                        device=self.device)
        return self.gathered

    def combine(self, rows: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """``out`` (all ``n`` elements) <- the trimmed mean of ``rows`` (``[W, stride >= n]``,
        row stride a multiple of 4); the counters advance."""
        W, n = self.W, self.n
        if (out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n
                or out.device.type != self.device.type):
            raise ValueError(f"TrimmedState.combine: {n} contiguous fp32 output elements on the "
                             "state's device are required")
        if (rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[0] != W
                or rows.shape[1] < n or rows.device != out.device
                or (rows.stride(1) != 1 and rows.shape[1] > 1)):
            raise ValueError(f"TrimmedState.combine: rows must be fp32 [{W}, >= {n}] with unit "
                             "element stride on the output's device")
        rs = int(rows.stride(0)) if W > 1 else -(-int(rows.shape[1]) // 4) * 4
        if rs % 4 or rs < n:
            raise ValueError(f"TrimmedState.combine: the row stride must be a multiple of 4 and "
                             f">= n = {n} (16-byte loads), got {rs}")
        if out.is_cuda:
            _lib.call("dn_trimmed_mean", rows.data_ptr(), W, rs, n, self.b, self.inv,
                      out.data_ptr(), self.trimmed.data_ptr(), _lib.stream())
            return out
        b = self.b
        x = rows[:, :n]
        u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        key = torch.where(u >= 0x80000000, u ^ 0xFFFFFFFF, u ^ 0x80000000)
        site = torch.arange(W, dtype=torch.int64).unsqueeze(1)
        word = torch.sort((key << 4) | site, dim=0).values  # < 2^36: exact in int64
        k = word >> 4
        ssite = word & 15
        bits = torch.where(k >= 0x80000000, k ^ 0x80000000, k ^ 0xFFFFFFFF)
        bits = torch.where(bits >= 0x80000000, bits - (1 << 32), bits).to(torch.int32)
        vals = bits.view(torch.float32)
        s = vals[b].clone()
        for p in range(b + 1, W - b):
            s = s + vals[p]
        out.copy_(s if W - 2 * b == 1 else s * torch.tensor(self.inv, dtype=torch.float32))
        ends = torch.cat([ssite[:b], ssite[W - b:]], 0).reshape(-1)
        self.trimmed += torch.bincount(ends, minlength=W)
        return out

    def counts(self) -> torch.Tensor:
        """The cumulative per-site trimmed-coordinate counts (int64 CPU tensor ``[W]``)."""
        return self.trimmed.detach().cpu().clone()

    # resume --------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"trimmed": self.counts()}

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        if self.device.type == "cuda" and _capturing():
            raise RuntimeError("TrimmedState.load_state_dict inside a HIP graph capture")
        t = sd.get("trimmed")
        if t is not None:
            if t.numel() != self.W:
                raise ValueError(f"trimmed mean: counters of {self.W} sites are required, got "
                                 f"{t.numel()}")
            self.trimmed.copy_(t.to(self.device, torch.int64).reshape(-1))
