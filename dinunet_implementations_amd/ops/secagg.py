"""Secure aggregation of the dSGD gradient: every party sends a pairwise-masked fixed-point image
of its gradient, the masks cancel in the mod-2^64 sum over the parties, and every party opens the
same exact sum -- nobody sees another party's gradient (``parallel.secagg`` agrees the keys).

On a GPU a release is the launches of ``csrc/kernels/secagg.hip``: ``mask_`` quantises (``q =
int64(rint(clamp(g, +-2^18) * 2^40))``) and adds ``sum_{j > rank} PRG(k_j) - sum_{j < rank}
PRG(k_j)`` with the ChaCha20 block function as the generator, at block index = element / 8,
release number ``t`` and the (fold, phase) domain word; ``open_`` turns the summed wire into the
fp32 mean and advances ``t``.  The wire has ``n + 8`` uint64 words: the extra block carries the
party's "had a non-finite element" flag and its clamped-element count, masked like the rest.
Release number, counts, keys and the opening factor live in one device block, so a captured HIP
graph replays releases with fresh masks and no host work.  On CPU tensors both halves are the
numpy mirror ``ops.reference.secagg_mask`` / ``secagg_open`` (no kernel library needed).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import _lib, reference

_lib.register("dn_secagg_mask", [_lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_void_p,
                                 _lib.c_void_p])
_lib.register("dn_secagg_open", [_lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_void_p,
                                 _lib.c_void_p])

# secagg.hip SaState: int32 W, rank, uint32 domain, pad; 8-byte words t, saturated, nonfinite,
# last_saturated, fp64 c; uint32 key[MAXW][8]; int32 part[PARTS][2] (size, party bound and
# partial count checked against the library on a GPU)
MAXW = reference.SA_MAX_PARTIES
PARTS = 1024
TAIL = reference.SA_TAIL
FRAC_BITS = reference.SA_FRAC_BITS
_W_W, _W_RANK, _W_DOMAIN = 0, 1, 2
_Q_T, _Q_SAT, _Q_NONFINITE, _Q_LAST, _Q_C = 2, 3, 4, 5, 6
_W_KEY = 14
BLOCK_BYTES = 4 * (_W_KEY + MAXW * 8 + PARTS * 2)


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class SecAggState:
    """The device block of one party's masked releases, and the two halves of a release.

    ``keys[j]`` is the 32-byte key this party shares with party ``j`` (``keys[rank]`` is not
    read).  The keys go into the block and nowhere else: this object keeps no host copy, and
    ``state_dict`` holds only the release number and the counts -- a resumed run agrees fresh
    keys (the opened mean does not depend on them).  ``mask_(grad, wire)`` fills ``wire`` (int64,
    ``grad.numel() + 8``) with release ``t + 1`` of ``grad`` (contiguous fp32, numel a multiple
    of 4); ``open_(total, grad)`` writes the mean of the ``world`` parties into ``grad`` from the
    mod-2^64 sum ``total`` of their wires (all NaN if any party had a non-finite element) and
    advances ``t``.  Writes to the block inside a HIP graph capture are refused."""

    MAX_PARTIES = MAXW

    def __init__(self, device, world: int, rank: int, keys: Sequence[Optional[bytes]],
                 domain: int = 0):
        self.device = torch.device(device)
        world, rank, domain = int(world), int(rank), int(domain)
        if not (2 <= world <= MAXW):
            raise ValueError(f"secure aggregation: 2 to {MAXW} parties (sums of more do not fit "
                             f"int64), got {world}")
        if not (0 <= rank < world):
            raise ValueError(f"secure aggregation: rank {rank} of {world} parties")
        if not (0 <= domain < 2 ** 32):
            raise ValueError(f"secure aggregation: domain word {domain!r} is not in [0, 2^32)")
        if len(keys) != world or any(j != rank and (not isinstance(k, (bytes, bytearray))
                                                    or len(k) != 32)
                                     for j, k in enumerate(keys)):
            raise ValueError("secure aggregation: one 32-byte key per peer is required")
        if self.device.type == "cuda":
            _lib.checked_struct(BLOCK_BYTES, "dn_secagg_state_size", "secure aggregation state",
                                dn_secagg_parts=PARTS, dn_secagg_maxw=MAXW)
        self.world, self.rank, self.domain = world, rank, domain
        self._block = torch.zeros(BLOCK_BYTES // 8, dtype=torch.int64, device=self.device)
        self._i = self._block.view(torch.int32)
        self._d = self._block.view(torch.float64)
        self._write_host_words(keys)

    def _write_host_words(self, keys):
        self._refuse_in_capture("keys")
        host = torch.zeros(_W_KEY + MAXW * 8, dtype=torch.int32)
        host[_W_W], host[_W_RANK] = self.world, self.rank
        host[_W_DOMAIN] = self.domain - (1 << 32) if self.domain >= 1 << 31 else self.domain
        for j, k in enumerate(keys):
            if j != self.rank:
                host[_W_KEY + 8 * j:_W_KEY + 8 * j + 8] = torch.frombuffer(bytearray(k),
                                                                          dtype=torch.int32)
        counters = self._block[_Q_T:_Q_C].clone()  # kernel-written words stay
        self._i[:host.numel()].copy_(host)
        self._block[_Q_T:_Q_C].copy_(counters)
        self._d[_Q_C] = 2.0 ** -FRAC_BITS / self.world  # the opening factor, once, in double
        host.zero_()

    def _refuse_in_capture(self, what: str):
        if self.device.type == "cuda" and _capturing():
            # the write would become a graph node that resets the value at every replay
            raise RuntimeError(f"SecAggState.{what} written inside a HIP graph capture")

    def rekey(self, keys: Sequence[Optional[bytes]]):
        """Fresh pair keys (a new agreement); the release number and the counts stay."""
        if len(keys) != self.world:
            raise ValueError("secure aggregation: one 32-byte key per peer is required")
        self._write_host_words(keys)

    # kernel-written words (one host read each) ---------------------------------------------------
    @property
    def releases(self) -> int:
        return int(self._block[_Q_T].item())

    @property
    def saturated(self) -> int:
        """Elements clamped to +-2^18, summed over the parties and the releases."""
        return int(self._block[_Q_SAT].item())

    @property
    def last_saturated(self) -> int:
        return int(self._block[_Q_LAST].item())

    @property
    def nonfinite(self) -> int:
        """Releases in which some party had a non-finite element (all NaN on every party)."""
        return int(self._block[_Q_NONFINITE].item())

    # the release ---------------------------------------------------------------------------------
    def wire_like(self, grad: torch.Tensor) -> torch.Tensor:
        return torch.zeros(grad.numel() + TAIL, dtype=torch.int64, device=grad.device)

    def _check(self, grad: torch.Tensor, wire: torch.Tensor, what: str):
        if (grad.dtype != torch.float32 or not grad.is_contiguous() or grad.numel() % 4
                or grad.numel() == 0 or grad.device.type != self.device.type
                or wire.dtype != torch.int64 or not wire.is_contiguous()
                or wire.numel() != grad.numel() + TAIL or wire.device != grad.device):
            raise ValueError(f"SecAggState.{what}: a contiguous fp32 gradient on the state's device "
                             "with a multiple of 4 elements and an int64 wire of 8 words more "
                             "are required")

    def _keys(self):
        k = self._i[_W_KEY:_W_KEY + MAXW * 8].cpu().numpy().view("uint32").reshape(MAXW, 8)
        return [k[j] for j in range(self.world)]

    def mask_(self, grad: torch.Tensor, wire: torch.Tensor) -> torch.Tensor:
        self._check(grad, wire, "mask_")
        if grad.is_cuda:
            _lib.call("dn_secagg_mask", grad.data_ptr(), grad.numel(), wire.data_ptr(),
                      self._block.data_ptr(), _lib.stream())
            return wire
        w = reference.secagg_mask(grad, self._keys(), self.rank, self.releases + 1, self.domain)
        wire.copy_(torch.from_numpy(w.view("int64")))
        return wire

    def open_(self, total: torch.Tensor, grad: torch.Tensor) -> torch.Tensor:
        self._check(grad, total, "open_")
        if grad.is_cuda:
            _lib.call("dn_secagg_open", total.data_ptr(), grad.numel(), grad.data_ptr(),
                      self._block.data_ptr(), _lib.stream())
            return grad
        mean, sat, bad = reference.secagg_open(total.numpy().view("uint64"), self.world)
        grad.copy_(mean)
        self._block[_Q_T] += 1
        self._block[_Q_LAST] = sat
        self._block[_Q_SAT] += sat
        self._block[_Q_NONFINITE] += bad
        return grad

    # resume --------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, int]:
        return {"t": self.releases, "saturated": self.saturated, "nonfinite": self.nonfinite,
                "last_saturated": self.last_saturated}

    def load_state_dict(self, sd: Dict[str, int]):
        """Continue a saved release count (the keys are this run's own)."""
        self._refuse_in_capture("load_state_dict")
        self._block[_Q_T] = int(sd.get("t", 0))
        self._block[_Q_SAT] = int(sd.get("saturated", 0))
        self._block[_Q_NONFINITE] = int(sd.get("nonfinite", 0))
        self._block[_Q_LAST] = int(sd.get("last_saturated", 0))
