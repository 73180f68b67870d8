"""Differentially private gradient release: clip the site's flat gradient to an L2 norm ``c`` and
add Gaussian noise of standard deviation ``sigma * c`` before any byte of it leaves the site.

On a GPU a release is the two launches of ``csrc/kernels/dp.hip``: the fp64 squared-norm partials
(as the clipped Adam forms them) with the release counter advanced on the device, then the clip
and the noise from a counter-based generator (Philox4x32-10) keyed by the seed, at counter
``(float4 index, release number, stream word)``.  Threshold, multiplier, key, stream and counter
live in one device block, so a captured HIP graph replays the release with no host work, never
repeats a draw, and follows a host write to the threshold or the multiplier without recapture.
On CPU tensors the release is the fp64 mirror ``ops.reference.dp_privatize`` (no kernel library
needed).  ``parallel.privacy`` turns the release count into (epsilon, delta).
"""
from __future__ import annotations

import math
import struct
from typing import Dict

import torch

from . import _lib, reference
from .optim import _f32

_lib.register("dn_dp_privatize", [_lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_void_p])
_lib.register("dn_dp_norm", [_lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_void_p])
_lib.register("dn_dp_apply", [_lib.c_void_p, _lib.c_long, _lib.c_void_p, _lib.c_void_p])

# dp.hip DpState: [DP_PARTS] fp64 partials, then 12 four-byte words {fp32 clip, fp32 sigma,
# uint32 seed_lo, seed_hi, stream, pad, uint64 t (two words), fp32 norm, int32 clipped, int32
# nonfinite, pad} (size and partial count checked against the library on a GPU)
DP_PARTS = 256
DP_WORDS = 12
_W_STREAM = 4  # last host-written word (clip, sigma, seed_lo, seed_hi, stream: words 0 - 4)
_W_NORM, _W_CLIPPED, _W_NONFINITE = 8, 9, 10
_Q_T = 3  # t as the fourth 8-byte word after the partials


def _check(name: str, value, positive: bool = False) -> float:
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"{name} must be a number, got {value!r}")
    v = float(value)
    if not (0.0 <= v <= 3.4e38) or (positive and v == 0.0):  # (an fp32 word on the device)
        raise ValueError(f"{name} must be a finite fp32 number {'> 0' if positive else '>= 0'}, "
                         f"got {value!r}")
    return v


def _i32(word: int) -> int:
    """The int32 with the bits of a uint32 word."""
    return struct.unpack("i", struct.pack("I", word & 0xFFFFFFFF))[0]


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class DPState:
    """The device block of one site's private releases and the release itself.

    ``privatize_(grad)`` replaces ``grad`` (contiguous fp32, numel a multiple of 4) by
    ``coef * grad + (noise_multiplier * clip_norm) * z``: ``G = ||grad||_2`` from an fp64 sum of
    squares, ``coef = fp32(min(1, clip_norm / (G + 1e-6)))`` (``G <= clip_norm``: exactly 1) and
    ``z`` standard normals from Philox4x32-10 at key ``seed``, counter ``(float4 index, t,
    stream)``, ``t`` the 1-based release number.  No two releases share a counter as long as
    ``(seed, stream)`` differ between sites, folds and phases.  A non-finite ``G`` makes the
    whole release NaN (it carries nothing) and counts in ``nonfinite``.  ``noise_multiplier = 0``
    skips the generator: with ``G <= clip_norm`` the gradient comes back bit for bit.

    ``clip_norm`` and ``noise_multiplier`` may be written from the host between replays of a
    captured graph (they are read on the device); a write inside a capture is refused."""

    def __init__(self, device, clip_norm: float, noise_multiplier: float = 0.0, seed: int = 0,
                 stream: int = 0):
        self.device = torch.device(device)
        c = _check("clip_norm", clip_norm, positive=True)
        s = _check("noise_multiplier", noise_multiplier)
        seed, stream = int(seed), int(stream)
        if not (0 <= seed < 2 ** 64):
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        if not (0 <= stream < 2 ** 32):
            raise ValueError(f"stream must be an integer in [0, 2^32), got {stream!r}")
        if self.device.type == "cuda":
            _lib.checked_struct(DP_PARTS * 8 + DP_WORDS * 4, "dn_dp_state_size", "dp state",
                                dn_dp_parts=DP_PARTS)
        self._clip_norm, self._sigma, self.seed, self.stream = c, s, seed, stream
        self._block = torch.zeros(DP_PARTS + DP_WORDS // 2, dtype=torch.float64, device=self.device)
        self._f = self._block[DP_PARTS:].view(torch.float32)
        self._i = self._block[DP_PARTS:].view(torch.int32)
        self._q = self._block[DP_PARTS:].view(torch.int64)
        self._write_host_words()

    def _write_host_words(self):
        """The host-written words from the host values (one small copy)."""
        w = struct.pack("ffiii", self._clip_norm, self._sigma, _i32(self.seed),
                        _i32(self.seed >> 32), _i32(self.stream))
        self._i[:_W_STREAM + 1].copy_(torch.tensor(struct.unpack("5i", w), dtype=torch.int32))

    def _refuse_in_capture(self, what: str):
        if self.device.type == "cuda" and _capturing():
            # the write would become a graph node that resets the value at every replay
            raise RuntimeError(f"DPState.{what} set inside a HIP graph capture")

    # host-written words ------------------------------------------------------------------------
    @property
    def clip_norm(self) -> float:
        return self._clip_norm

    @clip_norm.setter
    def clip_norm(self, value: float):
        v = _check("clip_norm", value, positive=True)
        self._refuse_in_capture("clip_norm")
        self._clip_norm = v
        self._write_host_words()

    @property
    def noise_multiplier(self) -> float:
        return self._sigma

    @noise_multiplier.setter
    def noise_multiplier(self, value: float):
        v = _check("noise_multiplier", value)
        self._refuse_in_capture("noise_multiplier")
        self._sigma = v
        self._write_host_words()

    # kernel-written words (one host read each) ---------------------------------------------------
    @property
    def releases(self) -> int:
        return int(self._q[_Q_T].item())

    @property
    def clipped(self) -> int:
        """Releases whose norm exceeded the threshold."""
        return int(self._i[_W_CLIPPED].item())

    @property
    def nonfinite(self) -> int:
        """Releases with a non-finite norm (all NaN)."""
        return int(self._i[_W_NONFINITE].item())

    @property
    def last_norm(self) -> float:
        """The last release's norm before the clip."""
        return float(self._f[_W_NORM].item())

    # the release ---------------------------------------------------------------------------------
    def privatize_(self, grad: torch.Tensor) -> torch.Tensor:
        if (grad.dtype != torch.float32 or not grad.is_contiguous() or grad.numel() % 4
                or grad.numel() == 0 or grad.device.type != self.device.type):
            raise ValueError("DPState.privatize_: a contiguous fp32 tensor on the state's device "
                             "with a multiple of 4 elements is required")
        if grad.is_cuda:
            _lib.call("dn_dp_privatize", grad.data_ptr(), grad.numel(), self._block.data_ptr(),
                      _lib.stream())
            return grad
        t = self.releases + 1
        self._q[_Q_T] = t
        c, s = _f32(self._clip_norm), _f32(self._sigma)
        _, G = reference.dp_coef(grad, c)
        Gf = _f32(G)
        self._f[_W_NORM] = Gf
        if not math.isfinite(Gf):
            self._i[_W_NONFINITE] += 1
        elif G > c:
            self._i[_W_CLIPPED] += 1
        if s == 0.0 and math.isfinite(Gf) and G <= c:
            return grad  # bit for bit
        grad.copy_(reference.dp_privatize(grad, c, s, self.seed, self.stream, t).to(torch.float32))
        return grad

    # resume --------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        return {"t": self.releases, "clipped": self.clipped, "nonfinite": self.nonfinite,
                "seed": self.seed, "stream": self.stream, "clip_norm": self._clip_norm,
                "noise_multiplier": self._sigma}

    def load_state_dict(self, sd: Dict[str, object]):
        """Continue a saved release sequence: the counter, the counts and the generator key and
        stream (the threshold and the multiplier stay as built)."""
        self._refuse_in_capture("load_state_dict")
        self.seed = int(sd.get("seed", self.seed))
        self.stream = int(sd.get("stream", self.stream))
        self._write_host_words()
        self._q[_Q_T] = int(sd.get("t", 0))
        self._i[_W_CLIPPED] = int(sd.get("clipped", 0))
        self._i[_W_NONFINITE] = int(sd.get("nonfinite", 0))
