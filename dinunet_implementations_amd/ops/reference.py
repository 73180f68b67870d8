"""Pure-PyTorch restatement of the reference math.

This module is the numerics oracle: every HIP kernel is tested against it, and it is the
execution path on CPU (gloo plumbing tests, ``SiteRunner`` on a laptop).  It reproduces the
reference quirks listed in SURVEY.md Appendix A:

* A1  i, f, o gates use sigma(sigma(x)); g = tanh of the last quarter; gate rows ordered
  ``[i|f|o|g]`` (``comps/icalstm/models.py:32-37``).
* A2  per-direction hidden = hidden_size // 2; the reverse direction runs on the time-flipped
  sequence and its outputs stay in processing order (``models.py:55,62-63``).
* A3  ``num_layers`` is ignored (``models.py:52,57``).
* A4  the encoder sees each window flattened C-major then W (``models.py:107``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor


def lstm_cell_seq(x: Tensor, w_ih: Tensor, b_ih: Optional[Tensor], w_hh: Tensor,
                  b_hh: Optional[Tensor], h0: Optional[Tuple[Tensor, Tensor]] = None,
                  cell=None) -> Tuple[Tensor, Tuple[Tensor, Tensor]]:
    """One direction of the reference LSTMCell over a ``[B, S, I]`` sequence.

    Mirrors ``comps/icalstm/models.py:20-45`` (double sigmoid on i/f/o).
    Returns ``hidden_seq [B, S, H]`` and the final ``(h, c)``.
    """
    B, S, _ = x.shape
    H = w_hh.shape[1]
    if h0 is None:
        h = x.new_zeros(B, H)
        c = x.new_zeros(B, H)
    else:
        h, c = h0
    # the input projection is time-parallel: hoist it out of the recurrence
    xp = F.linear(x, w_ih, b_ih)
    outs = []
    hprevs = []
    for t in range(S):
        hprevs.append(h)
        pre = xp[:, t] + F.linear(h, w_hh, b_hh)
        s = pre[:, :3 * H].sigmoid()
        i = torch.sigmoid(s[:, :H])
        f = torch.sigmoid(s[:, H:2 * H])
        o = torch.sigmoid(s[:, 2 * H:3 * H])
        g = torch.tanh(pre[:, 3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        outs.append(h)
    if cell is not None and xp.requires_grad:
        from . import capture as _cap
        if _cap.active() is not None:
            # rank-dAD capture: d(pre_t) == d(xp_t) == d(h2h out_t) for every t
            a_ih = x.detach().reshape(B * S, -1)
            a_hh = torch.stack(hprevs, 1).detach().reshape(B * S, H)

            def _hook(g, cell=cell, a_ih=a_ih, a_hh=a_hh):
                d = g.detach().reshape(B * S, -1)
                _cap.record(cell.i2h, a_ih, d)
                _cap.record(cell.h2h, a_hh, d)
            xp.register_hook(_hook)
    return torch.stack(outs, 1), (h, c)


def bilstm(x: Tensor, params, bidirectional: bool = True, modules=None):
    """Reference bi-LSTM wrapper (``comps/icalstm/models.py:59-66``).

    ``params`` is a list (one per direction) of ``(w_ih, b_ih, w_hh, b_hh)``.
    """
    mods = list(modules) if modules is not None else [None, None]
    hs, (h, c) = lstm_cell_seq(x, *params[0], cell=mods[0])
    if bidirectional:
        rhs, (rh, rc) = lstm_cell_seq(torch.flip(x, (1,)), *params[1], cell=mods[1])
        hs = torch.cat([hs, rhs], 2)
        h = torch.cat([h, rh], 1)
        c = torch.cat([c, rc], 1)
    return hs, (h, c)


def ica_windows(data: Tensor, window_size: int, window_stride: int, temporal_size: int) -> Tensor:
    """``[N, C, T] -> [N, S, C, W]`` with ``S = int(T / W)`` and offset ``j * stride``.

    Reproduces quirk A9 (``comps/icalstm/__init__.py:28-32``): the window *count* comes from the
    window size, the *offset* from the stride.
    """
    S = int(temporal_size / window_size)
    idx = torch.arange(S).unsqueeze(1) * window_stride + torch.arange(window_size).unsqueeze(0)
    if int(idx.max()) >= data.shape[2]:
        raise ValueError(f"windowing needs {int(idx.max()) + 1} time points, data has "
                         f"{data.shape[2]}")
    # [N, C, S, W] -> [N, S, C, W]
    return data[:, :, idx].permute(0, 2, 1, 3).contiguous()


def softmax_ce(logits: Tensor, labels: Tensor, weight: Optional[Tensor] = None,
               label_smoothing: float = 0.0):
    """Reference ICA loss head (``comps/icalstm/__init__.py:60-63``).  ``weight`` (per-class) and
    ``label_smoothing`` are ``F.cross_entropy``'s, mean reduction: the batch's loss is divided by
    ``sum_i weight[y_i]`` of that batch."""
    prob = torch.softmax(logits, 1)
    if weight is None and not label_smoothing:
        loss = F.cross_entropy(logits, labels)
    else:
        loss = F.cross_entropy(logits, labels, weight=_loss_weight(weight, logits),
                               label_smoothing=float(label_smoothing))
    return prob, loss, prob.argmax(1)


def log_softmax_nll(logits: Tensor, labels: Tensor, weight: Optional[Tensor] = None,
                    label_smoothing: float = 0.0):
    """Reference FS loss head (``comps/fs/__init__.py:54-57``).  With ``weight`` or
    ``label_smoothing`` the loss is ``F.cross_entropy`` on the logits (``nll_loss(log_softmax(z))
    == cross_entropy(z)``; torch's ``nll_loss`` has no smoothing argument); ``out`` stays the
    log-probabilities."""
    out = F.log_softmax(logits, 1)
    if weight is None and not label_smoothing:
        loss = F.nll_loss(out, labels)
    else:
        loss = F.cross_entropy(logits, labels, weight=_loss_weight(weight, logits),
                               label_smoothing=float(label_smoothing))
    return out, loss, out.argmax(1)


def _loss_weight(weight, logits: Tensor) -> Optional[Tensor]:
    if weight is None:
        return None
    return torch.as_tensor(weight, dtype=logits.dtype, device=logits.device)


def adam_(params, grads, exp_avg, exp_avg_sq, step: int, lr: float, beta1: float = 0.9,
          beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
          max_grad_norm: Optional[float] = None):
    """torch.optim.Adam (non-amsgrad, L2 weight decay) restated on flat fp32 tensors.
    ``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_`` on ``grads`` first (the norm from an
    fp64 sum of squares; a non-finite norm leaves everything untouched)."""
    if max_grad_norm:
        norm = float(grads.double().square().sum()) ** 0.5
        if norm != norm or norm in (float("inf"), float("-inf")):
            return params
        coef = torch.tensor(min(1.0, float(max_grad_norm) / (norm + 1e-6)), dtype=torch.float32)
        grads = grads * coef
    g = grads if weight_decay == 0 else grads + weight_decay * params
    exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
    exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (exp_avg_sq.sqrt() / (bc2 ** 0.5)).add_(eps)
    params.addcdiv_(exp_avg, denom, value=-lr / bc1)
    return params


def ema_decay_at(t: int, decay: float, warmup: bool = True) -> float:
    """The decay of the weight average at update ``t`` (1-based), in double, as optim.hip
    ema_omd computes it: ``min(decay, (1 + t) / (10 + t))`` with the warmup on, else ``decay``,
    ``decay`` being the fp32 device word."""
    d = float(torch.tensor(float(decay), dtype=torch.float32))
    t = float(int(t))
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def ema_update(e: Tensor, p: Tensor, t: int, decay: float, warmup: bool = True) -> Tensor:
    """The weight average after update ``t`` in fp64: ``e + omd (p - e)`` with ``omd = 1 - d_t``
    rounded to fp32 once (the word the kernels multiply by), from the average ``e`` before and
    the updated parameters ``p``."""
    omd = float(torch.tensor(1.0 - ema_decay_at(t, decay, warmup), dtype=torch.float32))
    e64, p64 = e.detach().double(), p.detach().double()
    return e64 + omd * (p64 - e64)


# ---- differentially private gradient release (csrc/kernels/dp.hip) --------------------------------
_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): ``counter`` four and ``key`` two 32-bit words (ints
    or equal-shaped integer arrays); the four output words as a uint32 numpy array ``[4, ...]``."""
    import numpy as np
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(w, dtype=np.uint64) & m32 for w in counter)
    k0, k1 = (np.asarray(w, dtype=np.uint64) & m32 for w in key)
    for _ in range(10):
        p0 = np.uint64(_PHILOX_M0) * c0  # (< 2^64: both factors are 32-bit)
        p1 = np.uint64(_PHILOX_M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m32,
                          (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m32)
        k0 = (k0 + np.uint64(_PHILOX_W0)) & m32
        k1 = (k1 + np.uint64(_PHILOX_W1)) & m32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3)).astype(np.uint32)


def dp_noise(n: int, seed: int, stream: int, t: int) -> Tensor:
    """The ``n`` (a multiple of 4) standard normals of release ``t`` (1-based) as dp.hip draws
    them, in fp64: float4 ``i`` is one Philox call at counter ``(i, t_lo, t_hi, stream)``, key
    ``(seed_lo, seed_hi)``; outputs ``x_k`` give ``u_k = ((x_k >> 8) + 1) 2^-24`` in (0, 1] and
    the normals ``r0 cos(2 pi u1), r0 sin(2 pi u1), r1 cos(2 pi u3), r1 sin(2 pi u3)`` with
    ``r0 = sqrt(-2 ln u0)``, ``r1 = sqrt(-2 ln u2)``."""
    import numpy as np
    n, seed, stream, t = int(n), int(seed), int(stream), int(t)
    if n % 4 or n < 0:
        raise ValueError("dp_noise: n must be a multiple of 4")
    i4 = np.arange(n // 4, dtype=np.uint64)
    x = philox4x32_10((i4, t & 0xFFFFFFFF, (t >> 32) & 0xFFFFFFFF, stream & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u = ((x >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = 2.0 * np.pi * u[1], 2.0 * np.pi * u[3]
    z = np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=1)
    return torch.from_numpy(z.reshape(-1))


def dp_coef(grad: Tensor, clip_norm: float):
    """``(coef, G)`` of the release's clip: ``G = ||grad||_2`` from an fp64 sum of squares, ``coef
    = min(1, c / (G + 1e-6))`` rounded to fp32 once with ``c`` the fp32 device word (``G <= c``:
    exactly 1); both as Python doubles, ``G`` unrounded."""
    c = float(torch.tensor(float(clip_norm), dtype=torch.float32))
    G = float(grad.detach().double().square().sum()) ** 0.5 if grad.numel() else 0.0
    if G != G or G in (float("inf"), float("-inf")):
        return float("nan"), G
    return float(torch.tensor(min(1.0, c / (G + 1e-6)), dtype=torch.float32)), G


def dp_privatize(grad: Tensor, clip_norm: float, noise_multiplier: float, seed: int,
                 stream: int, t: int) -> Tensor:
    """Release ``t`` (1-based) of ``grad`` (fp32, numel a multiple of 4) as dp.hip computes it,
    in fp64: ``coef * grad + (sigma c) z`` with :func:`dp_coef`'s ``coef``, :func:`dp_noise`'s
    ``z`` and ``sigma``, ``c`` the fp32 device words.  A norm that is not finite in fp32 gives all
    NaN (the release carries nothing); ``sigma == 0`` adds nothing."""
    flat = grad.detach().reshape(-1).cpu()
    c = float(torch.tensor(float(clip_norm), dtype=torch.float32))
    s = float(torch.tensor(float(noise_multiplier), dtype=torch.float32))
    coef, G = dp_coef(flat, c)
    Gf = float(torch.tensor(G, dtype=torch.float32))
    if Gf != Gf or Gf in (float("inf"), float("-inf")):
        return torch.full(flat.shape, float("nan"), dtype=torch.float64).view(grad.shape)
    out = flat.double() * coef
    if s != 0.0:
        out = out + (s * c) * dp_noise(flat.numel(), seed, stream, t)
    return out.view(grad.shape)
