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


# ---- secure aggregation: pairwise-masked integer sums (csrc/kernels/secagg.hip) -------------------
SA_FRAC_BITS = 40        # q = int64(rint(g * 2^40))
SA_CLAMP = 2.0 ** 18     # |g| is clamped to 2^18 (counted as saturated)
SA_TAIL = 8              # the wire's extra block: [non-finite flag, saturated count, 0 x 6]
SA_MAX_PARTIES = 16      # 16 * 2^58 < 2^63
_CHACHA_CONST = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"


def chacha20_blocks(key, blocks, w13: int, w14: int, w15: int):
    """The ChaCha20 block function (20 rounds, RFC 7539 state layout) for every block index of
    ``blocks``: words 0-3 the constants, 4-11 the 256-bit ``key`` (32 bytes, or 8 uint32 words),
    12 the block index, 13-15 as given.  Returns the output words as uint32 ``[len(blocks), 16]``
    (their little-endian bytes are the key stream)."""
    import numpy as np
    if isinstance(key, (bytes, bytearray)):
        if len(key) != 32:
            raise ValueError("chacha20_blocks: a 32-byte key is required")
        key = np.frombuffer(bytes(key), dtype="<u4")
    key = np.asarray(key, dtype=np.uint32).reshape(8)
    b = np.asarray(blocks, dtype=np.uint64).reshape(-1)
    if b.size and int(b.max()) > 0xFFFFFFFF:
        raise ValueError("chacha20_blocks: the block index is a 32-bit word")
    nb = b.size
    init = np.empty((16, nb), dtype=np.uint32)
    for i, c in enumerate(_CHACHA_CONST):
        init[i] = c
    for i in range(8):
        init[4 + i] = key[i]
    init[12] = b.astype(np.uint32)
    init[13], init[14], init[15] = (np.uint32(int(w) & 0xFFFFFFFF) for w in (w13, w14, w15))
    x = [init[i].copy() for i in range(16)]

    def rotl(v, r):
        return (v << np.uint32(r)) | (v >> np.uint32(32 - r))

    def qr(a, b_, c, d):
        x[a] += x[b_]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b_] = rotl(x[b_] ^ x[c], 12)
        x[a] += x[b_]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b_] = rotl(x[b_] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        out = np.stack(x, axis=1)
        out += init.T
    return out


def secagg_domain(fold: int, phase: int) -> int:
    """The generator's domain word (state word 15) of a fold and phase (1: pretraining)."""
    return (int(fold) * 4096 + int(bool(phase)) * 2048) & 0xFFFFFFFF


def secagg_prg(key, n: int, t: int, domain: int):
    """The pair mask of release ``t`` (1-based) for a wire of ``n`` data words plus the tail
    block, as uint64 ``[n + 8]``: block ``b``'s 16 little-endian output words are the 8 masks of
    elements ``8b .. 8b+7``; the tail block is ``b = ceil(n / 8)`` and sits at word ``n``."""
    import numpy as np
    n, t = int(n), int(t)
    nb = -(-n // 8)
    w = chacha20_blocks(key, np.arange(nb + 1, dtype=np.uint64), t & 0xFFFFFFFF,
                        (t >> 32) & 0xFFFFFFFF, domain)
    m = np.ascontiguousarray(w).astype("<u4").view("<u8").reshape(-1).astype(np.uint64)
    return np.concatenate([m[:n], m[8 * nb:8 * nb + SA_TAIL]])


def secagg_quantize(grad):
    """``(wire, saturated, nonfinite)`` of one party's fp32 gradient before masking: uint64
    ``[n + 8]`` residues of ``int64(rint(clamp(g, +-2^18) * 2^40))`` (a non-finite element: 0),
    then the tail block ``[nonfinite 0/1, saturated count, 0 x 6]``."""
    import numpy as np
    g = np.ascontiguousarray(torch.as_tensor(grad).detach().cpu().reshape(-1).numpy(),
                             dtype=np.float32)
    fin = np.isfinite(g)
    sat = fin & (np.abs(g) > np.float32(SA_CLAMP))
    v = np.where(fin, np.clip(g, np.float32(-SA_CLAMP), np.float32(SA_CLAMP)), np.float32(0))
    with np.errstate(all="ignore"):
        q = np.rint(v.astype(np.float32) * np.float32(2.0 ** SA_FRAC_BITS)).astype(np.int64)
    nonfinite, saturated = int(not fin.all()), int(sat.sum())
    tail = np.zeros(SA_TAIL, dtype=np.int64)
    tail[0], tail[1] = nonfinite, saturated
    return np.concatenate([q, tail]).view(np.uint64), saturated, nonfinite


def secagg_mask(grad, keys, rank: int, t: int, domain: int):
    """Party ``rank``'s wire buffer of release ``t``: ``q + sum_{j > rank} PRG(k_j) - sum_{j <
    rank} PRG(k_j)`` mod 2^64 with ``keys[j]`` the pair key shared with party ``j``
    (``keys[rank]`` is not read).  uint64 ``[n + 8]``."""
    import numpy as np
    wire, _, _ = secagg_quantize(grad)
    n = wire.size - SA_TAIL
    with np.errstate(over="ignore"):
        for j, k in enumerate(keys):
            if j == rank:
                continue
            m = secagg_prg(k, n, t, domain)
            wire = wire + m if j > rank else wire - m
    return wire


def secagg_open(total, world: int):
    """``(mean fp32 [n], saturated, nonfinite)`` of the mod-2^64 sum ``total`` (uint64 ``[n +
    8]``) of ``world`` parties' wire buffers: ``fp32(double(int64(sum)) * (2^-40 / world))``; all
    NaN when the summed non-finite word is not 0."""
    import numpy as np
    total = np.asarray(total).view(np.uint64).reshape(-1)
    n = total.size - SA_TAIL
    c = 2.0 ** -SA_FRAC_BITS / int(world)
    s = total.view(np.int64)
    mean = (s[:n].astype(np.float64) * c).astype(np.float32)
    nonfinite, saturated = int(s[n] != 0), int(s[n + 1])
    if nonfinite:
        mean = np.full(n, np.nan, dtype=np.float32)
    return torch.from_numpy(mean), saturated, nonfinite


def secagg_mean(grads):
    """The opened mean of the parties' gradients (what every party holds after a release)."""
    import numpy as np
    with np.errstate(over="ignore"):
        total = sum(secagg_quantize(g)[0] for g in grads)
    return secagg_open(total, len(grads))


# ---- top-k sparsified release with error feedback (csrc/kernels/topk.hip) --------------------------
def _f32(a):
    import numpy as np
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().reshape(-1).numpy()
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1)


def topk_k(n: int, ratio: float) -> int:
    """``k = min(n, max(1, ceil(ratio * n)))``: the pairs a site releases per step."""
    import math
    return min(int(n), max(1, math.ceil(float(ratio) * int(n))))


def topk_select(g, err, k: int):
    """``(idx int32 [k], val fp32 [k], err_new fp32 [n])`` of one release: ``acc = g + err`` (one
    fp32 add), ``key = bits(acc) & 0x7fffffff`` (NaN > inf > finite, +-0 tie); the ``k`` largest
    keys are selected, the lower index winning among equal keys; the pairs come in ascending
    index order; ``err_new`` is ``+0`` where selected and ``acc`` elsewhere."""
    import numpy as np
    with np.errstate(all="ignore"):
        acc = _f32(g) + _f32(err)
    n, k = acc.size, int(k)
    if not (1 <= k <= n):
        raise ValueError(f"topk_select: k = {k} of n = {n}")
    key = (acc.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
    order = np.argsort(-key, kind="stable")  # (-key, i) ascending
    idx = np.sort(order[:k]).astype(np.int32)
    val = acc[idx].copy()
    err_new = acc.copy()
    err_new[idx] = np.float32(0.0)
    return idx, val, err_new


def topk_combine(pairs, n: int):
    """The dense fp32 ``[n]`` sum of the ranks' ``(idx, val)`` pairs: ``out[i] = ((+0 + v_0) +
    v_1) + ...`` over the ranks that selected ``i``, in rank order; ``+0`` elsewhere."""
    import numpy as np
    out = np.zeros(int(n), dtype=np.float32)
    with np.errstate(all="ignore"):
        for idx, val in pairs:
            idx = np.asarray(idx).astype(np.int64).reshape(-1)
            out[idx] = out[idx] + _f32(val)  # (one rank's indices are distinct)
    return out


# ---- coordinate-wise trimmed mean / median over sites (csrc/kernels/trimmed.hip) -------------------
def trimmed_b(W: int, trim="median") -> int:
    """Sites dropped at each end of a coordinate's sorted values: ``trim`` itself, or for
    ``"median"`` ``(W - 1) // 2`` (one value kept at odd ``W``, the two middle ones at even)."""
    W = int(W)
    return (W - 1) // 2 if trim == "median" else int(trim)


def trimmed_inv(W: int, b: int):
    """``float32(1) / float32(W - 2b)``: the host-made reciprocal every backend multiplies by."""
    import numpy as np
    return np.float32(1.0) / np.float32(int(W) - 2 * int(b))


def trimmed_mean(rows, b: int):
    """``(out fp32 [n], trimmed int64 [W])`` of the coordinate-wise trimmed mean of ``rows`` (fp32
    ``[W, n]``, one row per site in rank order) with ``b`` sites dropped at each end,
    ``0 <= 2b < W``.

    Order: ``u = bits(x)``, ``key(x) = u ^ 0x80000000`` when the sign bit is clear, else ``~u``,
    compared as unsigned 32-bit: the IEEE total order -NaN < -inf < ... < -0 < +0 < ... < +inf <
    +NaN.  Per coordinate the ``W`` entries are sorted ascending by ``(key, site index)``: a
    strict order that depends on the values alone.  Value: ``s = v[b]; s = s + v[b+1]; ...; s = s
    + v[W-1-b]`` in fp32 in sorted order; ``out = s`` when ``m = W - 2b`` is 1, else ``s * inv``
    with ``inv = float32(1) / float32(m)``: no division, no fused multiply-add.  Counts:
    ``trimmed[w]`` is the number of coordinates at which site ``w`` sat at a sorted position ``<
    b`` or ``>= W - b``.

    Consequences: a NaN always sorts to an end, so with ``b >= 1`` up to ``b`` non-finite sites per
    coordinate and sign never reach the update.  ``b = 0`` is a mean summed in VALUE order, not
    site order: not bitwise dSGD.  The median is ``b = (W - 1) // 2``: one value at odd ``W``, the
    mean of the two middle values at even ``W``.  ``W = 1`` is the identity (``b`` must be 0)."""
    import numpy as np
    if isinstance(rows, torch.Tensor):
        rows = rows.detach().cpu().numpy()
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    if rows.ndim != 2 or rows.shape[0] < 1:
        raise ValueError(f"trimmed_mean: rows must be [W, n], got {rows.shape}")
    W, n = rows.shape
    b = int(b)
    if not (0 <= 2 * b < W):
        raise ValueError(f"trimmed_mean: 0 <= 2b < W is required, got b = {b}, W = {W}")
    u = rows.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u ^ np.uint32(0x80000000)).astype(np.uint64)
    site = np.arange(W, dtype=np.uint64)[:, None]
    # (key, site) as one word: 32 key bits above 32 site bits, so any W sorts the same way
    word = np.sort((key << np.uint64(32)) | site, axis=0)
    ssite = (word & np.uint64(0xFFFFFFFF)).astype(np.int64)
    k32 = (word >> np.uint64(32)).astype(np.uint32)
    vals = np.where(k32 & np.uint32(0x80000000), k32 ^ np.uint32(0x80000000),
                    ~k32).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        s = vals[b].copy()
        for p in range(b + 1, W - b):
            s = s + vals[p]
        out = s if W - 2 * b == 1 else s * trimmed_inv(W, b)
    ends = np.concatenate([ssite[:b], ssite[W - b:]], axis=0).reshape(-1)
    trimmed = np.bincount(ends, minlength=W).astype(np.int64)
    return np.ascontiguousarray(out, dtype=np.float32), trimmed
