"""An independent model of the gradient wire format (numpy only), written from the format
description at the top of ``csrc/kernels/payload.hip`` -- not from the kernels' code and not from
``parallel.collective``, which it is there to judge.

The format
----------
A payload is a run of sub-blocks ``[8-element header | 2,048 data elements]`` in the wire type
(fp16, bf16 or fp32); header element 0 holds the sub-block's integer exponent ``e`` as a wire
value, elements 1..7 are zero.  The data elements hold ``wire(x * scale * 2^e)``.  A rank-block of
``chunk`` data elements (a multiple of 2,048) is ``chunk / 2048`` sub-blocks; a payload of ``W``
ranks is ``W`` rank-blocks back to back, zero past the ``n`` source elements.

* pack: fp16 with ``scaled``: ``e = 15 - k`` where ``max |x| = f * 2^k`` with ``f`` in [0.5, 1)
  (so ``max |x| * 2^e < 2^15``), clamped to ``[E_LO, E_HI] = [-113, 100]``; ``e = 0`` when the
  maximum is zero, infinite or NaN (a NaN anywhere in the sub-block makes the maximum NaN).
  Every other wire: ``e = 0``.
* rowsum: sub-block ``s`` of the ``W`` rank-blocks -> one sub-block: ``emin = min_w e_w``,
  ``acc = sum_w wire_w * 2^-e_w`` in fp32 in site order starting from +0, the data are
  ``wire(acc * (scale * 2^emin))`` and the header is ``emin``.
* unpack: ``x = wire * (scale * 2^-e)``.

Arithmetic rules
----------------
Everything is numpy ``float32``.  Rounding to fp16 is ``astype(np.float16)``; rounding to bf16 is
round-to-nearest-even on the fp32 bit pattern (NaN stays NaN).  A multiplier is ONE fp32 product
``float32(scale) * 2^e`` (exact unless ``scale`` is itself within a factor 2^113 of the fp32
limits), and each element is multiplied by it once.

Un-scaling by ``2^-e`` is exact: a wire value is ``j * 2^q`` with ``|j| < 2^11`` (fp16), ``2^8``
(bf16) and ``q >= -24`` (fp16) or the value is an fp32 one (bf16 / fp32 wires, where ``e = 0``),
and with ``e <= 100`` the product ``j * 2^(q-e)`` is a multiple of ``2^-124`` with at most 11
significant bits -- representable -- while ``e >= -113`` and ``|wire| <= 2^15`` keep it below
``2^128``.  So ``acc + v * 2^-e`` rounds once whether the kernel contracts it into a fused
multiply-add or not, and this model (a product, then a sum) cannot differ from either.  The same
holds for the final ``wire * 2^-e`` of unpack at ``scale`` a power of two.

The fp64 truth and the per-element bound (``mean_bound``)
---------------------------------------------------------
Truth: ``m = sum_w float64(x_w) / W``.  With ``u`` the unit roundoff of the wire (2^-11 fp16,
2^-8 bf16, 2^-24 fp32) and ``h`` half its smallest spacing (2^-25 fp16, 2^-134 bf16, 0 fp32):

1. Site value.  ``x_w * 2^e_w`` is exact in fp32 (a power of two; where it underflows the fp32
   normal range the result is below ``2^-126 < h`` and the wire holds 0, an error below
   ``h``), then rounded once to the wire: the error of ``xhat_w = wire * 2^-e_w`` is at most
   ``d_w = max(u |x_w|, h 2^-e_w)`` (relative in the wire's normal range, absolute below it).
2. The fp32 sum of ``W`` terms from +0 makes ``W - 1`` roundings (sums in the subnormal range
   are exact), the multiplier ``float32(1/W) * 2^emin`` carries one (of 1/W), the product one
   more: ``g = (W+1) 2^-24 / (1 - (W+1) 2^-24)`` times ``S / W``, ``S = sum_w |xhat_w| <=
   sum_w (|x_w| + d_w)``.
3. The mean's single rounding to the wire: ``max(u |mhat|, h 2^-emin)`` with ``mhat`` the value
   the wire then holds (round-to-nearest errs by at most ``u`` times the ROUNDED value).
4. The final store ``wire * 2^-emin`` is exact unless it lands in the fp32 subnormal range, and
   a product of step 2 that is fp32-subnormal is rounded there before the wire rounds it again
   (bf16 / fp32 wires): one fp32 subnormal spacing, ``2^-149``, covers both.

``bound = sum_w d_w / W + g S / W + max(u |mhat|, h 2^-emin) + 2^-149``.  It presumes that
nothing overflows: the inputs are finite, ``sum_w |x_w| < 2^128`` (the fp32 sum is taken before
the division by ``W``) and, on the bf16 wire, no ``|x|`` rounds up to ``2^128``; where that fails
``mean_bound`` returns ``inf`` and the tests assert that it never does on the finite cases.
"""
import functools

import numpy as np

HDR = 8
SB = 2048
SBS = HDR + SB
E_LO, E_HI = -113, 100
WIRES = ("fp16", "bf16", "fp32")
U = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8, "fp32": 2.0 ** -24}
H = {"fp16": 2.0 ** -25, "bf16": 2.0 ** -134, "fp32": 0.0}
BITS = {"fp16": np.uint16, "bf16": np.uint16, "fp32": np.uint32}

MUTATIONS = ("amax_first_wave", "amax_ignores_nan", "emax", "round_every_add", "truncate",
             "header_late", "pad_not_zeroed", "clamp_m100")

f32 = np.float32


# ---- the wire types --------------------------------------------------------------------------
def encode(v, wire, mut=None):
    """fp32 values -> wire bits (round to nearest even; ``mut == "truncate"``: toward zero)."""
    v = np.ascontiguousarray(v, dtype=f32)
    if wire == "fp32":
        return v.view(np.uint32).copy()
    if wire == "fp16":
        with np.errstate(over="ignore", invalid="ignore"):
            r = v.astype(np.float16)
            if mut == "truncate":
                back = r.astype(f32)
                over = np.isfinite(v) & (np.abs(back) > np.abs(v))
                toward0 = np.nextafter(r, np.float16(0))
                r = np.where(over, toward0, r)
        return r.view(np.uint16).copy()
    u = v.view(np.uint32)
    if mut == "truncate":
        r = (u >> 16).astype(np.uint16)
    else:
        r = ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)
    nan = np.isnan(v)
    r[nan] = ((u[nan] >> 16) | np.uint32(0x7FC0)).astype(np.uint16)
    return r


def decode(bits, wire):
    """wire bits -> fp32 values (exact)."""
    bits = np.ascontiguousarray(bits)
    if wire == "fp32":
        return bits.view(f32).copy()
    if wire == "fp16":
        return bits.view(np.float16).astype(f32)
    return (bits.astype(np.uint32) << 16).view(f32)


def exp2(e):
    return np.ldexp(f32(1), np.asarray(e, dtype=np.int32)).astype(f32)


def block_exp(amax, lo=E_LO):
    """The exponents of sub-blocks whose max |x| is ``amax`` (fp32 array)."""
    amax = np.asarray(amax, dtype=f32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(amax) & (amax > 0)
    _, k = np.frexp(np.where(ok, amax, f32(1)))
    return np.where(ok, np.clip(15 - k, lo, E_HI), 0).astype(np.int32)


def numel(elems):
    return -(-int(elems) // SB) * SBS


def chunk_for(n, W):
    return max(SB, -(-int(n) // (SB * W)) * SB)


# ---- the three operations --------------------------------------------------------------------
def pack(x, W, chunk, wire, scale=1.0, scaled=True, mut=None, pad=7.0):
    """fp32 ``x`` [n] -> wire bits of ``W`` rank-blocks of ``chunk`` data elements."""
    x = np.asarray(x, dtype=f32).reshape(-1)
    n = x.size
    assert chunk % SB == 0 and W * chunk >= n
    nsb = W * chunk // SB
    body = np.full(nsb * SB, f32(pad) if mut == "pad_not_zeroed" else f32(0), dtype=f32)
    body[:n] = x
    b = body.reshape(nsb, SB)
    e = np.zeros(nsb, dtype=np.int32)
    if wire == "fp16" and scaled:
        a = np.abs(b[:, :512] if mut == "amax_first_wave" else b)
        amax = np.fmax.reduce(a, axis=1) if mut == "amax_ignores_nan" else a.max(axis=1)
        e = block_exp(amax, -100 if mut == "clamp_m100" else E_LO)
    sc = f32(scale) * exp2(e)
    out = np.zeros((nsb, SBS), dtype=BITS[wire])
    with np.errstate(over="ignore", invalid="ignore"):
        out[:, HDR:] = encode(b * sc[:, None], wire, mut).reshape(nsb, SB)
    out[:, 1 if mut == "header_late" else 0] = encode(e.astype(f32), wire)
    return out.reshape(-1)


def exponents(payload, wire):
    """The integer exponents in the headers of a payload of whole sub-blocks."""
    return decode(payload.reshape(-1, SBS)[:, 0], wire).astype(np.int32)


def rowsum(blocks, W, chunk, wire, scale, mut=None):
    """``W`` rank-blocks -> the wire bits of one: the scaled fp32 sum per sub-block."""
    nsb = chunk // SB
    v = np.asarray(blocks).reshape(W, nsb, SBS)
    es = decode(v[:, :, 0], wire).astype(np.int32).reshape(W, nsb)
    em = es.max(axis=0) if mut == "emax" else es.min(axis=0)
    acc = np.zeros((nsb, SB), dtype=f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for w in range(W):
            t = decode(v[w, :, HDR:], wire).reshape(nsb, SB) * exp2(-es[w])[:, None]
            if mut == "round_every_add":  # a 16-bit accumulator in the mean's own scale
                s_ = exp2(em)[:, None]
                acc = decode(encode((acc + t) * s_, wire), wire).reshape(nsb, SB) * exp2(-em)[:, None]
            else:
                acc = acc + t
        sc = f32(scale) * exp2(em)
        data = encode(acc * sc[:, None], wire, mut)
    out = np.zeros((nsb, SBS), dtype=BITS[wire])
    out[:, HDR:] = data.reshape(nsb, SB)
    out[:, 1 if mut == "header_late" else 0] = encode(em.astype(f32), wire)
    return out.reshape(-1)


def unpack(payload, n, wire, scale=1.0, mut=None):
    """The first ``n`` data elements of a payload of sub-blocks -> fp32."""
    nsb = -(-n // SB)
    v = np.asarray(payload)[:nsb * SBS].reshape(nsb, SBS)
    e = decode(v[:, 1 if mut == "header_late" else 0], wire).astype(np.int32)
    sc = f32(scale) * exp2(-e)
    with np.errstate(over="ignore", invalid="ignore"):
        out = decode(v[:, HDR:], wire).reshape(nsb, SB) * sc[:, None]
    return out.reshape(-1)[:n].astype(f32)


def site_mean(xs, wire, mut=None, stages=False):
    """The mean of the ``W`` site vectors ``xs`` as ``DirectMean.run_`` and ``PeerMean`` form it:
    pack per site, rank r takes rank-block r of every site, fp32 sum in site order times 1/W,
    the W mean blocks back to back, unpack.  ``stages``: also the payloads on the way."""
    W, n = len(xs), len(xs[0])
    chunk = chunk_for(n, W)
    blk = numel(chunk)
    sent = [pack(x, W, chunk, wire, mut=mut) for x in xs]
    means = [rowsum(np.concatenate([s[r * blk:(r + 1) * blk] for s in sent]), W, chunk, wire,
                    f32(1.0) / f32(W), mut=mut) for r in range(W)]
    gathered = np.concatenate(means)
    out = unpack(gathered, n, wire, mut=mut)
    return (out, sent, means) if stages else out


def gathered(x, wire):
    """What ``PeerGather`` hands every site for one site's vector: pack, then unpack."""
    x = np.asarray(x, dtype=f32)
    chunk = chunk_for(x.size, 1)
    return unpack(pack(x, 1, chunk, wire), x.size, wire)


# ---- truth and bound -------------------------------------------------------------------------
def truth(xs):
    return sum(np.asarray(x, dtype=np.float64) for x in xs) / len(xs)


def mean_bound(xs, wire, mhat):
    """The per-element bound of ``|mean - truth|`` derived in the module docstring; ``mhat`` is
    the mean under judgement (step 3 is relative to the rounded value)."""
    W, n = len(xs), len(xs[0])
    u, h = U[wire], H[wire]
    nsb = -(-n // SB)
    X = np.zeros((W, nsb * SB), dtype=np.float64)
    for w, x in enumerate(xs):
        X[w, :n] = np.abs(np.asarray(x, dtype=np.float64))
    if wire == "fp16":
        es = block_exp(X.reshape(W, nsb, SB).max(axis=2).astype(f32)).astype(np.float64)
    else:
        es = np.zeros((W, nsb))
    un = np.repeat(np.exp2(-es), SB, axis=1)                    # 2^-e_w per element
    d = np.maximum(u * X, h * un)
    S = (X + d).sum(axis=0)
    g = (W + 1) * 2.0 ** -24 / (1 - (W + 1) * 2.0 ** -24)
    r3 = np.maximum(u * np.abs(np.asarray(mhat, dtype=np.float64)),
                    (h * un.max(axis=0))[:n])                   # 2^-emin = max_w 2^-e_w
    b = (d.sum(axis=0) / W + g * S / W)[:n] + r3 + 2.0 ** -149
    over = S[:n] >= 2.0 ** 128
    if wire == "bf16":
        over |= X.max(axis=0)[:n] >= 2.0 ** 128 * (1 - 2.0 ** -9)
    return np.where(over, np.inf, b)


def err_ratio(out, xs, wire):
    """max over elements of ``|out - truth| / bound`` (inf where the bound is)."""
    b = mean_bound(xs, wire, out)
    if not np.all(np.isfinite(b)):
        return float("inf")
    return float((np.abs(np.asarray(out, dtype=np.float64) - truth(xs)) / b).max())


# ---- comparisons -----------------------------------------------------------------------------
def is_nan_bits(bits, wire):
    return np.isnan(decode(bits, wire))


def mismatches(got, want, wire):
    """Indices where two wire-bit arrays differ, positions where BOTH are NaN exempt."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    bad = got != want
    if bad.any():
        i = np.flatnonzero(bad)
        both = is_nan_bits(got[i], wire) & is_nan_bits(want[i], wire)
        return i[~both]
    return np.zeros(0, dtype=np.int64)


# ---- inputs ----------------------------------------------------------------------------------
POW2 = (-126, -86, -24, -14, 0, 14, 15, 16, 100, 115, 116, 127)
PATTERNS = (["zero", "negzero", "first_only", "last_only", "one_among_2^-30", "one_among_2^-45"]
            + [f"max_2^{k}{v}" for k in POW2 for v in ("", "-", "+")]
            + ["subnormal", "wide", "huge", "tiny"])


def _pattern(p, rng):
    """One sub-block of the named edge pattern ``PATTERNS[p]``."""
    name = PATTERNS[p]
    sign = np.where(rng.random(SB) < 0.5, f32(-1), f32(1))
    x = np.zeros(SB, dtype=f32)
    if name == "zero":
        return x
    if name == "negzero":
        return -x
    if name in ("first_only", "last_only"):
        # the maximum in the first / the last wave of the workgroup only
        x[0 if name == "first_only" else SB - 1] = f32(-(1 + rng.random()) * 2.0 ** int(rng.integers(-20, 10)))
        return x
    if name.startswith("one_among"):
        x[:] = sign * f32(2.0 ** (-30 if name.endswith("-30") else -45))
        x[(131 * p + 7) % SB] = f32(1)
        return x
    if name.startswith("max_2^"):
        k = int(name[6:].rstrip("+-"))
        top = f32(2.0 ** k)
        if name.endswith("-"):
            top = np.nextafter(top, f32(0))
        elif name.endswith("+"):
            top = np.nextafter(top, f32(np.inf))
        # everything else at most 2^(k-4): W of these sub-blocks still sum below 2^128
        x[:] = (rng.uniform(-1, 1, SB) * 2.0 ** (k - 4)).astype(f32)
        x[(131 * p + 7) % SB] = top * sign[0]
        return x
    if name == "subnormal":
        x[:] = f32(1e-40)
        return x
    z = rng.standard_normal(SB)
    if name == "wide":
        return (z * np.exp2(rng.integers(-40, 11, SB))).astype(f32)
    return (z * 2.0 ** (60 if name == "huge" else -100)).astype(f32)


def pattern_of(g, w, seed):
    return (g + w + seed) % len(PATTERNS)


def edge_gradients(n, W, seed=0):
    """``W`` fp32 vectors of ``n`` elements, sub-block g of site w holding pattern
    ``PATTERNS[(g + w + seed) % len(PATTERNS)]``: the sites disagree in every sub-block."""
    nsb = -(-n // SB)
    xs = []
    for w in range(W):
        x = np.empty(nsb * SB, dtype=f32)
        for g in range(nsb):
            p = pattern_of(g, w, seed)
            x[g * SB:(g + 1) * SB] = _pattern(p, np.random.default_rng([seed, g, w]))
        xs.append(x[:n].copy())
    return xs


def poisoned(xs):
    """``(ys, planted)``: copies of ``xs`` with, in site W-1, a NaN in sub-block 0 and +inf and
    -inf in two further sub-blocks, and +inf (site 0) against -inf (site W-1) at one index of a
    fourth; ``planted`` maps element index -> "nan" | "+inf" | "-inf", what the mean must hold
    there.  The infinities go into sub-blocks where every site's |x| is below 2^15 (an infinite
    maximum leaves an fp16 sub-block unscaled, and larger neighbours would overflow the wire and
    make infinities of their own); as many are planted as there are such sub-blocks."""
    W, n = len(xs), len(xs[0])
    ys = [x.copy() for x in xs]
    nsb = -(-n // SB)
    planted = {}

    def at(g):
        return g * SB + min(777 + g, n - 1 - g * SB)

    ys[W - 1][at(0)] = np.nan
    planted[at(0)] = "nan"
    quiet = [g for g in range(1, nsb)
             if max(float(np.abs(x[g * SB:(g + 1) * SB]).max()) for x in xs) < 2.0 ** 15]
    plan = (["pair"] if W > 1 else []) + ["+inf", "-inf"]
    for what, g in zip(plan, quiet):
        i = at(g)
        if what == "pair":
            ys[0][i], ys[W - 1][i] = np.inf, -np.inf
            planted[i] = "nan"
        else:
            ys[W - 1][i] = np.inf if what == "+inf" else -np.inf
            planted[i] = what
    return ys, planted


# ---- the shared grid -------------------------------------------------------------------------
def shapes():
    """(n, W) of the test grid."""
    return [(1, 1), (7, 2), (8, 2), (9, 2), (37, 2), (2047, 1), (2048, 1), (2049, 3), (4099, 3),
            (4 * 2 * SB, 4), (3 * 16 * SB + 9, 16)]


MODES = (("fp16", True), ("fp16", False), ("bf16", True), ("fp32", True))   # (wire, scaled)
SCALES = (1.0, 0.5, 1.0 / 3.0)


@functools.lru_cache(maxsize=None)
def inputs(n, W, poison):
    """The grid's site vectors of a shape (seeded by the shape, so that the small shapes see
    different patterns), read-only; with ``poison`` also what was planted."""
    xs = edge_gradients(n, W, seed=n % 1000 + W)
    planted = {}
    if poison:
        xs, planted = poisoned(xs)
    for x in xs:
        x.setflags(write=False)
    return tuple(xs), planted


@functools.lru_cache(maxsize=64)
def staged(n, W, wire, scaled, scale, poison):
    """The model's payloads of one grid case: every site's pack at ``scale``, every rank's rowsum
    at ``scale / W`` and the unpack at ``scale`` of the gathered means."""
    xs, _ = inputs(n, W, poison)
    chunk = chunk_for(n, W)
    blk = numel(chunk)
    sent = [pack(x, W, chunk, wire, scale, scaled) for x in xs]
    red = f32(scale) / f32(W)
    means = [rowsum(np.concatenate([s[r * blk:(r + 1) * blk] for s in sent]), W, chunk, wire, red)
             for r in range(W)]
    out = unpack(np.concatenate(means), n, wire, scale)
    return sent, means, out
