"""Plain fp64 reference of ONE launch of the fused Adam (``csrc/kernels/optim.hip`` adam_elem and
the prologue around it): numpy on the CPU, no project code.

``reference`` takes what the device holds before the launch -- ``p, g, m, v`` as fp32 arrays, the
update number ``t`` and the hyperparameters as fp32 words (``hyper``) plus the betas as doubles --
and returns the exact result of that one launch with a per-element error bound for each output.

Coefficients (``coefs``), as every step form computes them, in double and rounded to fp32 once::

    bc1  = f32(1 - b1d**t)          isb2 = f32(1 / sqrt(1 - b2d**t))          step = f32(lr / bc1)

Rule, everything in fp64 from the fp32 words (``1 - b`` is exact in fp32 for b in [0.5, 1], so
the kernel's ``1.f - b1`` and ``1.f - b2`` are the same numbers)::

    gr = g*gs + wd*p
    m' = b1*m + (1-b1)*gr
    v' = b2*v + (1-b2)*gr*gr
    p' = p - step*m' / (sqrt(v')*isb2 + eps)

One deviation from ``torch.optim.Adam`` is part of this reference and therefore not flagged by
it: ``1 - b2`` comes from the fp32 word ``0.999f = 0.999000012874603...``, not from the double
``1 - 0.999``.  ``v`` is relatively 1.29e-5 smaller than torch's and the update about 6e-6 larger.
The wrong reference ``omb2_double`` below takes the double; ``tests/test_adam_ref.py`` shows that
the bounds see it (so an error of 1e-5 in ``v`` does not pass).

Optional coefficients, from their documented formulas (not from ``FusedAdam.lr_at``, ``ops.optim.
clip_coef`` or ``ops.reference``, which mirror the code under test)::

    clip_gs    gs' = f32(gs * min(1, c / (G + 1e-6))),  G = gs * sqrt(fsum(g^2))
    sched_lr   w = t < W ? t/W : 1;  u = clamp((t-W)/(T-W), 0, 1);  r = lr_min/base
               d = 1 | 1-(1-r)u | r+(1-r) 0.5 (1+cos(pi u));  lr = f32(((base*scale)*w)*d)

Bounds
------
Per element, first order, ``u = 2^-24`` (one fp32 rounding is at most ``u`` of the rounded
value).  The unit of every bound is the magnitude of the TERMS of the sum, not of the result, so
cancellation does not need a wider constant::

    S_gr = |g*gs| + |wd*p|
    S_m  = |b1*m| + (1-b1)*S_gr
    S_v  = b2*v + (1-b2)*S_gr^2
    den  = sqrt(v')*isb2 + eps,    U = |step*m'/den|,    f = sqrt(v')*isb2/den

* ``|m_gpu - m'| <= K_m u S_m``, ``K_m = 6``: the two products and the sum of ``gr`` (3), then
  the products ``b1*m`` and ``(1-b1)*gr`` and their sum (3).  Each rounding is at most ``u`` of a
  quantity that ``S_m`` bounds.
* ``|v_gpu - v'| <= K_v u S_v``, ``K_v = 10``: ``gr`` carries ``3u`` of ``S_gr``, its square twice
  that plus the rounding of the product (7), then ``(1-b2)*``, ``b2*v`` and the sum (3).
* ``|p_gpu - p'| <= u (|p| + U) + step K_m u S_m / den + U (0.5 f K_v u S_v / v' + 5u)``: the
  final subtraction rounds once, at most ``u`` of ``|p| + U``; the error of ``m'`` reaches the
  update through ``step/den`` (written so that ``m' = 0`` needs no division); the relative error
  of ``v'`` reaches ``den`` halved by the root and scaled by ``f``, the share of ``den`` that is
  not ``eps``; and 5 more roundings: root, product with ``isb2``, sum with ``eps``, product
  ``step*m'``, quotient.  ``v' = 0`` happens only with ``g = 0, v = 0, wd = 0`` (then ``U = 0``
  too, and the term is taken as 0).

A contracted ``a*b + c`` (the library is built with ``-ffp-contract=fast``) rounds once less than
counted, never more.  The constants come from this count, not from the kernel.

Not resolved, and not claimed: a ``1 - b1`` taken from the double (``0.1`` instead of
``1 - 0.9f``) moves ``m`` by 4 units of ``u S_m``, which is below ``K_m``.

``emulate`` is the same rule in fp32 with numpy, rounded after every operation, with a switch that
fuses each ``a*b + c`` (the product exact in double, one rounding of the sum: a double rounding
that differs from a true fma in about one case in 2^29).  ``MUTATIONS`` are deliberately wrong
references; ``tests/test_adam_ref.py`` holds both emulations inside the bounds and requires every
wrong reference to break one by a factor of at least 4.
"""
import collections
import math

import numpy as np

U24 = 2.0 ** -24
K_M, K_V = 6.0, 10.0
N = 2053  # 513 float4 (more than one 256-thread workgroup) and a one-element scalar tail

MUTATIONS = ("eps_in_sqrt", "eps_before_bc", "no_isb2", "no_bc1", "adamw", "old_m", "wd_scaled",
             "omb2_double", "last_float4", "tail")
LENGTH_MUTATIONS = ("last_float4", "tail")

Hyper = collections.namedtuple("Hyper", "lr b1 b2 eps wd gs b1d b2d words")
Coef = collections.namedtuple("Coef", "bc1 isb2 step")
Result = collections.namedtuple("Result", "p m v bp bm bv")


def f32(x):
    """``x`` rounded to fp32 once, as a Python double."""
    return float(np.float32(x))


def hyper(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=0.0, gs=1.0, words=True):
    """The hyperparameters as the device holds them: fp32 words (as doubles) and the double
    betas.  ``words=False`` keeps every number a double and rounds no coefficient (the comparison
    with ``torch.optim.Adam`` in fp64)."""
    r = f32 if words else float
    b1, b2 = betas
    return Hyper(r(lr), r(b1), r(b2), r(eps), r(wd), r(gs), float(b1), float(b2), bool(words))


def coefs(h, t, lr=None):
    """``(bc1, isb2, step)`` of update ``t`` (``lr``: the scheduled rate in place of ``h.lr``)."""
    r = f32 if h.words else float
    bc1 = r(1.0 - h.b1d ** t)
    isb2 = r(1.0 / math.sqrt(1.0 - h.b2d ** t))
    return Coef(bc1, isb2, r((h.lr if lr is None else lr) / bc1))


def clip_gs(g, gs, c):
    """``(gs', G)`` of global-norm clipping at threshold ``c`` (fp32 words ``gs``, ``c``)."""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    G = gs * math.sqrt(math.fsum((g * g).tolist()))
    return f32(gs * min(1.0, c / (G + 1e-6))), G


def sched_lr(base, scale, lr_min, kind, W, T, t):
    """The scheduled rate of update ``t`` (fp32 words ``base``, ``scale``, ``lr_min``; ``kind``
    ``constant`` / ``linear`` / ``cosine``; ``W`` warmup updates, ``T`` schedule length)."""
    w = t / W if t < W else 1.0
    d = 1.0
    if kind != "constant" and T > W:
        u = min(max((t - W) / (T - W), 0.0), 1.0)
        r = lr_min / base if base > 0.0 else 1.0
        d = 1.0 - (1.0 - r) * u if kind == "linear" else r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * u))
    return f32(((base * scale) * w) * d)


def _f64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64).reshape(-1)


def reference(p, g, m, v, t, h, lr=None, gs=None, mutate=None):
    """One launch in fp64: ``Result(p', m', v', bound_p, bound_m, bound_v)``, float64 arrays.
    ``lr`` / ``gs``: the scheduled rate / the clipped gradient scale in place of ``h``'s.
    ``mutate``: one of ``MUTATIONS`` (a deliberately wrong reference)."""
    assert mutate is None or mutate in MUTATIONS, mutate
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    c = coefs(h, t, lr)
    gs = h.gs if gs is None else gs
    step = (h.lr if lr is None else lr) if mutate == "no_bc1" else c.step
    isb2 = 1.0 if mutate == "no_isb2" else c.isb2
    omb1, omb2 = 1.0 - h.b1, 1.0 - h.b2
    if mutate == "omb2_double":
        omb2 = 1.0 - h.b2d
    wd = 0.0 if mutate == "adamw" else h.wd
    gr = (g + wd * p) * gs if mutate == "wd_scaled" else g * gs + wd * p
    m1 = h.b1 * m + omb1 * gr
    v1 = h.b2 * v + omb2 * gr * gr
    if mutate == "eps_in_sqrt":
        den = np.sqrt(v1 + h.eps) * isb2
    elif mutate == "eps_before_bc":
        den = (np.sqrt(v1) + h.eps) * isb2
    else:
        den = np.sqrt(v1) * isb2 + h.eps
    p0 = p * (1.0 - (h.lr if lr is None else lr) * h.wd) if mutate == "adamw" else p
    upd = step * (m if mutate == "old_m" else m1) / den
    p1 = p0 - upd
    # bounds (module docstring)
    S_gr = np.abs(g * gs) + np.abs(wd * p)
    S_m = np.abs(h.b1 * m) + omb1 * S_gr
    S_v = h.b2 * v + omb2 * S_gr * S_gr
    Uu = np.abs(upd)
    f = np.sqrt(v1) * isb2 / den
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_v = np.where(v1 > 0, K_V * U24 * S_v / v1, 0.0)
    bm = K_M * U24 * S_m
    bv = K_V * U24 * S_v
    bp = U24 * (np.abs(p) + Uu) + step * bm / den + Uu * (0.5 * f * rel_v + 5.0 * U24)
    if mutate in LENGTH_MUTATIONS:
        n = p.size
        keep = slice(4 * (n // 4 - 1), 4 * (n // 4)) if mutate == "last_float4" else slice(4 * (n // 4), n)
        p1[keep], m1[keep], v1[keep] = p[keep], m[keep], v[keep]
    return Result(p1, m1, v1, bp, bm, bv)


def emulate(p, g, m, v, t, h, fuse=False, lr=None, gs=None):
    """The rule in fp32, rounded after every operation; ``fuse``: each ``a*b + c`` rounds once.
    Returns fp32 arrays ``(p', m', v')``."""
    F = np.float32
    p, g, m, v = (np.asarray(_f64(x), dtype=F) for x in (p, g, m, v))
    c = coefs(h, t, lr)
    gs = F(h.gs if gs is None else gs)
    b1, b2, eps, wd = F(h.b1), F(h.b2), F(h.eps), F(h.wd)
    step, isb2 = F(c.step), F(c.isb2)
    omb1, omb2 = F(1) - b1, F(1) - b2

    def mad(a, b, c_):  # a*b + c_
        if fuse:
            return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
                    + np.asarray(c_, np.float64)).astype(F)
        return (a * b).astype(F) + c_

    with np.errstate(all="ignore"):
        gr = mad(g, gs, (wd * p).astype(F))
        m1 = mad(b1, m, (omb1 * gr).astype(F))
        v1 = mad(b2, v, ((omb2 * gr).astype(F) * gr).astype(F))
        den = mad(np.sqrt(v1).astype(F), isb2, eps)
        p1 = p - ((step * m1).astype(F) / den).astype(F)
    return p1.astype(F), m1.astype(F), v1.astype(F)


def ratios(got, ref):
    """``{"p": .., "m": .., "v": ..}``: the largest ``|got - ref| / bound`` per output (an error
    where the bound is 0 counts as infinite, no error there as 0)."""
    out = {}
    for k, x, want, lim in zip("pmv", got, ref[:3], ref[3:]):
        err = np.abs(_f64(x) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(lim > 0, err / lim, np.where(err > 0, np.inf, 0.0))
        out[k] = float(r.max()) if r.size else 0.0
        if not np.all(np.isfinite(_f64(x))):
            out[k] = float("inf")
    return out


# ---------------------------------------------------------------------------------------------
# the input regimes shared by the CPU and the GPU test

Regime = collections.namedtuple("Regime", "p_scale g_scale t gs wd")


def regimes():
    """``{name: Regime}``: generic ``p ~ N(0, 1)`` and update-dominated ``p ~ 1e-4 N(0, 1)`` at
    ``t`` in {1, 2, 10, 1000, 100000}; ``g ~ 1e-10`` and ``g ~ 1e12``; ``grad_scale = f32(1/3)``;
    ``wd`` in {0, 1e-4}."""
    out = {}
    for t in (1, 2, 10, 1000, 100000):
        out[f"generic-t{t}"] = Regime(1.0, 1.0, t, 1.0, 1e-4)
        out[f"small-p-t{t}"] = Regime(1e-4, 1.0, t, 1.0, 1e-4)
    for t in (1, 10):
        out[f"small-p-wd0-t{t}"] = Regime(1e-4, 1.0, t, 1.0, 0.0)
    out["generic-wd0-t2"] = Regime(1.0, 1.0, 2, 1.0, 0.0)
    for t in (1, 1000):
        out[f"tiny-g-t{t}"] = Regime(1e-4, 1e-10, t, 1.0, 0.0)
        out[f"huge-g-t{t}"] = Regime(1e-4, 1e12, t, 1.0, 0.0)
    out["tiny-g-wd-t10"] = Regime(1e-4, 1e-10, 10, 1.0, 1e-4)
    out["third-generic-t1"] = Regime(1.0, 1.0, 1, 1.0 / 3.0, 1e-4)
    out["third-small-p-t10"] = Regime(1e-4, 1.0, 10, 1.0 / 3.0, 1e-4)
    return out


LAUNCHES = 4  # consecutive launches per regime, the state of one feeding the next


def regime_inputs(name, n=N):
    """``(p, m, v, [g of launch 0 .. LAUNCHES-1])`` of regime ``name`` as fp32 arrays, from a
    seeded generator.  ``t = 1`` starts from the zero moments of a fresh optimizer (there ``v'`` is
    all ``(1-b2) gr^2``), every other ``t`` from moments with a history (``m ~ 0.3 g``, ``v ~ (0.2
    .. 1.2) g^2``).  The tail element's gradient is ``+-4`` times the scale, so that every launch
    moves its ``m``, ``v`` and ``p`` by far more than a bound (``gr^2`` never meets ``v``)."""
    r = regimes()[name]
    rng = np.random.default_rng(sorted(regimes()).index(name) + 1000)
    F = np.float32
    p = (rng.standard_normal(n) * r.p_scale).astype(F)
    m = (rng.standard_normal(n) * 0.3 * r.g_scale).astype(F)
    v = ((0.2 + rng.random(n)) * r.g_scale ** 2).astype(F)
    if r.t == 1:
        m, v = np.zeros(n, dtype=F), np.zeros(n, dtype=F)
    gs = [(rng.standard_normal(n) * r.g_scale).astype(F) for _ in range(LAUNCHES)]
    for k, g in enumerate(gs):
        g[-1] = F(4.0 * r.g_scale * (-1) ** k)
    return p, m, v, gs


def regime_hyper(name):
    r = regimes()[name]
    return hyper(lr=1e-2, wd=r.wd, gs=r.gs)


# the flag test (clipping + schedule + average): gradients of norm about scale * sqrt(n) against a
# threshold CLIP_C * sqrt(n), alternately far below and far above it, grad_scale 1/3 included
CLIP_C = 1.0
CLIP_SCALES = (0.05, 10.0, 0.05, 10.0)
# cosine, warmup 2, lr_min at update 5: four updates cross the warmup and enter the decay
SCHEDULE = dict(kind="cosine", warmup_steps=2, decay_steps=5, lr_min=1e-3)


def clip_gradient(n, k):
    """The unit-scale gradient of launch ``k`` of the flag test (fp32, seeded)."""
    return np.random.default_rng(7000 + k).standard_normal(n).astype(np.float32)
