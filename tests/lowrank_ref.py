"""Plain torch reference of the low-rank gradient kernels (``csrc/kernels/lowrank.hip``): CPU only,
no project kernel.  Every function takes its precision from ``dtype``: fp64 is the reference the
GPU tests compare with, fp32 the baseline whose own error against fp64 sets their tolerance
(``assert_close``: kernel error <= 8 x max(baseline error, 2^-23), relative Frobenius).

The operations follow the kernels' formulas, not their schedules: ``P = (G + err) Q``, the
Cholesky QR ``Pn = P R^-1`` with the kernels' column-drop rule, ``Q = G^T Pn`` with the per-block
change norms, the ``dad_tol`` stop rule, the PowerSGD reconstruction with error feedback, the
rank-dAD mean of outer products and the modified Gram-Schmidt sweep.
"""
import math

import torch

EPS = 1e-8          # the kernels' guard in the relative change and in the MGS normalisation
U23 = 2.0 ** -23    # fp32 resolution: the floor of every baseline error


def _t(x, dtype):
    return x.detach().to("cpu", dtype)


def relerr(a, ref):
    """Relative Frobenius error of ``a`` against ``ref`` (both taken to fp64 on the CPU)."""
    a, ref = _t(a, torch.float64), _t(ref, torch.float64)
    den = float(ref.norm())
    return float((a - ref).norm()) / (den if den > 0 else 1.0)


# ---------------------------------------------------------------------------------------------
# operations

def gq(G, Q, err=None, dtype=torch.float64, mm=torch.matmul):
    """``M = G + err`` (``G`` itself without error feedback) and ``P = M Q``."""
    M = _t(G, dtype) if err is None else _t(G, dtype) + _t(err, dtype)
    return M, mm(M, _t(Q, dtype))


def cholqr(P, floor=1e-13, pivot=1e-6, dtype=torch.float64, info=False):
    """``Pn = P R^-1`` with ``R^T R = P^T P``, by the kernels' scaled Cholesky and drop rule: a
    column whose squared norm is ``<= floor * max`` is dropped, and so is one whose pivot in the
    Jacobi-scaled Gram (unit diagonal) is ``<= pivot``; a dropped column of ``Pn`` is zero and takes
    no part in the later eliminations.  ``info=True`` also returns the pivots met (0 for a column
    dropped by the floor) and the dropped mask."""
    P = _t(P, dtype)
    r = P.shape[1]
    A = P.t() @ P
    d = A.diagonal().clone()
    dmax = float(d.max()) if r else 0.0
    live = d > max(floor * dmax, 1e-280)
    s = torch.where(live, d.clamp_min(1e-300).rsqrt(), torch.zeros_like(d))
    As = A * s[:, None] * s[None, :]
    R = torch.zeros(r, r, dtype=dtype)      # R_s above the diagonal
    inv = torch.zeros(r, dtype=dtype)       # 1 / R_s[k][k], 0 for a dropped column
    piv = torch.zeros(r, dtype=dtype)
    dead = ~live
    for k in range(r):
        akk = float(As[k, k]) if live[k] else 0.0
        piv[k] = akk
        if dead[k] or akk <= pivot:
            dead[k] = True
            continue
        inv[k] = 1.0 / math.sqrt(akk)
        row = As[k, k + 1:] * inv[k]
        R[k, k + 1:] = row
        As[k + 1:, k + 1:] -= row[:, None] * row[None, :]
    x = P * s[None, :]
    for j in range(r):                      # forward substitution x <- x R_s^-1
        x[:, j] = x[:, j] * inv[j]
        x[:, j + 1:] -= x[:, j:j + 1] * R[j:j + 1, j + 1:]
    x[:, dead] = 0.0
    return (x, piv, dead) if info else x


def block_norms(Q, Q_prev):
    """Per block of 16 rows of ``Q``: ``(||Q - Q_prev||^2, ||Q||^2)`` as ``[blocks, 2]``."""
    n = Q.shape[0]
    nb = -(-n // 16)
    out = torch.zeros(nb, 2, dtype=Q.dtype)
    for b in range(nb):
        q, o = Q[16 * b:16 * b + 16], Q_prev[16 * b:16 * b + 16]
        out[b, 0] = ((q - o) ** 2).sum()
        out[b, 1] = (q ** 2).sum()
    return out


def gtp(G, P, Q_prev, dtype=torch.float64, mm=torch.matmul):
    """``Pn = cholqr(P)``, ``Q = G^T Pn`` and the per-block change norms against ``Q_prev``."""
    G = _t(G, dtype)
    Pn = cholqr(P, dtype=dtype)
    Q = mm(G.t(), Pn)
    return Pn, Q, block_norms(Q, _t(Q_prev, dtype))


def rel_change(norms):
    """The kernels' stop quantity from the per-block norms."""
    return math.sqrt(float(norms[:, 0].sum())) / (math.sqrt(float(norms[:, 1].sum())) + EPS)


def power_iterate(G, Q0, iters, tol=0.0, dtype=torch.float64, mm=torch.matmul):
    """The rank-dAD power iteration: returns ``Pn``, ``Q``, the iterations run and the relative
    change after each.  After the commit of iteration k the iteration stops when
    ``sqrt(sum D) / (sqrt(sum Qn) + 1e-8) < tol``: k + 1 iterations have then run."""
    G, Q = _t(G, dtype), _t(Q0, dtype)
    changes, Pn = [], None
    for _ in range(iters):
        _, P = gq(G, Q, dtype=dtype, mm=mm)
        Pn, Qn, nrm = gtp(G, P, Q, dtype=dtype, mm=mm)
        changes.append(rel_change(nrm))
        Q = Qn
        if tol > 0 and changes[-1] < tol:
            break
    return Pn, Q, len(changes), changes


def recon_ef(M, Pn, Q, dtype=torch.float64):
    """PowerSGD: ``G' = Pn Q^T`` and ``err' = M - G'``."""
    Gn = _t(Pn, dtype) @ _t(Q, dtype).t()
    return Gn, _t(M, dtype) - Gn


def pi_reconstruct(Ps, Qs, dtype=torch.float64):
    """rank-dAD: the mean over the sites of ``P_s Q_s^T``."""
    acc = None
    for P, Q in zip(Ps, Qs):
        t = _t(P, dtype) @ _t(Q, dtype).t()
        acc = t if acc is None else acc + t
    return acc / len(Ps)


def mgs(m, eps=EPS, dtype=torch.float64):
    """Modified Gram-Schmidt over the columns, each divided by ``norm + eps``."""
    m = _t(m, dtype).clone()
    for j in range(m.shape[1]):
        for i in range(j):
            m[:, j] -= (m[:, i] @ m[:, j]) * m[:, i]
        m[:, j] = m[:, j] / (m[:, j].norm() + eps)
    return m


def split3(A, B):
    """The persistent kernel's declared product precision: each fp32 operand as bf16 ``hi`` + bf16
    ``lo``, the product as ``lo*hi + hi*lo + hi*hi`` accumulated in fp32 (baseline only)."""
    A, B = _t(A, torch.float32), _t(B, torch.float32)
    ah = A.bfloat16().float()
    al = (A - ah).bfloat16().float()
    bh = B.bfloat16().float()
    bl = (B - bh).bfloat16().float()
    return (al @ bh + ah @ bl) + ah @ bh


def orthonormality(Pn, live=None):
    """``Pn^T Pn`` on the live columns (compare with the identity)."""
    Pn = _t(Pn, torch.float64)
    if live is not None:
        Pn = Pn[:, live]
    return Pn.t() @ Pn


# ---------------------------------------------------------------------------------------------
# inputs (all seeded, built in fp64, rounded to fp32)

def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def rand_orth(n, r, seed):
    """QR factor of an ``[n, r]`` Gaussian (orthonormal columns when ``n >= r``), fp32."""
    q, _ = torch.linalg.qr(torch.randn(n, r, generator=_gen(seed), dtype=torch.float64))
    return q.float()


def rand_p(n, r, seed):
    """A well-conditioned ``[n, r]`` factor that is not orthonormal: a QR factor times a
    unit-diagonal triangular mix (condition number of a few), fp32."""
    g = _gen(seed)
    q, _ = torch.linalg.qr(torch.randn(max(n, r), r, generator=g, dtype=torch.float64))
    t = torch.eye(r, dtype=torch.float64) + 0.3 * torch.randn(r, r, generator=g,
                                                             dtype=torch.float64).triu(1)
    scale = 0.5 + torch.rand(r, generator=g, dtype=torch.float64)
    return ((q @ t) * scale)[:n].float()


def spectrum(out_f, in_f, sigmas, seed, factors=False):
    """``U diag(s) V^T`` with seeded QR factors (as many singular values as fit), fp32;
    ``factors=True`` also returns the fp64 ``(U, s, V)``."""
    k = min(len(sigmas), out_f, in_f)
    g = _gen(seed)
    u, _ = torch.linalg.qr(torch.randn(out_f, k, generator=g, dtype=torch.float64))
    v, _ = torch.linalg.qr(torch.randn(in_f, k, generator=g, dtype=torch.float64))
    s = torch.tensor(list(sigmas)[:k], dtype=torch.float64)
    G = ((u * s) @ v.t()).float()
    return (G, (u, s, v)) if factors else G


def gapped(r):
    """``s_k = 32^(-k/r)`` for k < r, then ``s_(r-1) / 8 * 2^-(j+1)`` for 8 more: a spread below
    32 inside the rank and a gap after it, so ``Pn Pn^T G`` is well conditioned in fp32."""
    s = [32.0 ** (-k / r) for k in range(r)]
    return s + [s[-1] / 8 * 2.0 ** -(j + 1) for j in range(8)]


def gapped_case(shape, seed):
    """``(G, Q0)``: a ``gapped(r)`` spectrum and a random orthonormal start."""
    out_f, in_f, r = shape
    return spectrum(out_f, in_f, gapped(r), seed), rand_orth(in_f, r, seed + 1)


# every (shape, seed) the GPU tests run the power iteration on from ``gapped_case``
MIX = [(7, 5, 3), (256, 66, 10), (16, 16, 4), (25, 66, 10), (40, 100, 8), (33, 66, 3)]
NMIX = 19
MIXED8 = [(48, 64, 8), (40, 64, 5), (64, 32, 8), (33, 48, 5)] * 2
STAGED_SHAPES = [(256, 66, 10), (48, 64, 4), (40, 64, 3), (272, 1024, 16)]
PERSIST_SHAPES = [(48, 64, 4), (40, 64, 3), (256, 1000, 10), (272, 1024, 16), (25, 132, 10),
                  (1024, 64, 12), (64, 64, 13)]


def gapped_cases():
    cases = [(s, 31) for s in dict.fromkeys(STAGED_SHAPES + PERSIST_SHAPES)]
    cases += [(MIX[i % len(MIX)], 70 + i) for i in range(NMIX)]
    return cases + [(s, 90 + i) for i, s in enumerate(MIXED8)]


def geometric(ratio=4.0, n=12):
    return [float(ratio) ** -k for k in range(n)]


def exact_rank2(out_f, in_f, seed):
    """An fp32 matrix of exact rank 2 (small-integer factors: every entry is exact)."""
    g = _gen(seed)
    u = torch.randint(-3, 4, (out_f, 2), generator=g).double()
    v = torch.randint(-3, 4, (in_f, 2), generator=g).double()
    return (u @ v.t() / 8).float()


# ---------------------------------------------------------------------------------------------
# the dad_tol cases shared by the CPU conditions and the GPU tests

TOL_ITERS = 8
TOL_STOP = 3      # index k of the change the chosen tol first exceeds: k + 1 iterations run
TOL_STAGED = [(48, 66, 4), (40, 100, 8), (256, 66, 10)]
TOL_PERSIST = PERSIST_SHAPES
_tol_cache = {}


def warm_sigmas(r):
    """``32^(-k/r)`` inside the rank, then six more falling 4x each: the same 16x fall of the
    change per iteration as ``geometric(4)`` with every value far above fp32 rounding at any r."""
    s = [32.0 ** (-k / r) for k in range(r)]
    return s + [s[-1] * 4.0 ** -(j + 1) for j in range(6)]


def warm_start(V, r, seed, delta=0.3):
    """A start as a training step has it (the last step's Q): the leading ``r`` right singular
    vectors plus ``delta`` of the trailing ones, orthonormalised.  ``G Q0`` then has nearly
    orthogonal columns: every Cholesky pivot is near 1 and no drop decision is close, while a
    random start on a ``geometric(4)`` spectrum meets pivots of 16^-j, some within fp32 rounding
    of the 1e-6 drop threshold."""
    mix = torch.randn(V.shape[1] - r, r, generator=_gen(seed), dtype=torch.float64)
    q, rr = torch.linalg.qr(V[:, :r] + delta * (V[:, r:] @ mix))
    return (q * torch.sign(rr.diagonal())[None, :]).float()


def graded_start(V, sig, r, seed, delta=0.25):
    """The start a layer in steady state has on a graded spectrum (not orthonormal: Qsend is
    the last committed ``Q``).  Column j is ``v_j`` plus ``delta`` of the later leading vectors
    ``v_i``, ``j < i < r``: ``G Q0`` has column j led by ``sigma_j u_j``, and the mix of
    ``v_(j+1)`` into column j dies as ``(sigma_(j+1) / sigma_j)^2`` per iteration.  The columns
    the norm floor drops once ``Q`` carries the singular values (``(sigma_j / sigma_0)^4 <=
    1e-13``) are zero from the start, as a dropped column stays.  Measured on the CPU in fp64,
    fp32 and with split products: no pivot below 2e-4, the last live column's squared norm
    9.1e-13 of the largest (the floor is 1e-13) and the same columns dropped in all three.  (From
    a random orthonormal start on ``geometric(4)`` the pivots of the first two iterations fall as
    16^-j through the 1e-6 drop threshold, whatever the seed: an fp32 Gram then takes other drop
    decisions than an fp64 one, and they differ between hosts.)"""
    mix = torch.randn(r, r, generator=_gen(seed), dtype=torch.float64).tril(-1)
    q = V[:, :r] @ (torch.eye(r, dtype=torch.float64) + delta * mix)
    for j in range(r):
        if (sig[j] / sig[0]) ** 4 <= 1e-13:
            q[:, j] = 0.0
    return q.float()


def tol_case(shape, staged=None):
    """``(G, Q0, tol, k, fp64 changes)`` of a dad_tol case, ``tol`` the geometric mean of the fp64
    changes ``c_(k-1)`` and ``c_k``.  Staged cases: a ``geometric(4)`` spectrum from
    ``graded_start``, k = ``TOL_STOP``; at ranks 8 and 10 the columns from the seventh on are
    dropped by the norm floor in every iteration.  The
    persistent kernel's cases (ranks up to 16, products of 16-bit pairs, where 4^-15 would lie
    below the resolution): ``warm_sigmas(r)`` from ``warm_start``, k = ``TOL_STOP - 1``."""
    shape = tuple(shape)
    staged = shape in TOL_STAGED if staged is None else staged
    key = (shape, staged)
    if key not in _tol_cache:
        out_f, in_f, r = shape
        if staged:
            k = TOL_STOP
            G, (_, _, V) = spectrum(out_f, in_f, geometric(4.0, 12), 11, factors=True)
            Q0 = graded_start(V, geometric(4.0, 12), r, 12)
        else:
            k = TOL_STOP - 1
            G, (_, _, V) = spectrum(out_f, in_f, warm_sigmas(r), 11, factors=True)
            Q0 = warm_start(V, r, 12)
        ch = power_iterate(G, Q0, TOL_ITERS, 0.0)[3]
        _tol_cache[key] = (G, Q0, math.sqrt(ch[k - 1] * ch[k]), k, ch)
    return _tol_cache[key]


def pivots(G, Q0, iters, dtype=torch.float64, mm=torch.matmul):
    """Every Cholesky pivot the power iteration in ``dtype`` meets (``[iters, r]``; 0 for a column
    dropped by the floor), every squared column norm over the largest and the dropped mask of
    every iteration (``[iters, r]`` each)."""
    G, Q = _t(G, dtype), _t(Q0, dtype)
    piv, rat, dead = [], [], []
    for _ in range(iters):
        P = mm(G, Q)
        d = (P.double() ** 2).sum(0)
        rat.append(d / d.max().clamp_min(1e-300))
        Pn, pv, dd = cholqr(P, dtype=dtype, info=True)
        piv.append(pv.double())
        dead.append(dd)
        Q = mm(G.t(), Pn)
    return torch.stack(piv), torch.stack(rat), torch.stack(dead)


def decisions_clear(G, Q0, iters, dtype=torch.float64, mm=torch.matmul):
    """No drop decision of the iteration in ``dtype`` is close: every pivot is a factor 5 away
    from the 1e-6 threshold (an fp32 factorisation of the unit-diagonal Gram resolves a pivot to a
    few 1e-7), every squared column norm is 0 or a factor 5 away from 1e-13 of the largest."""
    piv, rat, _ = pivots(G, Q0, iters, dtype, mm)
    ok_p = (piv < 2e-7) | (piv > 5e-6)
    ok_r = (rat == 0) | (rat < 2e-14) | (rat > 5e-13)
    return bool(ok_p.all() and ok_r.all())


def dropped(Pn):
    """The columns of a factor that are entirely zero, as a list of bools."""
    return (_t(Pn, torch.float64) == 0).all(0).tolist()


def assert_close(got, ref64, base, what=""):
    """The tolerance rule: ``e_kernel <= 8 max(e_base, 2^-23)``; returns both errors."""
    e_k, e_b = relerr(got, ref64), relerr(base, ref64)
    assert math.isfinite(e_k), f"{what}: non-finite kernel output"
    assert e_k <= 8 * max(e_b, U23), f"{what}: e_kernel {e_k:.3e} > 8 max(e_base {e_b:.3e}, 2^-23)"
    return e_k, e_b


# ---------------------------------------------------------------------------------------------
# the dropped-column cases shared by the CPU conditions and the GPU tests

DROP_SHAPE = (40, 66, 5)


def drop_p_cases():
    """``{name: (P, dropped columns)}`` for the one-launch dropped-column tests."""
    n, _, r = DROP_SHAPE
    base = rand_p(n, r, 21)
    copy = base.clone()
    copy[:, 3] = copy[:, 1]
    zero = base.clone()
    zero[:, 2] = 0.0
    return {"copy": (copy, [3]), "zero_col": (zero, [2]),
            "all_zero": (torch.zeros(n, r), list(range(r)))}
