"""The reference of the low-rank kernel tests (``tests/lowrank_ref.py``) checked on the CPU, and
the conditions its inputs must meet before any GPU result is compared with it: unambiguous stop
decisions for every ``dad_tol`` case and unambiguous pivots for every dropped-column case."""
import math

import pytest
import torch

import lowrank_ref as ref
from dinunet_implementations_amd.parallel.lowrank import _mgs_torch_, dad_factors


@pytest.mark.parametrize("n,r", [(40, 1), (48, 4), (257, 10), (1024, 16)])
def test_cholqr_is_sign_fixed_householder_qr(n, r):
    P = ref.rand_p(n, r, 3).double()
    q, rr = torch.linalg.qr(P)
    q = q * torch.sign(rr.diagonal())[None, :]      # R with a positive diagonal, as Cholesky's
    Pn, piv, dead = ref.cholqr(P, info=True)
    assert not dead.any() and float(piv.min()) > 1e-2
    # fp64 CholQR loses cond(P)^2 * 2^-53; cond(P) is a few: 1e-12 leaves three digits to spare
    assert ref.relerr(Pn, q) < 1e-12
    assert ref.relerr(ref.orthonormality(Pn), torch.eye(r)) < 1e-12


def test_cholqr_drop_rule():
    for name, (P, dropped) in ref.drop_p_cases().items():
        Pn, piv, dead = ref.cholqr(P, info=True)
        assert sorted(torch.nonzero(dead).flatten().tolist()) == dropped, name
        assert torch.isfinite(Pn).all() and float(Pn[:, dropped].abs().max()) == 0.0, name
        live = [c for c in range(P.shape[1]) if c not in dropped]
        if live:  # the live columns are the QR of the live columns alone
            q, rr = torch.linalg.qr(P[:, live].double())
            q = q * torch.sign(rr.diagonal())[None, :]
            assert ref.relerr(Pn[:, live], q) < 1e-12, name


@pytest.mark.parametrize("shape", [(48, 66, 4), (256, 66, 10), (40, 100, 8)])
def test_power_iterate_spans_dad_factors(shape):
    out_f, in_f, r = shape
    G = ref.spectrum(out_f, in_f, ref.gapped(r), 5)
    # dad_factors draws its own start: the same draw, orthonormalised the same way
    q0 = _mgs_torch_(torch.randn(in_f, r, generator=torch.Generator().manual_seed(9)))
    p, q = dad_factors(torch.eye(out_f), G, r, 5, 0.0, generator=torch.Generator().manual_seed(9))
    Pn, Q, ran, _ = ref.power_iterate(G, q0, 5, 0.0)
    assert ran == 5
    want = Pn @ Q.t()
    b_p, b_q, _, _ = ref.power_iterate(G, q0, 5, 0.0, dtype=torch.float32)
    # P Q^T = Pn Pn^T G depends on span(Pn) alone: MGS and Cholesky QR agree to fp32 rounding
    ref.assert_close(p @ q.t(), want, b_p @ b_q.t(), f"dad_factors {shape}")


@pytest.mark.parametrize("n,r", [(5, 5), (40, 1), (769, 16)])
def test_mgs_is_the_engine_mgs(n, r):
    m = torch.randn(n, r, generator=torch.Generator().manual_seed(2))
    want = _mgs_torch_(m.clone())
    got = ref.mgs(m, dtype=torch.float32)
    assert ref.relerr(got, want) < 4 * ref.U23 * r  # the same sweep, up to fp32 summation order
    assert ref.relerr(ref.mgs(m), want) < 64 * ref.U23 * r


BASELINES = ({}, {"dtype": torch.float32}, {"dtype": torch.float32, "mm": ref.split3})


@pytest.mark.parametrize("shape", ref.TOL_STAGED + ref.TOL_PERSIST)
def test_tol_cases_are_unambiguous(shape):
    G, Q0, tol, k, ch = ref.tol_case(shape)
    assert all(c >= tol for c in ch[:k]) and ch[k] < tol
    assert ch[k - 1] / tol >= 3 and tol / ch[k] >= 3, (ch, tol)
    want = ref.power_iterate(G, Q0, ref.TOL_ITERS, tol)
    for kw in BASELINES:
        got = ref.power_iterate(G, Q0, ref.TOL_ITERS, tol, **kw)
        assert got[2] == k + 1, (kw, got[2])
        assert ref.dropped(got[0]) == ref.dropped(want[0]), kw   # a baseline drops what fp64 drops


@pytest.mark.parametrize("shape", ref.TOL_STAGED + ref.TOL_PERSIST)
def test_tol_cases_drop_decisions_are_clear(shape):
    """In fp64 and in both baseline precisions: no pivot or column norm near its threshold, and
    the same columns dropped at every iteration."""
    G, Q0, _, _, _ = ref.tol_case(shape)
    dead64 = ref.pivots(G, Q0, ref.TOL_ITERS)[2]
    for kw in BASELINES:
        assert ref.decisions_clear(G, Q0, ref.TOL_ITERS, **kw), kw
        assert torch.equal(ref.pivots(G, Q0, ref.TOL_ITERS, **kw)[2], dead64), kw


def test_gapped_cases_drop_nothing():
    for shape, seed in ref.gapped_cases():
        G, Q0 = ref.gapped_case(shape, seed)
        for kw in BASELINES:
            piv = ref.pivots(G, Q0, 5, **kw)[0]
            assert float(piv.min()) > 5e-6, (shape, seed, kw, float(piv.min()))


def test_dropped_pivots_are_unambiguous():
    cases = [P for P, _ in ref.drop_p_cases().values()]
    Q0 = ref.rand_orth(66, 4, 8)
    G2 = ref.exact_rank2(48, 66, 7)
    cases.append(ref.gq(G2, Q0)[1])
    cases.append(ref.gq(torch.zeros(48, 66), Q0)[1])
    for P in cases:
        piv = ref.cholqr(P, info=True)[1]
        assert all(p < 1e-10 or p > 1e-2 for p in piv.tolist()), piv


def test_split3_resolution():
    A = torch.randn(64, 256, generator=torch.Generator().manual_seed(1))
    B = torch.randn(256, 16, generator=torch.Generator().manual_seed(2))
    want = A.double() @ B.double()
    e3 = ref.relerr(ref.split3(A, B), want)
    # two bf16 parts keep 16 bits of each operand: the dropped lo*lo term is 2^-16 relative
    assert e3 < 2.0 ** -14
    assert e3 > ref.relerr(A @ B, want)
    ah = A.bfloat16().float()
    assert ref.relerr(ah @ B.bfloat16().float(), want) > 50 * e3  # one part alone is far off
    assert math.isfinite(e3)
