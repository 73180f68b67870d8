"""``tests/adam_ref.py`` on the CPU: the fp64 reference of one fused-Adam launch against
``torch.optim.Adam``, its bounds against two fp32 emulations of the rule, and every deliberately
wrong reference against those bounds.  No project kernel runs here; ``tests/test_adam_ref_gpu.py``
holds ``optim.hip`` to the same reference and the same bounds on the same inputs.

Which regime catches which wrong reference (``test_every_wrong_reference_breaks_a_bound``; the
largest ``|fp32 emulation - wrong reference| / bound`` over all regimes, the output and the regime
it occurs in, as measured here)::

    eps_in_sqrt    p  1.4e+11  tiny-g-t1         (sqrt(1e-8) against sqrt(v') ~ 1e-12)
    eps_before_bc  p  4.2e+07  tiny-g-t1         (eps scaled by 1/sqrt(bc2) = 31.6)
    no_isb2        p  9.6e+05  small-p-t1
    no_bc1         p  1.3e+07  tiny-g-t1
    adamw          m  3.2e+09  tiny-g-wd-t10     (wd*p is nearly all of gr there); v and p too
    old_m          p  2.8e+06  huge-g-t1
    wd_scaled      v  8.7e+05  third-generic-t1  (m 8.6e+05, p 902; invisible with grad_scale 1)
    omb2_double    v  21.9     generic-t1;       p 6.5 in small-p-t1
    last_float4    p, m, v > 1e6, and >= 4 in every regime (the elements keep their old values)
    tail           p, m, v > 1e6, and >= 4 in every regime

The two ``eps`` placements need a gradient near ``eps`` (``tiny-g``): with ``g ~ 1`` they move the
update by 1e-8 relatively, which no fp32 test can see.  ``omb2_double`` -- the deviation from
torch the module docstring of ``adam_ref`` describes, relatively 1.29e-5 on the new part of ``v``
-- is the narrowest: 21.6 bounds of ``v`` (216 units of ``u S_v``) where ``v'`` is all
``(1-b2) gr^2``, that is at ``t = 1`` from the zero moments of a fresh optimizer; with a history
in ``v`` only a thousandth of it is new and the difference drowns.  ``1 - b1`` from the double
would be 4 units of ``u S_m``, below ``K_m = 6``: not resolved, not claimed.
"""
import math

import numpy as np
import pytest
import torch

import adam_ref as ar

F32_MIN = float(np.finfo(np.float32).tiny)
F32_MAX = float(np.finfo(np.float32).max)


# ---- 1. the reference itself ---------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_reference_is_torch_adam_in_fp64(wd):
    rng = np.random.default_rng(3)
    n = 257
    p = torch.nn.Parameter(torch.tensor(rng.standard_normal(n), dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    h = ar.hyper(lr=1e-2, wd=wd, words=False)
    rp, rm, rv = p.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n)
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        rp, rm, rv = ar.reference(rp, g, rm, rv, t, h)[:3]
        st = opt.state[p]
        for got, want in ((rp, p.detach().numpy()), (rm, st["exp_avg"].numpy()),
                          (rv, st["exp_avg_sq"].numpy())):
            err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            assert float(err.max()) <= 1e-12, (t, float(err.max()))


def test_coefficients_are_fp32_words():
    h = ar.hyper(lr=1e-2)
    assert h.b2 == float(np.float32(0.999)) and h.b2d == 0.999 and h.b2 != h.b2d
    # 1 - b from the fp32 word is itself an fp32 number (what the kernel's 1.f - b gives)
    for b in (h.b1, h.b2):
        assert float(np.float32(1.0 - b)) == 1.0 - b
        assert float(np.float32(1) - np.float32(b)) == 1.0 - b
    # the deviation from torch: 1 - 0.999f is relatively 1.29e-5 below the double 1 - 0.999
    assert abs(((1.0 - h.b2d) - (1.0 - h.b2)) / (1.0 - h.b2d) - 1.29e-5) < 1e-7
    c = ar.coefs(h, 1)
    assert c.bc1 == ar.f32(1 - 0.9) and c.step == ar.f32(h.lr / c.bc1)
    assert c.isb2 == ar.f32(1 / math.sqrt(1 - 0.999))
    c = ar.coefs(h, 100000)
    assert c.bc1 == 1.0 and c.isb2 == 1.0 and c.step == h.lr


def test_schedule_and_clip_formulas():
    b, lo = ar.f32(1e-2), ar.f32(1e-3)
    assert ar.sched_lr(b, 1.0, lo, "constant", 0, 0, 7) == b
    assert ar.sched_lr(b, 1.0, lo, "cosine", 2, 5, 1) == ar.f32(b * 0.5)      # warmup
    assert ar.sched_lr(b, 1.0, lo, "cosine", 2, 5, 2) == b                    # its end
    assert ar.sched_lr(b, 1.0, lo, "cosine", 2, 5, 5) == ar.f32(b * (lo / b))  # the floor
    assert ar.sched_lr(b, 1.0, lo, "linear", 2, 6, 4) == ar.f32(b * (1 - (1 - lo / b) * 0.5))
    mid = ar.sched_lr(b, 0.5, lo, "cosine", 2, 6, 4)
    assert mid == ar.f32((b * 0.5) * (lo / b + (1 - lo / b) * 0.5 * (1 + math.cos(math.pi / 2))))
    g = np.full(16, 0.5, dtype=np.float32)  # norm 2
    assert ar.clip_gs(g, 1.0, 10.0) == (1.0, 2.0)
    gs, G = ar.clip_gs(g, 1.0, 1.0)
    assert G == 2.0 and gs == ar.f32(1.0 / (2.0 + 1e-6))
    third = ar.f32(1 / 3)
    gs, G = ar.clip_gs(g, third, 0.25)
    assert G == third * 2.0 and gs == ar.f32(third * (0.25 / (G + 1e-6)))


# ---- 2. the bounds hold the fp32 rule ------------------------------------------------------------
def _run(name, fuse):
    """The LAUNCHES launches of regime ``name`` by the emulation, each judged against the
    reference of that launch: ``[(inputs, emulated outputs, reference)]``."""
    p, m, v, gs = ar.regime_inputs(name)
    h, t = ar.regime_hyper(name), ar.regimes()[name].t
    out = []
    for k, g in enumerate(gs):
        ref = ar.reference(p, g, m, v, t + k, h)
        got = ar.emulate(p, g, m, v, t + k, h, fuse=fuse)
        out.append(((p, g, m, v, t + k), got, ref))
        p, m, v = got
    return out


@pytest.fixture(scope="module")
def runs():
    return {(name, fuse): _run(name, fuse) for name in ar.regimes() for fuse in (False, True)}


def test_regime_list_is_the_one_the_issue_names():
    rs = ar.regimes().values()
    assert {r.t for r in rs} == {1, 2, 10, 1000, 100000}
    assert {r.p_scale for r in rs} == {1.0, 1e-4} and {r.wd for r in rs} == {0.0, 1e-4}
    assert {r.g_scale for r in rs} == {1.0, 1e-10, 1e12}
    assert {ar.f32(r.gs) for r in rs} == {1.0, ar.f32(1 / 3)}
    for p in (1.0, 1e-4):
        assert {r.t for r in rs if r.p_scale == p and r.g_scale == 1.0} >= {1, 2, 10, 1000, 100000}


@pytest.mark.parametrize("fuse", [False, True])
def test_both_fp32_emulations_stay_inside_the_bounds(runs, fuse):
    worst = {"p": (0, ""), "m": (0, ""), "v": (0, "")}
    for name in ar.regimes():
        for k, (_, got, ref) in enumerate(runs[(name, fuse)]):
            for o, r in ar.ratios(got, ref).items():
                worst[o] = max(worst[o], (r, f"{name} launch {k}"))
                assert r <= 1.0, (name, k, o, r)
    print("fused" if fuse else "plain", {o: (round(r, 3), w) for o, (r, w) in worst.items()})
    # the bounds are not slack by orders of magnitude either: the rule uses a fair part of them
    assert worst["m"][0] > 0.2 and worst["v"][0] > 0.2 and worst["p"][0] > 0.2


def test_inputs_meet_what_the_gpu_test_relies_on(runs):
    """No ``v' = 0``, every magnitude (squares included) in the fp32 normal range, every launch
    moves the tail element of every output, and the tail exists."""
    assert ar.N % 4 == 1 and ar.N // 4 > 256
    for (name, fuse), launches in runs.items():
        for (p, g, m, v, t), got, ref in launches:
            r = ar.regimes()[name]
            gr = np.abs(g.astype(np.float64) * ar.f32(r.gs)) + np.abs(ar.f32(r.wd) * p.astype(np.float64))
            for x in (np.abs(p), np.abs(g), np.abs(m), v, gr, gr * gr * (1 - ar.f32(0.999)),
                      ref.v, np.abs(ref.m), np.abs(ref.p)):
                x = np.asarray(x, dtype=np.float64)
                if r.t == 1 and (x is m or x is v) or not x.any():
                    continue  # (the zero moments of a fresh optimizer)
                assert float(x.min()) >= F32_MIN and float(x.max()) <= F32_MAX / 4, name
            assert float(ref.v.min()) > 0
            # the tail element moves by more than twice its bound (so any result inside the bound
            # differs from the input), and nearly every other element moves too
            for new, old, want, lim in zip(got, (p, m, v), ref[:3], ref[3:]):
                assert abs(want[-1] - float(old[-1])) > 2 * lim[-1] > 0, name
                assert np.count_nonzero(new != old) > 0.99 * ar.N, name


def test_clip_inputs_keep_away_from_the_threshold():
    """The flag test's gradients: norms well below and well above the threshold, none within
    1e-3 relative of it (the fp64 norm of the reference and the device's partial sums may then
    differ in the last bits without changing which branch is taken)."""
    below = above = 0
    for n in (ar.N + 3, 356):
        for k, scale in enumerate(ar.CLIP_SCALES):
            g = ar.clip_gradient(n, k) * np.float32(scale)
            for gs in (1.0, ar.f32(1 / 3)):
                c = ar.CLIP_C * math.sqrt(n)
                _, G = ar.clip_gs(g, gs, ar.f32(c))
                assert abs(G - c) > 1e-3 * c
                below += G < 0.5 * c
                above += G > 2 * c
    assert below and above


# ---- 3. the bounds see every wrong reference -----------------------------------------------------
def _worst_against(mutate, runs):
    """Largest ``|emulation - wrong reference| / wrong reference's bound`` per output over all
    regimes and launches, with where it occurs."""
    worst = {"p": (0.0, ""), "m": (0.0, ""), "v": (0.0, "")}
    for name in ar.regimes():
        h = ar.regime_hyper(name)
        for (p, g, m, v, t), got, _ in runs[(name, True)]:
            bad = ar.reference(p, g, m, v, t, h, mutate=mutate)
            for o, r in ar.ratios(got, bad).items():
                worst[o] = max(worst[o], (r, name))
    return worst


@pytest.mark.parametrize("mutate", ar.MUTATIONS)
def test_every_wrong_reference_breaks_a_bound(runs, mutate):
    worst = _worst_against(mutate, runs)
    print("\n" + mutate, {o: (f"{r:.3g}", w) for o, (r, w) in worst.items()})
    assert max(r for r, _ in worst.values()) >= 4.0, worst
    if mutate in ar.LENGTH_MUTATIONS:
        # every output, in every regime: the skipped elements keep their inputs
        for name in ar.regimes():
            (p, g, m, v, t), got, _ = runs[(name, False)][0]
            bad = ar.reference(p, g, m, v, t, ar.regime_hyper(name), mutate=mutate)
            assert all(r >= 4.0 for r in ar.ratios(got, bad).values()), name
        return
    if mutate == "wd_scaled":
        # invisible wherever grad_scale is 1
        for name, r in ar.regimes().items():
            if r.gs == 1.0:
                (p, g, m, v, t), got, ref = runs[(name, False)][0]
                bad = ar.reference(p, g, m, v, t, ar.regime_hyper(name), mutate=mutate)
                assert all(np.array_equal(a, b) for a, b in zip(bad[:3], ref[:3]))
        return


def test_one_minus_b2_from_the_double_is_seen_on_v_and_p(runs):
    """The deviation from torch, 1.29e-5 of ``v``: far above the unit of the ``v`` bound."""
    worst = _worst_against("omb2_double", runs)
    assert worst["v"][0] >= 20 and worst["p"][0] >= 4, worst
    assert worst["m"][0] <= 1.0  # m does not depend on b2
