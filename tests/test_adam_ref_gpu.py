"""The fused Adam of ``csrc/kernels/optim.hip`` (adam_elem in adam_kernel and adam_pack_kernel,
the prologue adam_begin, slab_grad, pack_store / pack_store4) against the fp64 reference and the
derived per-element bounds of ``tests/adam_ref.py``.

Every comparison is per launch: ``p, g, m, v`` are read back, one launch runs, and its outputs are
held to the reference of that one launch; the GPU's own state then feeds the next launch, so the
moments are realistic and nothing drifts.  Each case prints its worst ``error / bound`` per
output.  ``tests/test_adam_ref.py`` shows on the CPU that the same bounds, on the same inputs,
hold an fp32 emulation of the rule and reject every wrong reference of ``adam_ref.MUTATIONS``.

1. the rule in every input regime, three step forms, four launches each, ``n = 2053``;
2. lengths: the scalar tail alone (1..3), around one float4, and one float4 row past
   ``dn_adam``'s 2048-workgroup cap, so the grid-stride loop runs twice; padding untouched;
3. the pack form through the C ABI past its 4096-workgroup cap;
4. clipping, schedule and average together, all four forms, with the reference's own clipped
   gradient scale and scheduled rate;
5. exact cases, bitwise;
6. ``slab_grad`` directly: hand-built slab sources, every loop remainder, wrong rows poisoned;
7. the operand images at ``pack_store4``'s fallback paths.

Measured on one MI355X, the largest ``error / bound`` of any case: ``p`` 0.998 (the pack form at
4,195,332 elements; the bound's first term is the half ulp of the final subtraction, which that
many elements come close to), ``m`` 0.498 and ``v`` 0.474 (``tiny-g-wd-t10``, all forms alike),
the slab gradient 0.436 (``SRC_COL | SRC_GATE``, 2 splits).  The three forms give the same figures
to the digit.  Run once against scratch builds of ``optim.hip`` with ``adam_elem`` edited, tests
of this file failed for each edit: ``eps`` moved inside the root 32 of 96 (every ``t = 1`` and
``tiny-g`` regime, the flag, slab and image tests), ``inv_sqrt_bc2`` dropped 87, ``p`` updated
from the old ``m`` 93, the scalar tail skipped 79.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import adam_ref as ar

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = ar.N
FORMS = ("step", "graphable", "prebumped")
PAD_M, PAD_V = 7.0, 9.0  # what the moments hold behind a sliced buffer


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    for k in ("DINUNET_EMA_DECAY", "DINUNET_LR_SCHEDULE", "DINUNET_MAX_GRAD_NORM"):
        monkeypatch.delenv(k, raising=False)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- a vector of n elements sliced from a padded buffer ------------------------------------------
class _Vector:
    """``FlatParams`` / ``FusedAdam`` over ``n`` elements that are the head of a longer buffer
    (``tests/adam_bits.py``'s trick: any ``n`` reaches the kernel, the scalar tail included); the
    gradient keeps its padded length (the norm kernel takes whole float4s).  ``full``: the
    unsliced buffers, whose padding no launch may touch."""

    def __init__(self, p, m, v, h, clip=0, sched=None, ema=0):
        from dinunet_implementations_amd.ops import FlatParams, FusedAdam
        n = self.n = p.size
        rng = np.random.default_rng(n)
        head = nn.Parameter(_dev(np.concatenate([p, rng.standard_normal(3).astype(np.float32)])))
        flat = self.flat = FlatParams([head])
        opt = self.opt = FusedAdam(flat, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=h.wd,
                                   max_grad_norm=clip, lr_schedule=sched, ema_decay=ema)
        assert (h.lr, h.b1d, h.b2d, h.eps) == (ar.f32(1e-2), 0.9, 0.999, ar.f32(1e-8))
        opt.exp_avg.fill_(PAD_M)
        opt.exp_avg_sq.fill_(PAD_V)
        opt.exp_avg[:n].copy_(_dev(m))
        opt.exp_avg_sq[:n].copy_(_dev(v))
        self.full = {"p": flat.data, "m": opt.exp_avg, "v": opt.exp_avg_sq}
        self.pad0 = {k: _bits(t[n:]).clone() for k, t in self.full.items()}
        flat.data = flat.data[:n]
        opt.exp_avg, opt.exp_avg_sq = opt.exp_avg[:n], opt.exp_avg_sq[:n]
        if ema:
            opt.ema = opt.ema[:n]
        self.gs = h.gs

    def set_grad(self, g, pad=0.5):
        self.flat.grad.fill_(pad)
        self.flat.grad[:self.n].copy_(_dev(g))

    def state(self):
        torch.cuda.synchronize()
        return _np(self.flat.data), _np(self.opt.exp_avg), _np(self.opt.exp_avg_sq)

    def padding_untouched(self):
        return all(torch.equal(_bits(t[self.n:]), self.pad0[k]) for k, t in self.full.items())


def _launch(form, flat, opt, gs, t):
    """Update number ``t`` by ``form``, host and device step numbers kept in step."""
    opt.step_count = t - 1
    if form == "step":
        opt.step(gs)
    else:
        opt.sync_device_step()
        if form == "graphable":
            opt.step_graphable(gs)
        else:
            opt.device_step().add_(1)  # what the caller's step prologue / encoder GEMM does
            if form == "prebumped":
                opt.step_graphable(gs, prebumped=True)
            else:
                opt.step_pack(gs)
        opt.step_count += 1
    torch.cuda.synchronize()
    assert opt.step_count == t


def _held(tag, got, ref):
    """Assert the outputs ``got = (p, m, v)`` inside the bounds of ``ref``; the ratios."""
    r = ar.ratios(got, ref)
    print(tag, "error / bound", {k: round(x, 3) for k, x in r.items()})
    assert all(x <= 1.0 for x in r.values()), (tag, r)
    return r


# ---- 1. the rule, every regime, three forms ------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ar.regimes()))
@pytest.mark.parametrize("form", FORMS)
def test_rule_in_every_regime(form, name):
    p, m, v, grads = ar.regime_inputs(name)
    h, t0 = ar.regime_hyper(name), ar.regimes()[name].t
    vec = _Vector(p, m, v, h)
    for k, g in enumerate(grads):
        vec.set_grad(g)
        before = vec.state()
        ref = ar.reference(before[0], g, before[1], before[2], t0 + k, h)
        _launch(form, vec.flat, vec.opt, ar.regimes()[name].gs, t0 + k)
        after = vec.state()
        _held(f"{form} {name} t={t0 + k}", after, ref)
        for new, old in zip(after, before):  # the launch did update, the scalar tail included
            assert not np.array_equal(new, old) and new[N - 1] != old[N - 1]
            assert np.count_nonzero(new != old) > 0.99 * N
        assert np.array_equal(_np(vec.flat.grad[:N]), g)  # these forms leave the gradient
    assert vec.padding_untouched()


# ---- 2. lengths ----------------------------------------------------------------------------------
PAST_CAP = 2048 * 256 * 4 + 1027  # one float4 row past dn_adam's grid cap, and a tail of 3


def _generic(n, seed, history=True):
    rng = np.random.default_rng(seed)
    F = np.float32
    p, g = rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)
    m = (0.3 * rng.standard_normal(n)).astype(F) if history else np.zeros(n, F)
    v = (0.2 + rng.random(n)).astype(F) if history else np.zeros(n, F)
    return p, g, m, v


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 1027, PAST_CAP])
@pytest.mark.parametrize("form", ["step", "graphable"])
def test_every_length_updates_every_element_and_nothing_else(form, n):
    p, g, m, v = _generic(n, n)
    g[-4:] = np.float32(4.0) * np.sign(g[-4:])  # (gr^2 far from v: the last elements must move)
    h = ar.hyper(wd=1e-4)
    vec = _Vector(p, m, v, h)
    vec.set_grad(g)
    ref = ar.reference(p, g, m, v, 3, h)
    _launch(form, vec.flat, vec.opt, 1.0, 3)
    after = vec.state()
    _held(f"{form} n={n}", after, ref)
    for new, old in zip(after, (p, m, v)):
        assert np.count_nonzero(new != old) > 0.99 * n - 1  # (n = 1: the one element may not)
    # every element, the last float4 and the tail by name: each moved off its input
    for new, old, want, lim in zip(after, (p, m, v), ref[:3], ref[3:]):
        moved = np.abs(want - old) > 2 * lim
        assert moved[-4:].all() and moved.sum() > 0.99 * n - 1
        assert np.array_equal(new[moved] != old[moved], np.ones(int(moved.sum()), bool))
    assert vec.padding_untouched()


# ---- the C ABI of the packing launch -------------------------------------------------------------
def _pack_call(p, g, m, v, t, h, segs=(), srcs=None, dims=(0, 0, 0), update=1, zero_grad=1):
    """``dn_adam_pack`` on device tensors ``p, g, m, v`` (no gather, no record): update number
    ``t`` from a device counter that already holds it (the prebumped form)."""
    from dinunet_implementations_amd.ops import _lib
    from dinunet_implementations_amd.ops.optim import _AdamArgs, _Seg, _Src
    _lib.checked_struct(_AdamArgs, "dn_adam_args_size", "adam argument block")
    _lib.checked_struct(_Seg, "dn_pack_seg_size", "pack segment")
    _lib.checked_struct(_Src, "dn_slab_src_size", "slab source")
    tdev = torch.tensor([t], dtype=torch.int32, device=DEV)
    args = _AdamArgs(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, p.numel(),
                     h.lr, h.b1, h.b2, h.eps, h.wd, h.gs, 1.0, 1.0, h.b1d, h.b2d,
                     tdev.data_ptr(), 0, 0, None, None, None, None)
    tab = (_Seg * max(1, len(segs)))(*[_Seg(*s) for s in segs])
    src = None
    if srcs is not None:
        src = (_Src * max(1, len(srcs)))(*[_Src(*s) for s in srcs])
    I, Hd, HD = dims
    _lib.call("dn_adam_pack", ctypes.addressof(args), int(update), int(zero_grad),
              ctypes.addressof(tab), len(segs), I, Hd, HD,
              None, 0, 0, None, None, 1, None, 0, None, None, None, 0, None,
              ctypes.addressof(src) if src is not None else None, _lib.stream())
    torch.cuda.synchronize()


# ---- 3. the pack form past its cap ---------------------------------------------------------------
def test_pack_form_past_its_workgroup_cap():
    n = 4096 * 256 * 4 + 4 * 257  # 257 float4s into the second pass of the stride loop
    p, g, m, v = _generic(n, 77)
    h = ar.hyper(wd=1e-4, gs=1.0 / 3.0)
    dp, dg, dm, dv = (_dev(x) for x in (p, g, m, v))
    ref = ar.reference(p, g, m, v, 2, h)
    _pack_call(dp, dg, dm, dv, 2, h)
    after = (_np(dp), _np(dm), _np(dv))
    _held(f"pack n={n}", after, ref)
    for new, old in zip(after, (p, m, v)):
        assert np.count_nonzero(new != old) > 0.99 * n
        assert not np.array_equal(new[-4 * 257:], old[-4 * 257:])  # the second pass
    assert int(torch.count_nonzero(dg)) == 0  # the gradient zeroed as it was consumed
    assert torch.equal(_bits(dg), torch.zeros_like(_bits(dg)))


# ---- bare LSTM parameters with a persistent pack -------------------------------------------------
def _bare_pack(I, Hd, ndir, seed, h, clip=0, sched=None, ema=0):
    """Parameters of an ``ndir``-direction LSTM (``W_ih [4Hd, I]``, ``b_ih``, ``W_hh [4Hd, Hd]``,
    ``b_hh``) and two cast tensors of 7 and 10 elements in one flat buffer, their
    ``PersistentPack`` attached to the optimizer.  No model."""
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.ops.lstm import PersistentPack
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: nn.Parameter(torch.randn(*s, generator=gen).to(DEV))
    ps = []
    for _ in range(ndir):
        ps += [mk(4 * Hd, I), mk(4 * Hd), mk(4 * Hd, Hd), mk(4 * Hd)]
    casts = [mk(7), mk(10)]
    flat = FlatParams(ps + casts)
    opt = FusedAdam(flat, lr=1e-2, weight_decay=h.wd, max_grad_norm=clip, lr_schedule=sched,
                    ema_decay=ema)
    pp = PersistentPack(ps, I, torch.device(DEV), casts=casts)
    opt.attach_pack(pp)
    return ps, casts, flat, opt, pp


def _images(pp):
    return [pp.wih_p, pp.bias_p, pp.whh_p, pp.whhT_p] + pp.casts


def _assert_images(pp, ps, casts, I):
    """Every image equals ``dn_lstm_pack`` of the current parameters bit for bit, every cast
    ``p.to(bfloat16)``, and the padded rows and columns are zero."""
    from dinunet_implementations_amd.ops.lstm import pack_params
    out = []
    wih, bias, whh, whhT, _ = pack_params(ps, I, torch.device(DEV), casts=casts, cast_out=out)
    torch.cuda.synchronize()
    assert torch.equal(pp.wih_p, wih) and torch.equal(pp.whh_p, whh)
    assert torch.equal(pp.whhT_p, whhT)
    nb = bias.numel()
    assert torch.equal(pp.bias_p[:nb] + pp.bias_p[nb:], bias)
    for img, fresh, c in zip(pp.casts, out, casts):
        assert torch.equal(img, fresh) and torch.equal(img, c.detach().to(torch.bfloat16))
        assert float(img.float().abs().max()) > 0
    Hd, HD, nd = pp.Hd, pp.HD, pp.ndir
    assert float(pp.wih_p.float().abs().max()) > 0 and float(pp.whh_p.float().abs().max()) > 0
    assert int(torch.count_nonzero(pp.wih_p.view(nd, HD, 4, I)[:, Hd:])) == 0
    assert int(torch.count_nonzero(pp.bias_p.view(2, nd, HD, 4)[:, :, Hd:])) == 0
    w_hh = torch.stack([ps[4 * d + 2].detach().to(torch.bfloat16) for d in range(nd)])
    for img in (pp.whh_p, pp.whhT_p):  # whatever the layout: nothing beyond the real entries
        assert int(torch.count_nonzero(img)) == int(torch.count_nonzero(w_hh))
    if HD <= 192:
        a, b = pp.whh_p.view(nd, HD, 4, HD), pp.whhT_p.view(nd, HD, HD, 4)
        assert int(torch.count_nonzero(a[:, Hd:])) == 0 == int(torch.count_nonzero(a[..., Hd:]))
        assert int(torch.count_nonzero(b[:, Hd:])) == 0 == int(torch.count_nonzero(b[:, :, Hd:]))
        for d in range(nd):  # [m = 4u + g][k] of reference row g Hd + u, and its transpose
            want = w_hh[d].view(4, Hd, Hd).permute(1, 0, 2)
            assert torch.equal(a[d, :Hd, :, :Hd], want)
            assert torch.equal(b[d, :Hd, :Hd, :], want.permute(2, 0, 1))


# ---- 4. clipping, schedule and average together --------------------------------------------------
@pytest.mark.parametrize("form", FORMS + ("pack",))
def test_flags_together_use_the_reference_scale_and_rate(form):
    h = ar.hyper(wd=1e-4, gs=1.0 / 3.0)
    sc = dict(ar.SCHEDULE)
    if form == "pack":
        ps, casts, flat, opt, pp = _bare_pack(6, 6, 1, 5, h, clip=1.0, sched=sc, ema=0.9)
        n = nfull = flat.data.numel()
        assert nfull == 356
    else:
        p, _, m, v = _generic(N, 21, history=False)
        vec = _Vector(p, m, v, h, clip=1.0, sched=sc, ema=0.9)
        flat, opt, n, nfull = vec.flat, vec.opt, N, vec.flat.grad.numel()
    c = ar.CLIP_C * math.sqrt(nfull)
    opt.max_grad_norm = c
    base, lo = ar.f32(1e-2), ar.f32(sc["lr_min"])
    sides, rates = [], []
    for k, scale in enumerate(ar.CLIP_SCALES):
        t = k + 1
        g = ar.clip_gradient(nfull, k) * np.float32(scale)
        flat.grad.copy_(_dev(g))
        torch.cuda.synchronize()
        before = (_np(flat.data), _np(opt.exp_avg), _np(opt.exp_avg_sq))
        e0 = opt.ema.clone()
        gs1, G = ar.clip_gs(g, h.gs, ar.f32(c))
        lr_t = ar.sched_lr(base, 1.0, lo, sc["kind"], sc["warmup_steps"], sc["decay_steps"], t)
        ref = ar.reference(before[0], g[:n], before[1], before[2], t, h, lr=lr_t, gs=gs1)
        _launch(form, flat, opt, 1.0 / 3.0, t)
        after = (_np(flat.data), _np(opt.exp_avg), _np(opt.exp_avg_sq))
        _held(f"{form} flags t={t} G/c={G / c:.3g} lr={lr_t:.4g}", after, ref)
        assert abs(float(opt.grad_norm) - G) <= 1e-6 * G and int(opt.skipped_steps) == 0
        got = np.float32(float(opt.applied_lr))
        assert abs(float(got) - lr_t) <= float(np.spacing(np.float32(lr_t))), (float(got), lr_t)
        assert (gs1 == h.gs) == (G < c)
        sides.append(G > c)
        rates.append(lr_t)
        assert not torch.equal(opt.ema, e0)  # the average follows
        if form == "pack":
            assert int(torch.count_nonzero(flat.grad)) == 0
            _assert_images(pp, ps, casts, 6)
    assert sides == [False, True, False, True]
    assert rates[0] == ar.f32(base * 0.5) and rates[1] == base and lo < rates[3] < rates[2] < base
    if form != "pack":
        assert vec.padding_untouched()


# ---- 5. exact cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["step", "graphable"])
def test_zero_gradient_on_zero_moments_changes_nothing(form):
    p, _, m, v = _generic(N, 31, history=False)
    vec = _Vector(p, m, v, ar.hyper())
    vec.set_grad(np.zeros(N, np.float32))
    _launch(form, vec.flat, vec.opt, 1.0, 1)
    for new, old in zip(vec.state(), (p, m, v)):
        assert np.array_equal(new.view(np.int32), old.view(np.int32))
    assert vec.padding_untouched()


@pytest.mark.parametrize("form", ["step", "graphable"])
def test_zero_gradient_decays_the_moments_exactly(form):
    p, _, m, v = _generic(N, 32)
    h = ar.hyper()
    vec = _Vector(p, m, v, h)
    vec.set_grad(np.zeros(N, np.float32))
    ref = ar.reference(p, np.zeros(N), m, v, 5, h)
    _launch(form, vec.flat, vec.opt, 1.0, 5)
    after = vec.state()
    assert np.array_equal(after[1], np.float32(h.b1) * m)  # m' = fl(b1 m)
    assert np.array_equal(after[2], np.float32(h.b2) * v)  # v' = fl(b2 v)
    assert not np.array_equal(after[1], m) and not np.array_equal(after[2], v)
    _held(f"{form} g=0", after, ref)
    assert not np.array_equal(after[0], p)


def test_priming_launch_leaves_p_m_v():
    h = ar.hyper(wd=1e-4)
    ps, casts, flat, opt, pp = _bare_pack(6, 6, 1, 6, h)
    n = flat.data.numel()
    opt.exp_avg.copy_(_dev((0.3 * np.random.default_rng(1).standard_normal(n)).astype(np.float32)))
    opt.exp_avg_sq.fill_(0.5)
    flat.grad.copy_(_dev(ar.clip_gradient(n, 0)))
    torch.cuda.synchronize()
    before = [_bits(t).clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)]
    assert all(int(torch.count_nonzero(t)) == 0 for t in _images(pp))
    opt.step_count = 3
    opt.sync_device_step()
    opt.step_pack(update=False)
    torch.cuda.synchronize()
    for t, b in zip((flat.data, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(_bits(t), b)
    assert int(torch.count_nonzero(flat.grad)) == 0
    _assert_images(pp, ps, casts, 6)


# ---- 6. slab_grad directly -----------------------------------------------------------------------
SRC_ROWS, SRC_COL, SRC_GATE = 1, 2, 4
PK_CAST = 1
POISON = 1e30  # in every slab row / column that must not be read, and in g


def _slab_case(mode, splits, beta, seed):
    """One ``dn_adam_pack`` launch whose only segment takes its gradient from a hand-built slab
    source; ``(largest error / bound of m', ...)``.  ``m = v = 0``, ``wd = 0``, ``gs = 1``:
    ``m' = (1-b1) alpha sum_s slab`` exposes the gradient ``slab_grad`` formed."""
    gate, col = bool(mode & SRC_GATE), bool(mode & SRC_COL)
    Hd, HD = 6, 64
    M, Nc = (4 * HD if gate else 24), (3 if col else 8)
    rows = 4 * Hd if gate else M
    n = rows if col else rows * Nc
    rng = np.random.default_rng(seed)
    slab = np.full((splits, M, Nc), POISON, dtype=np.float32)
    # segment element j -> slab (row, column)
    j = np.arange(n)
    r, k = (j, np.zeros(n, int)) if col else (j // Nc, j % Nc)
    if gate:
        r = 4 * (r % Hd) + r // Hd  # reference row g Hd + u -> slab row 4 u + g
    slab[:, r, k] = rng.standard_normal((splits, n)).astype(np.float32)
    assert np.count_nonzero(slab == np.float32(POISON)) == splits * (M * Nc - n)
    alpha = ar.f32(1.0 / 3.0)
    h = ar.hyper()
    p = rng.standard_normal(n).astype(np.float32)
    dp, dm, dv = _dev(p), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    dg = torch.full((n,), POISON, device=DEV)
    dslab = _dev(slab)
    img = torch.zeros(n, dtype=torch.bfloat16, device=DEV)
    _pack_call(dp, dg, dm, dv, 1, h, segs=[(0, n, PK_CAST, 0, img.data_ptr(), None)],
               srcs=[(dslab.data_ptr(), slab.size, M, Nc, splits, mode, alpha, float(beta))],
               dims=(8, Hd, HD))
    used = slab[:, r, k].astype(np.float64)  # [splits][n]
    grad = alpha * used.sum(0)
    omb1 = 1.0 - h.b1
    lim = (splits + 3) * ar.U24 * omb1 * alpha * np.abs(used).sum(0)
    err = np.abs(_np(dm).astype(np.float64) - omb1 * grad)
    assert float(lim.min()) > 0 and np.all(np.isfinite(_np(dm)))
    ratio = float((err / lim).max())
    assert ratio <= 1.0, (mode, splits, beta, ratio)
    # and the rest of the launch from that gradient: v' and p' within their bounds widened by
    # what the gradient's own error eg brings (first order: 2 |g| eg on g^2, and twice the
    # relative error on an update in which m' and sqrt(v') both carry it), the zeroed g, the image
    ref = ar.reference(p, grad, np.zeros(n), np.zeros(n), 1, h)
    eg = lim / omb1
    assert np.all(np.abs(_np(dv) - ref.v) <= ref.bv + (1 - h.b2) * (2 * np.abs(grad) * eg + eg * eg))
    upd = np.abs(ref.p - p)
    assert float(np.abs(grad).min()) > 0 and float(upd.min()) > 1e-3
    assert np.all(np.abs(_np(dp) - ref.p) <= ref.bp + 2 * upd * eg / np.abs(grad))
    assert np.all(_np(dp) != p)
    assert int(torch.count_nonzero(dg)) == 0
    assert torch.equal(img, dp.to(torch.bfloat16))
    return ratio


@pytest.mark.parametrize("mode", [SRC_ROWS, SRC_COL, SRC_ROWS | SRC_GATE, SRC_COL | SRC_GATE])
def test_slab_grad_sums_the_right_rows_in_every_loop_shape(mode):
    worst = (0.0, None)
    for splits in (2, 3, 4, 6, 7, 8, 9):
        for beta in (0, 1):
            r = _slab_case(mode, splits, beta, 100 * mode + splits)
            worst = max(worst, (r, (splits, beta)))
    print("slab mode", mode, "worst error / bound", round(worst[0], 3), "at (splits, beta)", worst[1])


# ---- 7. the images at pack_store4's fallback paths -----------------------------------------------
@pytest.mark.parametrize("I,Hd", [(6, 6), (20, 50), (8, 200)])
def test_images_at_the_fallback_paths(I, Hd):
    """(6, 6): ``I % 4 != 0`` and ``Hd % 4 != 0``; (20, 50): the W_ih fast path beside the W_hh
    fallback; (8, 200): ``HD = 256``, the fragment layout.  The casts of 7 and 10 elements end in
    a partial float4."""
    h = ar.hyper(wd=1e-4)
    ps, casts, flat, opt, pp = _bare_pack(I, Hd, 2, 10 * I + Hd, h)
    n = flat.data.numel()
    assert pp.HD == (256 if Hd == 200 else 64)
    real = np.zeros(n, bool)  # (the alignment gaps between tensors hold p = g = 0: exact case)
    for q, o, cnt in flat.segments():
        real[o:o + cnt] = True
    g = ar.clip_gradient(n, 3) * real
    flat.grad.copy_(_dev(g))
    torch.cuda.synchronize()
    before = (_np(flat.data), _np(opt.exp_avg), _np(opt.exp_avg_sq))
    ref = ar.reference(before[0], g, before[1], before[2], 1, h)
    _launch("pack", flat, opt, 1.0, 1)
    after = (_np(flat.data), _np(opt.exp_avg), _np(opt.exp_avg_sq))
    _held(f"pack images I={I} Hd={Hd}", after, ref)
    assert np.all(after[0][real] != before[0][real]) and np.array_equal(after[0][~real], before[0][~real])
    assert int(torch.count_nonzero(flat.grad)) == 0
    _assert_images(pp, ps, casts, I)


def test_cast_image_at_a_destination_that_is_not_8_byte_aligned():
    n, SENT = 1036, -1232.0  # 259 float4: two workgroups
    p, g, m, v = _generic(n, 55)
    h = ar.hyper()
    ref = ar.reference(p, g, m, v, 4, h)
    outs = []
    for shift in (1, 0):  # one bf16 element = 2 bytes off, then aligned
        dp, dg, dm, dv = (_dev(x) for x in (p, g, m, v))
        buf = torch.full((n + 8,), SENT, dtype=torch.bfloat16, device=DEV)
        dst = buf.data_ptr() + 2 * shift
        assert (dst % 8 != 0) == bool(shift)
        _pack_call(dp, dg, dm, dv, 4, h, segs=[(0, n, PK_CAST, 0, dst, None)])
        _held(f"pack cast shift={shift}", (_np(dp), _np(dm), _np(dv)), ref)
        assert torch.equal(buf[shift:shift + n], dp.to(torch.bfloat16))
        rest = torch.cat([buf[:shift], buf[shift + n:]])
        assert bool((rest == SENT).all())
        outs.append((dp, dm, dv))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
