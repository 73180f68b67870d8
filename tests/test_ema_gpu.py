"""The weight average of the fused Adam on the GPU (optim.hip ema_omd and the EMA forms of
adam_kernel / adam_pack_kernel, elementwise.hip swap_f32_kernel): the per-step rule against the
fp64 mirror, the update left bit for bit as it was, the three step forms (and the slab-fed pack)
against each other, skipped and priming launches, a captured graph that follows the decay, the
swap, and an evaluation that reads the average."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from test_grad_clip_gpu import FORMS, _assert_images, _grad, _ica, _one, _state

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 2053  # more than one workgroup of float4s (513 > 256 threads) and a one-element scalar tail
# |fl(e + omd (p - e)) - exact| per element, in units of max(|e|, |p|) = M: the difference, the
# product and the sum each round once, each by at most 2^-24 of a magnitude of at most 2 M (a
# contracted product-sum rounds once less), so 3 * 2^-23 M <= 2^-21 M
BOUND = 2.0 ** -21


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    for k in ("DINUNET_EMA_DECAY", "DINUNET_LR_SCHEDULE", "DINUNET_MAX_GRAD_NORM"):
        monkeypatch.delenv(k, raising=False)


def _f32(x):
    return float(np.float32(x))


def _within(e_t, e_prev, p_t, t, decay=0.9, warmup=True):
    """max over elements of |e_t - ref| / (BOUND * max(|e_prev|, |p_t|)) (<= 1 passes)."""
    from dinunet_implementations_amd.ops.reference import ema_update
    ref = ema_update(e_prev, p_t, t, decay, warmup)
    lim = BOUND * torch.maximum(e_prev.double().abs(), p_t.double().abs())
    err = (e_t.double() - ref).abs()
    assert bool((err <= lim).all()), float((err - lim).max())
    return err, lim


# ---- 1. the per-step rule against fp64 -----------------------------------------------------------
@pytest.mark.parametrize("form", ["step", "graphable"])
def test_rule_matches_the_fp64_mirror_tail_included(form):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    flat = FlatParams([nn.Parameter(torch.randn(N + 3, device=DEV))])
    opt = FusedAdam(flat, lr=1e-1, ema_decay=0.9, ema_warmup=True)
    # an odd-length view reaches adam_kernel's scalar tail (test_scalar_tail_uses_the_rate)
    flat.data, flat.grad = flat.data[:N], flat.grad[:N]
    opt.exp_avg, opt.exp_avg_sq, opt.ema = opt.exp_avg[:N], opt.exp_avg_sq[:N], opt.ema[:N]
    assert torch.equal(opt.ema, flat.data)  # e_0 = p_0
    ramp = cap = 0
    # six updates from a fresh optimizer, where (1 + t) / (10 + t) is still far below 0.9; the
    # ramp meets the cap at t = 80 (81 / 90), so four more updates run there, the update number
    # moved on by hand (both forms take it from step_count)
    for t in list(range(1, 7)) + [79, 80, 81, 82]:
        opt.step_count = t - 1
        e_prev = opt.ema.clone()
        _one(form, flat, opt, _grad(N, t, scale=1.0))
        torch.cuda.synchronize()
        p_t, e_t = flat.data.clone(), opt.ema.clone()
        err, lim = _within(e_t, e_prev, p_t, t)
        assert float(err[N - 1]) <= float(lim[N - 1]) and float(lim[N - 1]) > 0  # the tail
        assert not torch.equal(e_t, e_prev) and not torch.equal(e_t, p_t)
        assert float(e_t[N - 1]) != float(e_prev[N - 1])
        d = opt.ema_decay_at(t)
        print(form, t, "d_t", d, "max err / bound", float((err / lim.clamp_min(1e-300)).max()))
        assert float(opt.applied_ema_decay) == _f32(d)
        ramp += d < _f32(0.9)
        cap += d == _f32(0.9)
    assert ramp == 7 and cap == 3  # the decay crossed from the warmup ramp to the cap
    assert opt.step_count == 82


# ---- the three step forms on the small ICA model ------------------------------------------------
def _packed_opt(ema, clip=None, seed=0):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    m = _ica(seed)
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3, weight_decay=1e-4, max_grad_norm=clip, ema_decay=ema)
    pp = m.persistent_pack(flat.data.device)
    opt.attach_pack(pp)
    return m, flat, opt, pp


def _images(pp):
    return [t.clone() for t in [pp.wih_p, pp.bias_p, pp.whh_p, pp.whhT_p] + pp.casts + pp.extra]


# ---- 2. the update is untouched ------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_the_update_is_bit_identical_with_the_average_on(form):
    runs = []
    for ema in (0.9, 0):
        m, flat, opt, pp = _packed_opt(ema)
        assert (opt.ema is not None) == bool(ema)
        for s in range(3):
            _one(form, flat, opt, _grad(flat.grad.numel(), s))
        torch.cuda.synchronize()
        if form == "pack":
            assert float(flat.grad.abs().max()) == 0.0
            _assert_images(pp, m, flat)
        runs.append(_state(flat, opt) + [flat.grad.clone()] + _images(pp))
    assert runs[0][0].abs().max() > 0
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- 3. the forms agree bitwise on the average ---------------------------------------------------
def test_three_forms_agree_bitwise_on_the_average():
    res = {}
    for form in FORMS:
        m, flat, opt, pp = _packed_opt(0.9)
        n = flat.grad.numel()
        for s in range(2):  # a state with history, by the plain form in all three
            _one("step", flat, opt, _grad(n, s))
        e0 = opt.ema.clone()
        _one(form, flat, opt, _grad(n, 9))
        torch.cuda.synchronize()
        assert opt.step_count == 3 and not torch.equal(opt.ema, e0)
        assert float(opt.applied_ema_decay) == _f32(opt.ema_decay_at(3))
        _within(opt.ema, e0, flat.data, 3)
        res[form] = _state(flat, opt) + [opt.ema.clone(), opt.applied_ema_decay.clone()]
    for form in FORMS[1:]:
        for a, b in zip(res["step"], res[form]):
            assert torch.equal(a, b), form


def _device_fed(monkeypatch, armed, ema=0.9):
    """test_adam_slab_gpu's run (warm-up + 3 replays of a 2-step graph, 3 split-K slabs) with the
    average on: the optimizer, the flat buffer and whether the step armed the slab sources."""
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.ops import gemm as gemm_mod
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime import step as step_mod
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    from test_adam_slab_gpu import K, REPLAYS, WARM, _data
    monkeypatch.setattr(step_mod, "ADAM_PACK", True)
    monkeypatch.setattr(step_mod, "ADAM_SLABS", armed)
    monkeypatch.setattr(gemm_mod, "_GROUP_SPLITS", 3)
    m = _ica(0)
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3, ema_decay=ema)
    eng = make_engine("dSGD", m, flat, SiteGroup(device=torch.device("cuda")),
                      {"precision_bits": "32"})
    step = step_mod.TrainStep(m, flat, opt, eng, task="ica", use_graph=True)
    X, Y, nb = _data(8, 24)
    feed = DeviceFeed(step, X, Y, 8, nb, col=1, steps_per_graph=K)
    assert step._apack is not None
    feed.run(WARM)
    feed.run(K * REPLAYS)
    torch.cuda.synchronize()
    assert opt.step_count == WARM + K * REPLAYS
    return flat, opt, step._slabs_ok()


def test_slab_fed_pack_form_agrees_bitwise_on_the_average(monkeypatch):
    f1, o1, a1 = _device_fed(monkeypatch, True)
    f0, o0, a0 = _device_fed(monkeypatch, False)
    assert a1 and not a0
    assert torch.equal(o1.ema, o0.ema) and torch.equal(f1.data, f0.data)
    assert not torch.equal(o1.ema, f1.data)
    assert float(o1.applied_ema_decay) == _f32(o1.ema_decay_at(o1.step_count))
    # and the device-fed update itself is the one of a run without the average
    f2, o2, a2 = _device_fed(monkeypatch, True, ema=0)
    assert a2 and o2.ema is None and torch.equal(f2.data, f1.data)


# ---- 4. a skipped update -------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_skipped_update_leaves_the_average_and_takes_its_number(form):
    m, flat, opt, pp = _packed_opt(0.9, clip=0.5)
    n = flat.grad.numel()
    _one("step", flat, opt, _grad(n, 0))
    torch.cuda.synchronize()
    before = opt.ema.clone()
    assert not torch.equal(before, flat.data)
    g = _grad(n, 1)
    g[n // 2] = float("inf")
    _one(form, flat, opt, g)
    torch.cuda.synchronize()
    assert int(opt.skipped_steps) == 1 and opt.step_count == 2
    assert torch.equal(opt.ema, before)
    assert float(opt.applied_ema_decay) == _f32(opt.ema_decay_at(1))  # no average was taken
    _one(form, flat, opt, _grad(n, 2))
    torch.cuda.synchronize()
    assert int(opt.skipped_steps) == 1 and opt.step_count == 3
    assert opt.ema_decay_at(3) > opt.ema_decay_at(2)
    assert float(opt.applied_ema_decay) == _f32(opt.ema_decay_at(3))
    _within(opt.ema, before, flat.data, 3)
    assert not torch.equal(opt.ema, before)


# ---- 5. priming ----------------------------------------------------------------------------------
def test_priming_launch_leaves_the_average():
    m, flat, opt, pp = _packed_opt(0.9)
    n = flat.grad.numel()
    _one("step", flat, opt, _grad(n, 0))
    torch.cuda.synchronize()
    before, p0, applied = opt.ema.clone(), flat.data.clone(), float(opt.applied_ema_decay)
    flat.grad.copy_(_grad(n, 1))
    opt.sync_device_step()
    opt.step_pack(update=False)
    torch.cuda.synchronize()
    assert torch.equal(opt.ema, before) and torch.equal(flat.data, p0)
    assert float(opt.applied_ema_decay) == applied
    assert float(flat.grad.abs().max()) == 0.0
    _assert_images(pp, m, flat)


# ---- 6. a captured graph -------------------------------------------------------------------------
def _vector(ema=0.9):
    """(No warmup: at these update numbers the ramp lies below both decays the test sets.)"""
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    torch.manual_seed(3)
    flat = FlatParams([nn.Parameter(torch.randn(N, device=DEV))])
    return flat, FusedAdam(flat, lr=1e-2, ema_decay=ema, ema_warmup=False)


def test_captured_graph_follows_the_decay_without_recapture():
    fe, oe = _vector()
    fg, og = _vector()
    n = fe.grad.numel()
    for f, o in ((fe, oe), (fg, og)):  # (library loaded and the kernel resident before capture)
        _one("graphable", f, o, _grad(n, 100))
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        og.step_graphable()
    assert torch.equal(og.ema, oe.ema)  # captured, not run
    for i in range(5):
        if i == 3:
            for o in (oe, og):
                o.ema_decay = 0.5
        g = _grad(n, i)
        _one("graphable", fe, oe, g)
        fg.grad.copy_(g)
        gr.replay()
        og.step_count += 1
        torch.cuda.synchronize()
        assert torch.equal(og.ema, oe.ema) and torch.equal(fg.data, fe.data), i
        want = og.ema_decay_at(og.step_count)
        assert float(og.applied_ema_decay) == _f32(want), i
        assert want == (0.5 if i >= 3 else _f32(0.9))
    # the new decay shows in the values: the eager twin that kept 0.9 ends elsewhere
    fk, ok = _vector()
    _one("graphable", fk, ok, _grad(n, 100))
    for i in range(5):
        _one("graphable", fk, ok, _grad(n, i))
    torch.cuda.synchronize()
    assert torch.equal(fk.data, fe.data) and not torch.equal(ok.ema, oe.ema)


def test_setter_and_swap_refuse_a_capture(monkeypatch):
    flat, opt = _vector()
    e0 = opt.ema.clone()
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        opt.ema_decay = 0.5
    with pytest.raises(RuntimeError, match="capture"):
        opt.swap_ema()
    monkeypatch.undo()
    assert opt.ema_decay == 0.9 and torch.equal(opt.ema, e0) and not opt._swapped
    words = opt._emas.cpu()
    assert float(words.view(torch.float32)[0]) == _f32(0.9) and int(words[1]) == 0


# ---- 7. the swap ---------------------------------------------------------------------------------
def test_swap_kernel_exchanges_and_twice_restores():
    from dinunet_implementations_amd.ops import _lib
    g = torch.Generator(device=DEV).manual_seed(11)
    A = torch.randn(N + 3, device=DEV, generator=g)
    B = torch.randn(N + 3, device=DEV, generator=g)
    A[5], B[N - 1] = float("nan"), -0.0
    a0, b0 = A.clone(), B.clone()
    bits = lambda t: t.view(torch.int32)
    _lib.call("dn_swap_f32", A.data_ptr(), B.data_ptr(), N, _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(A[:N]), bits(b0[:N])) and torch.equal(bits(B[:N]), bits(a0[:N]))
    assert torch.equal(A[N:], a0[N:]) and torch.equal(B[N:], b0[N:])  # nothing past n
    _lib.call("dn_swap_f32", A.data_ptr(), B.data_ptr(), N, _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(bits(A), bits(a0)) and torch.equal(bits(B), bits(b0))
    with pytest.raises(RuntimeError):  # misaligned
        _lib.call("dn_swap_f32", A.data_ptr() + 4, B.data_ptr(), 8, _lib.stream())
    with pytest.raises(RuntimeError):  # overlapping
        _lib.call("dn_swap_f32", A.data_ptr(), A.data_ptr() + 16, 8, _lib.stream())


def test_scope_swaps_in_and_back_and_refuses_updates():
    m, flat, opt, pp = _packed_opt(0.9)
    n = flat.grad.numel()
    for s in range(2):
        _one("pack", flat, opt, _grad(n, s))
    torch.cuda.synchronize()
    p0, e0, im0 = flat.data.clone(), opt.ema.clone(), _images(pp)
    assert not torch.equal(p0, e0)
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            assert torch.equal(flat.data, e0) and torch.equal(opt.ema, p0)
            for call in (opt.step, opt.step_graphable, opt.step_pack):
                with pytest.raises(RuntimeError, match="swapped"):
                    call()
            1 / 0  # the scope swaps back however it ends
    torch.cuda.synchronize()
    assert torch.equal(flat.data, p0) and torch.equal(opt.ema, e0)
    for a, b in zip(_images(pp), im0):
        assert torch.equal(a, b)
    _assert_images(pp, m, flat)
    _one("pack", flat, opt, _grad(n, 2))  # and updates go on
    assert opt.step_count == 3


# ---- 8. evaluation reads the average -------------------------------------------------------------
def _trainer(seed, ema):
    """The ICA task's trainer around ``_ica(seed)``."""
    from dinunet_implementations_amd.config import build_config
    from dinunet_implementations_amd.tasks.ica import ICATrainer

    class T(ICATrainer):
        def _init_nn_model(self):
            self.nn["net"] = _ica(seed)

    cfg = build_config(overrides=dict(task_id="ICA-Classification", num_components=20,
                                      window_size=10, window_stride=10, temporal_size=120,
                                      input_size=64, hidden_size=128, batch_size=8,
                                      ema_decay=ema))
    tr = T(cache=cfg, state={}, device=torch.device("cuda", 0))
    tr.init_nn()
    return tr


def _result(res):
    return res["out"].clone(), res["averages"].average, res["metrics"].scores()


@pytest.mark.parametrize("device_fed", [False, True])
def test_evaluation_inside_the_scope_reads_the_average(device_fed):
    from dinunet_implementations_amd.data.loader import DeviceLoader
    from dinunet_implementations_amd.runtime.evalfeed import EvalFeed
    g = torch.Generator().manual_seed(1)
    X = torch.randn(13, 12, 20, 10, generator=g).cuda()  # one full batch of 8 and a tail of 5
    Y = torch.randint(0, 2, (13,), generator=g).cuda()
    tr, other = _trainer(0, 0.9), _trainer(1, 0)
    assert tr.optimizer.ema is not None and other.optimizer.ema is None
    assert not torch.equal(tr.flat.data, other.flat.data)
    tr.optimizer.ema.copy_(other.flat.data)

    def run(t):
        if device_fed:
            feed = feeds.setdefault(id(t), EvalFeed(t, X, Y, 8))
            return _result(feed.run())
        return _result(t.evaluate(DeviceLoader(X, Y, 8)))

    feeds = {}
    raw = run(tr)
    want = run(other)
    assert not torch.equal(raw[0], want[0])
    p0 = tr.flat.data.clone()
    with tr.ema_weights():
        got = run(tr)
    assert torch.equal(got[0], want[0]) and got[1:] == want[1:]
    torch.cuda.synchronize()
    assert torch.equal(tr.flat.data, p0) and torch.equal(tr.optimizer.ema, other.flat.data)
    again = run(tr)
    assert torch.equal(again[0], raw[0]) and again[1:] == raw[1:]
