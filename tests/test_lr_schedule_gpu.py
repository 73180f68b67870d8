"""Learning-rate schedule of the fused Adam on the GPU (optim.hip sched_lr in the SCHED forms of
adam_kernel / adam_pack_kernel): the device rate against the host formula, the three step forms
against each other, constant against off, clipping and schedule together, and captured graphs
that follow the schedule, ``lr_scale`` and ``lr`` without recapture."""

import pytest
import torch
import torch.nn as nn

from test_grad_clip_gpu import (FORMS, _assert_images, _data, _grad, _ica, _one, _state,
                                _ulp_apart)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KINDS = ("constant", "linear", "cosine")


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("DINUNET_LR_SCHEDULE", raising=False)
    monkeypatch.delenv("DINUNET_MAX_GRAD_NORM", raising=False)


def _sched(kind, W=3, T=10, lr_min=0.0):
    return {"kind": kind, "warmup_steps": W, "decay_steps": T, "lr_min": lr_min}


# ---- the device rate against the host formula -------------------------------------------------------
N = 2053  # more than one workgroup of float4s (513 > 256 threads) and a one-element scalar tail
# betas fp32 holds exactly: with a gradient of ones and zero state the first update's m / bc1 and
# sqrt(v / bc2) are exactly 1 in the kernel's fp32 arithmetic, so the parameter shows the rate
# alone (with 0.9 / 0.999, 1 - b2 in fp32 is already 3e-5 away from the double bias correction)
BETAS = (0.5, 0.75)


@pytest.mark.parametrize("form", ["step", "graphable"])
@pytest.mark.parametrize("kind", KINDS)
def test_device_rate_matches_the_host_formula(kind, form):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    flat = FlatParams([nn.Parameter(torch.zeros(N, device=DEV))])
    assert flat.data.numel() == N + 3  # (padded to whole float4s: the last real element is 2052)
    opt = FusedAdam(flat, lr=1e-3, betas=BETAS, lr_schedule=_sched(kind, lr_min=1e-4))
    ones = torch.ones_like(flat.grad)
    for t in range(1, 14):
        _one(form, flat, opt, ones)
        got, want = float(opt.applied_lr), opt.lr_at(t)
        print(kind, form, t, got, want)
        assert _ulp_apart(got, want), (t, got, want)
        if kind == "constant" or t <= 3:
            assert got == want, (t, got, want)
        if t == 1:
            # m / bc1 = 1 and sqrt(v / bc2) = 1: p = -lr / (1 + eps) in every element, the
            # second workgroup's and the last float4 included
            p = flat.data[:N]
            assert float(p.min()) == float(p.max())
            assert _ulp_apart(float(p[0]), -got * (1.0 / (1.0 + 1e-8)))
    assert opt.step_count == 13


def test_scalar_tail_uses_the_rate():
    """A buffer whose length is no multiple of four reaches adam_kernel's scalar tail: the flat
    buffer pads every tensor, so the optimizer is pointed at an odd-length view."""
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    flat = FlatParams([nn.Parameter(torch.zeros(N + 3, device=DEV))])
    opt = FusedAdam(flat, lr=1e-3, betas=BETAS, lr_schedule=_sched("cosine"))
    flat.data, flat.grad = flat.data[:N], flat.grad[:N]
    opt.exp_avg, opt.exp_avg_sq = opt.exp_avg[:N], opt.exp_avg_sq[:N]
    flat.grad.fill_(1.0)
    opt.step()
    got = float(opt.applied_lr)
    assert got == opt.lr_at(1)
    assert float(flat.data.min()) == float(flat.data.max()) == float(flat.data[N - 1])
    assert _ulp_apart(float(flat.data[N - 1]), -got * (1.0 / (1.0 + 1e-8)))


# ---- the three step forms on the small ICA model ---------------------------------------------------
def _packed_opt(schedule, clip=None, seed=0):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    m = _ica(seed)
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3, weight_decay=1e-4, max_grad_norm=clip, lr_schedule=schedule)
    pp = m.persistent_pack(flat.data.device)
    opt.attach_pack(pp)
    return m, flat, opt, pp


def test_three_forms_agree_bitwise_under_a_schedule():
    res = {}
    for form in FORMS:
        m, flat, opt, pp = _packed_opt(_sched("cosine", W=2, T=6))
        n = flat.grad.numel()
        for s in range(2):  # a state with history, by the plain form in all three
            _one("step", flat, opt, _grad(n, s))
        p0 = flat.data.clone()
        _one(form, flat, opt, _grad(n, 9))
        torch.cuda.synchronize()
        assert opt.step_count == 3 and not torch.equal(flat.data, p0)
        assert _ulp_apart(float(opt.applied_lr), opt.lr_at(3)) and opt.lr_at(3) < opt.lr_at(2)
        res[form] = _state(flat, opt) + [opt.applied_lr.clone()]
        if form == "pack":
            assert float(flat.grad.abs().max()) == 0.0
            _assert_images(pp, m, flat)
    for form in FORMS[1:]:
        for a, b in zip(res["step"], res[form]):
            assert torch.equal(a, b), form
    # the schedule took effect: the same three steps without it end elsewhere
    m, flat, opt, _ = _packed_opt(None)
    for s in (0, 1, 9):
        _one("step", flat, opt, _grad(flat.grad.numel(), s))
    assert (flat.data - res["step"][0]).abs().max() > 1e-5


@pytest.mark.parametrize("form", FORMS)
def test_constant_is_bit_identical_to_off(form):
    runs = []
    for schedule in (None, "constant"):
        m, flat, opt, pp = _packed_opt(schedule)
        for s in range(3):
            _one(form, flat, opt, _grad(flat.grad.numel(), s))
        torch.cuda.synchronize()
        runs.append(_state(flat, opt) + [pp.wih_p.clone()])
    assert opt.applied_lr is not None and float(opt.applied_lr) == opt.lr_at(3)
    assert runs[0][0].abs().max() > 0
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("form", FORMS)
def test_clipping_and_schedule_together(form):
    m, flat, opt, pp = _packed_opt(_sched("linear", W=0, T=10), clip=0.5)
    n = flat.grad.numel()
    _one(form, flat, opt, _grad(n, 0))
    torch.cuda.synchronize()
    before = _state(flat, opt)
    g = _grad(n, 1)
    g[n // 2] = float("inf")
    _one(form, flat, opt, g)
    torch.cuda.synchronize()
    for a, b in zip(_state(flat, opt), before):
        assert torch.equal(a, b)
    assert int(opt.skipped_steps) == 1
    assert _ulp_apart(float(opt.applied_lr), opt.lr_at(2))  # the skipped update took its number
    _one(form, flat, opt, _grad(n, 2))
    torch.cuda.synchronize()
    assert int(opt.skipped_steps) == 1 and opt.step_count == 3
    assert _ulp_apart(float(opt.applied_lr), opt.lr_at(3)) and opt.lr_at(3) < 0.95 * opt.lr_at(2)
    assert not torch.equal(flat.data, before[0]) and torch.isfinite(flat.data).all()


# ---- captured steps ---------------------------------------------------------------------------------
def _trainer(schedule, **kw):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.step import TrainStep
    m = _ica(0)
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3, lr_schedule=schedule)
    eng = make_engine("dSGD", m, flat, SiteGroup(device=torch.device("cuda")),
                      {"precision_bits": "32"})
    return m, flat, TrainStep(m, flat, opt, eng, task="ica", **kw)


def test_device_fed_graph_follows_schedule_scale_and_rate_without_recapture(monkeypatch):
    """K = 4 whole steps per HIP graph (Adam-emitted pack), warmup 3 and cosine decay to update
    10, against the host-fed eager loop on the same batches
    (test_device_fed_graph_clips_and_follows_the_threshold's cohort, batch and tolerance);
    ``lr_scale`` and then ``lr`` change between replays of the SAME graphs."""
    from dinunet_implementations_amd.ops import DeviceSource
    from dinunet_implementations_amd.runtime import step as step_mod
    monkeypatch.setattr(step_mod, "ADAM_PACK", True)
    xs, ys, X, Y = _data(8)
    B = xs.shape[1]
    sched = _sched("cosine", lr_min=1e-4)
    _, fh, sh = _trainer(sched, use_graph=False)
    _, fd, sd = _trainer(sched, use_graph=True)
    src = DeviceSource(X, Y, B)
    sd.bind(src, steps_per_graph=4)
    assert sd._apack is not None

    def host(lo, hi):
        for c in range(lo, hi):
            xb, yb = src.batch(c)
            sh(xb.float(), yb)

    def close():
        torch.cuda.synchronize()
        print("max |host - device-fed|", float((fh.data - fd.data).abs().max()),
              "applied", float(sd.opt.applied_lr), float(sh.opt.applied_lr))
        return (torch.allclose(fh.data, fd.data, rtol=1e-6, atol=1e-7)
                and float(sd.opt.applied_lr) == float(sh.opt.applied_lr))

    host(0, 7)
    sd.run(3)
    sd.prepare(8)
    graphs = {k: v[0] for k, v in sd._dgraphs.items()}
    assert 4 in graphs
    sd.run(4)
    assert close() and _ulp_apart(float(sd.opt.applied_lr), sd.opt.lr_at(7))
    for s in (sh, sd):
        s.opt.lr_scale = 0.5
    host(7, 11)
    sd.run(4)  # passes update 10, the end of the decay
    assert close() and _ulp_apart(float(sd.opt.applied_lr), sd.opt.lr_at(11))
    assert float(sd.opt.applied_lr) == pytest.approx(0.5 * 1e-4, rel=1e-6)
    for s in (sh, sd):
        s.opt.lr = 3e-3
    host(11, 15)
    sd.run(4)
    assert close() and _ulp_apart(float(sd.opt.applied_lr), sd.opt.lr_at(15))
    # past the decay's end every base gives lr_scale * lr_min: a longer decay shows the new one
    for s in (sh, sd):
        s.opt.set_decay_steps(30)
    host(15, 19)
    sd.run(4)
    assert close() and _ulp_apart(float(sd.opt.applied_lr), sd.opt.lr_at(19))
    assert float(sd.opt.applied_lr) > 4e-4  # (2.1e-4 at the first base rate)
    assert sd.opt.step_count == sh.opt.step_count == 19
    assert all(sd._dgraphs[k][0] is g for k, g in graphs.items())  # the same graph objects
    # the schedule mattered: the host loop without one ends elsewhere
    _, fk, sk = _trainer(None, use_graph=False)
    for c in range(19):
        xb, yb = src.batch(c)
        sk(xb.float(), yb)
    torch.cuda.synchronize()
    assert not torch.allclose(fk.data, fh.data, rtol=1e-6, atol=1e-7)


def test_host_fed_captured_step_keeps_its_graph_when_the_rate_changes():
    """With the rate on the device an ``opt.lr`` change leaves ``step.graph`` alone (and the
    replays follow it: the eager loop given the same change agrees, at
    test_graph_replay_matches_eager's tolerance); with the schedule off the graph is dropped, as
    before."""
    xs, ys, _, _ = _data(8)
    sched = _sched("cosine")
    _, fe, se = _trainer(sched, use_graph=False)
    _, fg, sg = _trainer(sched, use_graph=True)
    _, fo, so = _trainer(None, use_graph=True)
    for i in range(5):
        for s in (se, sg, so):
            s(xs[i], ys[i])
    assert sg.graph is not None and sg.graph_opt and so.graph is not None and so.graph_opt
    g_on, g_off = sg.graph, so.graph
    for s in (se, sg, so):
        s.opt.lr = 5e-4
    for i in range(5, 8):
        for s in (se, sg, so):
            s(xs[i], ys[i])
    torch.cuda.synchronize()
    assert sg.graph is g_on
    assert so.graph is not g_off  # the parent's behaviour: the rate is baked into that capture
    assert _ulp_apart(float(sg.opt.applied_lr), sg.opt.lr_at(8))
    assert float(sg.opt.applied_lr) == float(se.opt.applied_lr) < 5e-4
    assert torch.allclose(fe.data, fg.data, rtol=1e-5, atol=1e-6)


def test_setters_refuse_a_capture(monkeypatch):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    flat = FlatParams([nn.Parameter(torch.zeros(8, device=DEV))])
    opt = FusedAdam(flat, lr=1e-3, lr_schedule=_sched("cosine"))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        opt.lr = 2e-3
    with pytest.raises(RuntimeError, match="capture"):
        opt.lr_scale = 0.5
    with pytest.raises(RuntimeError, match="capture"):
        opt.set_decay_steps(20)
    monkeypatch.undo()
    assert opt.lr == 1e-3 and opt.lr_scale == 1.0 and opt.lr_schedule.decay_steps == 10
    words = opt._lrs.cpu()
    assert float(words.view(torch.float32)[1]) == 1.0 and int(words[5]) == 10


# ---- the site loop ----------------------------------------------------------------------------------
def test_ica_site_logs_the_scheduled_rate_device_fed_and_host_fed(tmp_path):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from test_runtime_gpu import _ica_root, _run_site
    root = _ica_root(tmp_path)
    ov = {"epochs": 3, "batch_size": 8, "seed": 3, "lr_schedule": "cosine", "lr_warmup_steps": 2}
    dev = _run_site(root, str(tmp_path / "dev"), dict(ov, device_feed=True))[0]
    host = _run_site(root, str(tmp_path / "host"), dict(ov, device_feed=False))[0]
    assert dev.get("feed") == "device" and "feed" not in host
    steps = dev["split_sizes"]["train"] // 8
    assert steps > 2
    from dinunet_implementations_amd.config import build_config
    lr = float(build_config(overrides=ov)["learning_rate"])
    mirror = FusedAdam(FlatParams([nn.Parameter(torch.zeros(4))]), lr=lr,
                       lr_schedule={"kind": "cosine", "warmup_steps": 2, "decay_steps": 3 * steps})
    print("learning_rate", dev["learning_rate"], [mirror.lr_at(e * steps) for e in (1, 2, 3)])
    assert len(dev["learning_rate"]) == 3
    for e in (1, 2, 3):
        assert _ulp_apart(dev["learning_rate"][e - 1], mirror.lr_at(e * steps)), e
    assert dev["learning_rate"][2] < 1e-3 * lr  # the decay ends with the phase's last update
    assert dev["learning_rate"] == host["learning_rate"]
