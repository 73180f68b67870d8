"""Global-norm gradient clipping of the fused Adam on the GPU (optim.hip grad_sqnorm_kernel and
the clipped forms of adam_kernel / adam_pack_kernel): the norm kernel against an fp64 reference,
the three step forms against each other and the CPU path, the skip guard, and a device-fed
K-step graph whose threshold changes between replays."""
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

DEV = "cuda"
ATOL, RTOL = 1e-5, 1e-4  # test_fused_adam_matches_torch's
SCALES = (1.0, 0.02, 3.0, 0.02, 1.0, 0.02)


def _ulp_apart(a: float, b: float) -> bool:
    """fp32 values equal or adjacent."""
    ta, tb = torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)
    return bool(ta == tb) or bool(torch.nextafter(ta, tb) == tb)


def _vector_opt(n, c=1e30):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    flat = FlatParams([nn.Parameter(torch.zeros(n, device=DEV))])
    return flat, FusedAdam(flat, lr=1e-3, max_grad_norm=c)


def _norm_of(g):
    """(G fp32, the fp64 partials, skipped) the clipped step records for gradient ``g``."""
    from dinunet_implementations_amd.ops.optim import CLIP_PARTS
    flat, opt = _vector_opt(g.numel())
    flat.grad.copy_(g)
    opt.step()
    torch.cuda.synchronize()
    return float(opt.grad_norm), opt._clip[:CLIP_PARTS].clone(), int(opt.skipped_steps)


def _lengths():
    from dinunet_implementations_amd.ops.optim import CLIP_PARTS
    return (4, 4 * 256 * CLIP_PARTS + 4, 1063108)  # one float4 past a grid pass; the ICA model


@pytest.mark.parametrize("which", [0, 1, 2])
def test_norm_kernel_matches_fp64_reference(which):
    n = _lengths()[which]
    g = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n))
    want = float(torch.linalg.vector_norm(g.double()).float())
    got, parts, skipped = _norm_of(g)
    print(n, "norm", got, "reference", want)
    assert _ulp_apart(got, want) and skipped == 0
    # fp64 accumulation: only the final rounding to fp32 can differ
    s = float(g.double().square().sum())
    assert abs(float(parts.sum()) - s) <= 1e-12 * s
    again, parts2, _ = _norm_of(g)
    assert again == got and torch.equal(parts, parts2)  # fixed order: the same bits


def test_norm_kernel_range_and_non_finite():
    n = _lengths()[1]
    g = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    g[n - 3] = 1e30  # its square overflows fp32, not fp64
    got, _, skipped = _norm_of(g)
    assert math.isfinite(got) and skipped == 0
    assert _ulp_apart(got, float(torch.linalg.vector_norm(g.double()).float()))
    g[7] = float("inf")
    got, _, skipped = _norm_of(g)
    assert math.isinf(got) and skipped == 1
    g[7] = float("nan")
    got, _, skipped = _norm_of(g)
    assert math.isnan(got) and skipped == 1


def test_gpu_step_matches_cpu_path():
    """The CPU test's 6-step case: the same gradients (computed once, on the CPU model) go through
    ``step()`` of a GPU optimizer and of a CPU one, so the two norms are of the same vector."""
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    torch.manual_seed(1)
    mods = nn.Sequential(nn.Linear(33, 17), nn.Linear(17, 5))
    twin = nn.Sequential(nn.Linear(33, 17), nn.Linear(17, 5))
    twin.load_state_dict(mods.state_dict())
    twin = twin.to(DEV)
    fc, fg = FlatParams(mods.parameters()), FlatParams(twin.parameters())
    oc = FusedAdam(fc, lr=1e-2, weight_decay=1e-4, max_grad_norm=10)
    og = FusedAdam(fg, lr=1e-2, weight_decay=1e-4, max_grad_norm=10)
    clipped = 0
    for s in SCALES:
        x = torch.randn(8, 33) * s
        oc.zero_grad()
        mods(x).square().sum().backward()
        fg.grad.copy_(fc.grad)
        oc.step()
        og.step()
        a, b = float(og.grad_norm), float(oc.grad_norm)
        print("norm gpu", a, "cpu", b)
        assert _ulp_apart(a, b)
        clipped += b > 10
    assert clipped == 3
    assert torch.allclose(fg.data.cpu(), fc.data, atol=ATOL, rtol=RTOL)
    assert torch.allclose(og.exp_avg.cpu(), oc.exp_avg, atol=ATOL, rtol=RTOL)


# ---- the three step forms on the small ICA model ------------------------------------------------
def _ica(seed=0, hidden=128):
    from dinunet_implementations_amd.models import ICALstm
    torch.manual_seed(seed)
    m = ICALstm(input_size=64, hidden_size=hidden, num_comps=20, window_size=10).cuda().train()
    m.classifier[0].p = 0.0
    return m


def _packed_opt(clip, seed=0, ema=None):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    m = _ica(seed)
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3, weight_decay=1e-4, max_grad_norm=clip, ema_decay=ema)
    pp = m.persistent_pack(flat.data.device)
    opt.attach_pack(pp)
    return m, flat, opt, pp


def _grad(n, seed, scale=1e-2):
    return torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * scale


def _one(form, flat, opt, g):
    """One update of ``form`` from gradient ``g`` (host and device step numbers kept in step)."""
    flat.grad.copy_(g)
    if form == "step":
        opt.step()
        return
    opt.sync_device_step()
    if form == "graphable":
        opt.step_graphable()
    else:
        opt.device_step().add_(1)  # what the step's encoder GEMM does (dn_gemm_arm_bump)
        opt.step_pack()
    opt.step_count += 1


def _state(flat, opt):
    return [t.clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)]


def _fresh_images(m, flat):
    from dinunet_implementations_amd.ops.lstm import pack_params
    lin = m.encoder[0]
    casts = []
    params = [t for cell in m.lstm.lstms for t in cell.params()]
    wih, bias, whh, whhT, _ = pack_params(params, m.lstm.input_size, flat.data.device,
                                          casts=(lin.weight, lin.bias), cast_out=casts)
    torch.cuda.synchronize()
    return wih, bias, whh, whhT, casts


def _assert_images(pp, m, flat):
    wih, bias, whh, whhT, casts = _fresh_images(m, flat)
    assert torch.equal(pp.wih_p, wih) and torch.equal(pp.whh_p, whh)
    assert torch.equal(pp.whhT_p, whhT)
    n = bias.numel()
    assert torch.equal(pp.bias_p[:n] + pp.bias_p[n:], bias)
    for a, b in zip(pp.casts, casts):
        assert torch.equal(a, b)


FORMS = ("step", "graphable", "pack")


def test_three_forms_agree_bitwise_when_clipping():
    c = 0.5
    res = {}
    for form in FORMS:
        m, flat, opt, pp = _packed_opt(c)
        n = flat.grad.numel()
        for s in range(2):  # a state with history, by the plain form in all three
            _one("step", flat, opt, _grad(n, s))
        p0 = flat.data.clone()
        _one(form, flat, opt, _grad(n, 9))
        torch.cuda.synchronize()
        G = float(opt.grad_norm)
        assert G > c and int(opt.skipped_steps) == 0 and opt.step_count == 3
        assert not torch.equal(flat.data, p0)
        res[form] = _state(flat, opt) + [G]
        if form == "pack":
            assert float(flat.grad.abs().max()) == 0.0
            _assert_images(pp, m, flat)  # the images of the clipped parameters
    for form in FORMS[1:]:
        for a, b in zip(res["step"][:3], res[form][:3]):
            assert torch.equal(a, b), form
        assert res[form][3] == res["step"][3]
    # the clip took effect: the same three steps without it end elsewhere
    m, flat, opt, _ = _packed_opt(None)
    for s in (0, 1, 9):
        _one("step", flat, opt, _grad(flat.grad.numel(), s))
    assert (flat.data - res["step"][0]).abs().max() > 1e-5


@pytest.mark.parametrize("form", FORMS)
def test_non_finite_gradient_skips_on_the_gpu(form):
    m, flat, opt, pp = _packed_opt(0.5)
    n = flat.grad.numel()
    _one("step", flat, opt, _grad(n, 0))
    before = _state(flat, opt)
    g = _grad(n, 1)
    g[n // 2] = float("inf")
    _one(form, flat, opt, g)
    torch.cuda.synchronize()
    for a, b in zip(_state(flat, opt), before):
        assert torch.equal(a, b)
    assert int(opt.skipped_steps) == 1 and opt.step_count == 2
    assert math.isinf(float(opt.grad_norm))
    if form == "pack":
        assert float(flat.grad.abs().max()) == 0.0  # still zeroed, images still rewritten
        _assert_images(pp, m, flat)
    _one(form, flat, opt, _grad(n, 2))  # the next finite step updates
    torch.cuda.synchronize()
    assert int(opt.skipped_steps) == 1 and opt.step_count == 3
    assert not torch.equal(flat.data, before[0]) and torch.isfinite(flat.data).all()


@pytest.mark.parametrize("form", FORMS)
def test_off_is_bit_equal_to_a_threshold_never_reached(form):
    runs = []
    for c in (None, 1e30):
        m, flat, opt, pp = _packed_opt(c)
        for s in range(5):
            _one(form, flat, opt, _grad(flat.grad.numel(), s))
        torch.cuda.synchronize()
        runs.append(_state(flat, opt) + [pp.wih_p.clone()])
    assert runs[0][0].abs().max() > 0
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- captured device-fed steps -------------------------------------------------------------------
def _trainer(clip, **kw):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.step import TrainStep
    m = _ica(0)
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3, max_grad_norm=clip)
    eng = make_engine("dSGD", m, flat, SiteGroup(device=torch.device("cuda")),
                      {"precision_bits": "32"})
    return m, flat, TrainStep(m, flat, opt, eng, task="ica", **kw)


C1, C2 = 0.05, 0.005  # thresholds below the small model's gradient norm (printed by the test)


def test_device_fed_graph_clips_and_follows_the_threshold(monkeypatch):
    """K = 4 whole steps per HIP graph, Adam-emitted pack, clipping on, against the host-fed
    eager loop on the same batches (test_device_fed_multistep_graph_matches_host_fed's
    tolerance); then the threshold is lowered between two replays of the SAME graph."""
    from dinunet_implementations_amd.ops import DeviceSource
    from dinunet_implementations_amd.runtime import step as step_mod
    monkeypatch.setattr(step_mod, "ADAM_PACK", True)
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = torch.randn(8, 8, 12, 20, 10, device="cuda", generator=gen)
    ys = torch.randint(0, 2, (8, 8), device="cuda", generator=gen)
    B = xs.shape[1]
    X = xs.reshape(-1, *xs.shape[2:]).to(torch.bfloat16)
    Y = ys.reshape(-1)
    _, fh, sh = _trainer(C1, use_graph=False)
    _, fd, sd = _trainer(C1, use_graph=True)
    src = DeviceSource(X, Y, B)
    sd.bind(src, steps_per_graph=4)
    assert sd._apack is not None

    def host(lo, hi):
        norms = []
        for c in range(lo, hi):
            xb, yb = src.batch(c)
            sh(xb.float(), yb)
            norms.append(float(sh.opt.grad_norm))
        return norms

    def close():
        torch.cuda.synchronize()
        d = (fh.data - fd.data).abs().max()
        print("max |host - device-fed|", float(d))
        return torch.allclose(fh.data, fd.data, rtol=1e-6, atol=1e-7)

    norms = host(0, 7)
    sd.run(3)
    sd.prepare(8)
    graph = sd._dgraphs[4][0]
    sd.run(4)
    print("host norms", norms, "device-fed last", float(sd.opt.grad_norm))
    assert min(norms) > C1  # every step clipped
    assert close()
    # a lower threshold, the same captured graph
    sh.opt.max_grad_norm = C2
    sd.opt.max_grad_norm = C2
    norms = host(7, 11)
    sd.run(4)
    assert sd._dgraphs[4][0] is graph
    assert float(sd.opt.grad_norm) > C2 and min(norms) > C2
    assert close()
    assert sd.opt.step_count == sh.opt.step_count == 11
    assert int(sd.opt.skipped_steps) == 0
    # the lower threshold mattered: the host loop at the first threshold ends elsewhere
    _, fk, sk = _trainer(C1, use_graph=False)
    for c in range(11):
        xb, yb = src.batch(c)
        sk(xb.float(), yb)
    torch.cuda.synchronize()
    assert not torch.allclose(fk.data, fh.data, rtol=1e-6, atol=1e-7)


def _data(n=8):
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = torch.randn(n, 8, 12, 20, 10, device="cuda", generator=gen)
    ys = torch.randint(0, 2, (n, 8), device="cuda", generator=gen)
    return xs, ys, xs.reshape(-1, *xs.shape[2:]).to(torch.bfloat16), ys.reshape(-1)


def test_host_fed_captured_step_clips():
    """The one-site captured step (Adam inside the graph) against the eager loop, at
    test_graph_replay_matches_eager's tolerance."""
    xs, ys, _, _ = _data(6)
    _, fe, se = _trainer(C1, use_graph=False)
    _, fg, sg = _trainer(C1, use_graph=True)
    for i in range(xs.shape[0]):
        se(xs[i], ys[i])
        sg(xs[i], ys[i])
        assert float(sg.opt.grad_norm) > C1
    torch.cuda.synchronize()
    assert sg.graph is not None and sg.graph_opt
    assert torch.allclose(fe.data, fg.data, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("accum", [1, 2])
def test_device_fed_forms_without_the_pack_clip(accum, monkeypatch):
    """The device-fed bodies whose update is the plain captured Adam (no Adam-emitted pack; with
    accumulation: two micro-batches per update) against the host-fed steps on the same batches,
    at test_device_feed_accumulation_matches_host_loop's dSGD tolerance."""
    from dinunet_implementations_amd.runtime import step as step_mod
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    monkeypatch.setattr(step_mod, "ADAM_PACK", False)
    _, _, X, Y = _data(6)
    B, nb = 8, 5
    _, fh, sh = _trainer(C1, use_graph=True, accum=accum)
    _, fd, sd = _trainer(C1, use_graph=True, accum=accum)
    feed = DeviceFeed(sd, X, Y, B, nb, col=1, steps_per_graph=4)
    g = torch.Generator(device="cuda").manual_seed(5)
    nbb = nb * accum
    for _ in range(2):
        order = torch.randint(0, X.shape[0], (nbb * B,), device="cuda", generator=g)
        for c in range(nbb):
            rows = order[c * B:(c + 1) * B]
            sh(X[rows].float(), Y[rows], first=c % accum == 0, last=c % accum == accum - 1)
        feed.run_epoch(order)
        torch.cuda.synchronize()
    assert sd._apack is None and sd._dK == 4
    assert all(v[2] for v in sd._dgraphs.values()), "the update must be inside the replays"
    assert sd.opt.step_count == sh.opt.step_count == 2 * nb
    assert float(sd.opt.grad_norm) > C1 and int(sd.opt.skipped_steps) == 0
    assert torch.allclose(fh.data, fd.data, rtol=1e-6, atol=1e-7), (fh.data - fd.data).abs().max()


def test_threshold_setter_refuses_a_capture(monkeypatch):
    _, opt = _vector_opt(8, c=1.0)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        opt.max_grad_norm = 2.0
    monkeypatch.undo()
    assert opt.max_grad_norm == 1.0 and float(opt._clip_f[0]) == 1.0


# ---- the launchers' argument block ---------------------------------------------------------------
def test_argument_block_layout_and_refusals():
    """The host mirror of optim.hip AdamArgs has the library's size, and every refusal Python can
    reach is a DN_BAD_SHAPE status before any launch (the buffers stay as they were)."""
    import ctypes
    from dinunet_implementations_amd.ops import _lib
    from dinunet_implementations_amd.ops.optim import _AdamArgs, _Src
    L = _lib.lib()
    L.dn_adam_args_size.restype = ctypes.c_long
    assert int(L.dn_adam_args_size()) == ctypes.sizeof(_AdamArgs)
    m, flat, opt, pp = _packed_opt(0.5, ema=0.9)
    opt.sync_device_step()
    opt.device_step().add_(1)
    flat.grad.copy_(_grad(flat.grad.numel(), 0))
    before = _state(flat, opt) + [opt.ema.clone(), flat.grad.clone(), pp.wih_p.clone()]
    pack, tab, cnt = opt._pack[:3]
    BAD, st = 1, _lib.stream()

    def block(**fields):
        a = opt._adam_args(1.0, opt._clip.data_ptr(), 0)
        for k, v in fields.items():
            setattr(a, k, v)
        return a

    def adam(a, bump=0):
        return L.dn_adam(ctypes.addressof(a), bump, st)

    def adam_pack(a, update, srcs=None):
        return L.dn_adam_pack(ctypes.addressof(a), update, 1, ctypes.addressof(tab), cnt, pack.I,
                              pack.Hd, pack.HD, None, 0, 0, None, None, 1, None, 0, None, None,
                              None, 1, None, ctypes.addressof(srcs) if srcs else None, st)

    n = flat.data.numel()
    off = dict(p=flat.data.data_ptr() + 4, n=n - 4)  # (misaligned, and still inside the buffer)
    assert adam(block(**off)) == BAD and adam_pack(block(**off), 1) == BAD
    assert adam(block(es=None)) == BAD and adam_pack(block(es=None), 1) == BAD  # ema without state
    assert adam(block(ema=None)) == BAD  # and the state without the average
    assert adam(block(tdev=None), bump=1) == BAD  # nothing to advance
    assert adam_pack(block(), 0) == BAD  # clip with update = 0
    assert adam_pack(block(), 1, srcs=(_Src * cnt)()) == BAD  # slab sources with clip
    assert adam_pack(block(cs=None), 0, srcs=(_Src * cnt)()) == BAD  # ... or without an update
    torch.cuda.synchronize()
    after = _state(flat, opt) + [opt.ema, flat.grad, pp.wih_p]
    for a, b in zip(after, before):
        assert torch.equal(a, b)
    assert int(opt.skipped_steps) == 0
