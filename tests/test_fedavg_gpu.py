"""Federated averaging on the GPU: the two kernels of ``csrc/kernels/fedavg.hip`` against the numpy
mirror ``tests/fedavg_ref.py`` bit for bit (every tensor they write), the drift against an fp64
sum, the launchers' refusals, and the device-fed epoch in segments of ``fedavg_local_steps``
updates against the host-fed loop, on one site and on a one-rank RCCL group."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fedavg_ref as fr

pytestmark = pytest.mark.gpu

W_ODD = float(np.float32(1.3))
# the last: one float4 past what the capped grid (2048 workgroups x 256 threads x 4 elements)
# covers in one pass, plus a scalar tail -- the grid-stride loop wraps
SIZES = [1, 4, 2053, 2 * 1024 * 1024 + 5]
DN_BAD_SHAPE = 1


@pytest.fixture(scope="module")
def inputs():
    """Per size: the anchor, three rounds of parameters (numpy, made once, never changed)."""
    out = {}
    for n in SIZES:
        rng = np.random.default_rng(n)
        a = rng.standard_normal(n).astype(np.float32)
        steps = [(rng.standard_normal(n) * 0.01 * (r + 1)).astype(np.float32) for r in range(3)]
        out[n] = (a, steps)
    return out


def _state(a, beta):
    from dinunet_implementations_amd.ops import FedAvgState
    flat = SimpleNamespace(data=torch.from_numpy(a.copy()).cuda(),
                           grad=torch.zeros(a.size, device="cuda"))
    st = FedAvgState(flat, beta)
    st.begin()
    return flat, st


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("beta", [0.0, 0.9])
@pytest.mark.parametrize("w,eta", [(1.0, 1.0), (W_ODD, 0.5)])
def test_kernels_equal_the_mirror_bit_for_bit(inputs, n, beta, w, eta):
    a0, steps = inputs[n]
    flat, st = _state(a0, beta)
    a = a0.copy()
    u = np.zeros(n, dtype=np.float32) if beta > 0 else None
    for step in steps:
        flat.data.add_(torch.from_numpy(step).cuda())
        p = _np(flat.data)
        d, drift = fr.delta(p, a, w)
        st.delta(w)
        assert fr.same_bits(_np(flat.grad), d)
        assert fr.same_bits(_np(flat.data), p) and fr.same_bits(_np(st.anchor), a)  # read only
        a, p2, u, g0 = fr.adopt(d, a, u, eta, beta)  # a world of one: the mean is the delta
        st.adopt(eta)
        assert fr.same_bits(_np(st.anchor), a) and fr.same_bits(_np(flat.data), p2)
        assert fr.same_bits(_np(flat.grad), g0)
        if beta > 0:
            assert fr.same_bits(_np(st.u), u)
        got = float(st.drift)
        print(f"n={n} drift {got!r} fp64 {drift!r} rel {abs(got - drift) / drift:.3e}")
        assert abs(got - drift) <= 1e-10 * drift


@pytest.mark.parametrize("n", [2053, SIZES[-1]])
def test_drift_is_identical_on_two_runs(inputs, n):
    a0, steps = inputs[n]
    got = []
    for _ in range(2):
        flat, st = _state(a0, 0.0)
        flat.data.add_(torch.from_numpy(steps[0]).cuda())
        st.delta(W_ODD)
        st.adopt(1.0)
        got.append(_np(st._work).copy())
    assert np.array_equal(got[0].view(np.uint64), got[1].view(np.uint64))
    assert got[0][-1] > 0
    # the drift does not see the site weight
    t = (a0 + steps[0]).astype(np.float32) - a0
    want = float(np.sqrt(np.sum(t.astype(np.float64) ** 2)))
    assert abs(got[0][-1] - want) <= 1e-10 * want


@pytest.mark.parametrize("beta", [0.0, 0.9])
def test_non_finite_parameters_pass_through(beta):
    n = 2053
    a0 = np.random.default_rng(1).standard_normal(n).astype(np.float32)
    flat, st = _state(a0, beta)
    where = {3: float("nan"), 1024: float("inf"), 2050: float("-inf"), 2052: float("nan")}
    for i, v in where.items():  # float4 body and scalar tail
        flat.data[i] = v
    p = _np(flat.data)
    st.delta(W_ODD)
    d = _np(flat.grad)
    want, _ = fr.delta(p, a0, W_ODD)
    assert fr.same_bits(d, want)
    for i, v in where.items():
        assert np.isnan(d[i]) if v != v else d[i] == v
    st.adopt(1.0)
    p2 = _np(flat.data)
    for i, v in where.items():
        assert np.isnan(p2[i]) if v != v else p2[i] == v
    assert np.isfinite(np.delete(p2, list(where))).all()
    assert not np.isfinite(float(st.drift))


def test_launchers_refuse_bad_shapes():
    from dinunet_implementations_amd.ops import _lib
    flat, st = _state(np.zeros(64, dtype=np.float32), 0.9)
    L, s = _lib.lib(), _lib.stream()
    p, a, g, u, w = (t.data_ptr() for t in (flat.data, st.anchor, flat.grad, st.u, st._work))
    assert L.dn_fedavg_delta(p, a, g, 0, 1.0, w, s) == DN_BAD_SHAPE
    assert L.dn_fedavg_delta(p, a, g, -4, 1.0, w, s) == DN_BAD_SHAPE
    assert L.dn_fedavg_adopt(p, a, g, u, 0, 1.0, 0.9, w, s) == DN_BAD_SHAPE
    for k in range(3):  # each pointer 4 bytes off a 16-byte boundary
        args = [p, a, g]
        args[k] += 4
        assert L.dn_fedavg_delta(*args, 8, 1.0, w, s) == DN_BAD_SHAPE
    for k in range(4):
        args = [p, a, g, u]
        args[k] += 4
        assert L.dn_fedavg_adopt(*args, 8, 1.0, 0.9, w, s) == DN_BAD_SHAPE
    torch.cuda.synchronize()
    assert not flat.grad.any() and not st.u.any()  # nothing was launched


# ---- device-fed against host-fed ------------------------------------------------------------------
K_LOCAL, NB, EPOCHS = 2, 5, 2   # segments of 2, 2 and 1 updates: a partial last segment


def _fed(group=None, cfg=None):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.step import TrainStep
    from test_step_gpu import _model
    m = _model(0)
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3)
    grp = group or SiteGroup(device=torch.device("cuda"))
    eng = make_engine("fedAvg", m, flat, grp,
                      {"precision_bits": "32", "fedavg_local_steps": K_LOCAL, **(cfg or {})})
    eng.begin()
    # the step gets the solo dSGD engine: the local updates are one-site steps
    return eng, flat, TrainStep(m, flat, opt, eng.local, task="ica", use_graph=True)


def _data():
    from test_step_gpu import _batches
    xs, ys = _batches(n=6, B=8, S=4)  # 4 windows per subject
    return xs.reshape(-1, *xs.shape[2:]).to(torch.bfloat16), ys.reshape(-1), xs.shape[1]


def _orders(X, B):
    g = torch.Generator(device="cuda").manual_seed(5)
    return [torch.randint(0, X.shape[0], (NB * B,), device="cuda", generator=g)
            for _ in range(EPOCHS)]


def _recorder(eng, step, log):
    def after():
        eng.round()
        log.append((step.opt.step_count, bool(eng.flat.grad.any()), eng.drift))
    return after


def _device_fed(group=None, cfg=None):
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    X, Y, B = _data()
    eng, flat, step = _fed(group, cfg)
    feed = DeviceFeed(step, X, Y, B, NB, col=1, segment=K_LOCAL)
    assert feed.segments() == [2, 2, 1] and step._dK == 2
    log = []
    for order in _orders(X, B):
        feed.run_epoch(order, after=_recorder(eng, step, log))
    torch.cuda.synchronize()
    return eng, flat, step, log


@pytest.fixture(scope="module")
def device_run():
    return _device_fed()


def test_device_fed_segments_match_the_host_loop(device_run):
    X, Y, B = _data()
    eh, fh, sh = _fed()
    host = []
    after = _recorder(eh, sh, host)
    for order in _orders(X, B):
        for c in range(NB):
            rows = order[c * B:(c + 1) * B]
            sh(X[rows].float(), Y[rows])
            if eh.round_due(c + 1, NB):
                after()
    torch.cuda.synchronize()
    ed, fd, sd, dev = device_run
    # the same rounds at the same update numbers, the gradient buffer zero after every one
    assert [u for u, _, _ in host] == [u for u, _, _ in dev] == [2, 4, 5, 7, 9, 10]
    assert not any(dirty for _, dirty, _ in host + dev)
    assert eh.rounds == ed.rounds == 6 and sd.opt.step_count == sh.opt.step_count == 10
    assert all(d > 0 for _, _, d in dev)
    # the local updates ran the one-site step form: whole steps, the update inside the replays
    assert set(sd._dgraphs) == {2, 1}
    assert all(v[2] is True for v in sd._dgraphs.values()), "the update must be inside the replays"
    assert sd.engine is ed.local and not sd.engine.group.distributed and not sd.comm_graph
    # ... the very form a one-site dSGD trainer binds on this feed
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    from test_step_gpu import _trainer
    _, _, solo = _trainer(0, use_graph=True)
    DeviceFeed(solo, X, Y, B, NB, col=1, steps_per_graph=2)
    assert (sd._apack is not None, sd._slabs_ok()) == (solo._apack is not None, solo._slabs_ok())
    assert ed.comm_bytes == 0
    assert torch.allclose(fh.data, fd.data, rtol=1e-6, atol=1e-7), (fh.data - fd.data).abs().max()
    assert torch.equal(ed.state.anchor, fd.data)


def test_prepare_captures_the_segment_graphs():
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    X, Y, B = _data()
    eng, flat, step = _fed()
    feed = DeviceFeed(step, X, Y, B, NB, col=1, segment=K_LOCAL)
    feed.run(step.eager_warmup)  # the warm-up steps precede every capture
    feed.prepare(NB)
    assert set(step._dgraphs) == {2, 1}
    graphs = dict(step._dgraphs)
    feed.run_epoch(_orders(X, B)[0], after=eng.round)
    torch.cuda.synchronize()
    assert all(step._dgraphs[k] is graphs[k] for k in graphs) and eng.rounds == 3


def test_one_rank_rccl_runs_the_distributed_round(device_run, request):
    """The same device-fed run with the round's mean taken over a one-rank RCCL group: the
    distributed path (all-reduce, times 1/W) gives the one-site parameters."""
    rccl1 = request.getfixturevalue("rccl1")
    ed, fd, sd, dev = device_run
    er, frr, sr, log = _device_fed(rccl1)
    assert er.group.distributed and not er.local.group.distributed
    assert [u for u, _, _ in log] == [u for u, _, _ in dev]
    assert er.comm_bytes == 6 * 4 * frr.grad.numel()
    assert all(v[2] is True for v in sr._dgraphs.values())
    assert torch.equal(frr.data, fd.data)
    assert [d for _, _, d in log] == [d for _, _, d in dev]


@pytest.fixture
def rccl1():
    import torch.distributed as dist
    from mp_util import init_one_rank_rccl
    from test_step_gpu import _OneRankGroup
    init_one_rank_rccl()
    try:
        yield _OneRankGroup(dist.group.WORLD)
    finally:
        dist.destroy_process_group()
