"""Coordinate-wise trimmed mean on the GPU (``csrc/kernels/trimmed.hip``): values and per-site
counts bit for bit against the numpy mirror (``ops.reference.trimmed_mean``) for every template
instantiation the tests can reach cheaply, determinism, graph capture of the combine and the
training step in its three forms.

Where the mirror's result is a NaN the comparison is "NaN at the same position": the payload of
a NaN that an addition makes or passes on (inf + -inf, NaN + NaN) is the one thing the contract
leaves to the adder, and the host's and the GPU's differ.  Every other element is compared by
its bits."""
import numpy as np
import pytest
import torch

from dinunet_implementations_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

WS = (1, 2, 3, 4, 5, 8, 16)
# one thread's scalar tail; one full vector; vector + tail; one workgroup's worth +- 1 (1024 = 256
# threads x 4); several workgroups with a tail
NS = (1, 3, 4, 5, 1023, 1024, 4099, 70001)
FLT_MAX = 3.4028234663852886e38


def _u32(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t).view(np.uint32)


_ROWS = {}


def rows_for(W, n):
    """Random bit patterns (every exponent, both signs, NaNs among them) salted with the special
    values and with values repeated across sites; made once per (W, n) and left unchanged."""
    if (W, n) not in _ROWS:
        rng = np.random.default_rng(1000 * W + n)
        u = rng.integers(0, 1 << 32, (W, n), dtype=np.uint64).astype(np.uint32)
        x = u.view(np.float32).copy()
        special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -4e-45, FLT_MAX,
                            -FLT_MAX, 1.0, -1.0], np.float32)
        special[5:6].view(np.uint32)[:] = 0xFFC00001
        hit = rng.random((W, n)) < 0.3
        x[hit] = special[rng.integers(0, special.size, int(hit.sum()))]
        dup = rng.random(n) < 0.25  # the same value at several (here: all later) sites
        w0 = rng.integers(0, W, n)
        for w in range(W):
            m = dup & (w >= w0)
            x[w, m] = x[w0[m], np.nonzero(m)[0]]
        if n >= 4:
            x[:, 0] = FLT_MAX          # the sum overflows
            x[:, 1] = np.float32(-0.0)  # all sites equal
            x[:, 2] = 1e-45             # denormals add up
        _ROWS[(W, n)] = x
    return _ROWS[(W, n)]


def _device_rows(x, n):
    """[W, stride] on the GPU, stride = n rounded up to 4, the padding filled with NaN."""
    W = x.shape[0]
    stride = -(-n // 4) * 4
    buf = torch.full((W, stride), float("nan"), device="cuda")
    buf[:, :n].copy_(torch.from_numpy(x))
    return buf


def _check(st, buf, x, b, what):
    n = x.shape[1]
    big = torch.full((n + 8,), 7.0, device="cuda")
    before = st.counts()
    st.combine(buf, big[:n])
    torch.cuda.synchronize()
    want, trimmed = ref.trimmed_mean(x, b)
    got = big[:n].cpu().numpy()
    assert bool((big[n:] == 7.0).all()), what  # nothing written past n
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(_u32(got)[~nan], _u32(want)[~nan]), what
    assert list(st.counts() - before) == list(trimmed), what
    return got, trimmed


@pytest.mark.parametrize("W", WS)
def test_kernel_matches_the_mirror(W):
    from dinunet_implementations_amd.ops import TrimmedState
    for n in NS:
        x = rows_for(W, n)
        buf = _device_rows(x, n)
        for b in range((W + 1) // 2):
            st = TrimmedState("cuda", n, W, b)
            assert st.stride == buf.shape[1] and st.gather_buffer().shape == buf.shape
            _check(st, buf, x, b, (W, n, b))


@pytest.mark.parametrize("W,n", [(3, 4099), (4, 70001), (16, 70001)])
def test_grid_stride_loop_wraps(W, n):
    """The grid is bounded by the CU count, which 70,001 coordinates do not exhaust: with the
    launch bounded to 3 workgroups (768 threads x 4 coordinates a round) every thread runs the
    loop more than once, the tail included."""
    from dinunet_implementations_amd.ops import TrimmedState
    from dinunet_implementations_amd.ops import trimmed as T
    x = rows_for(W, n)
    buf = _device_rows(x, n)
    T.set_max_blocks(3)
    try:
        for b in sorted({0, (W - 1) // 2}):
            _check(TrimmedState("cuda", n, W, b), buf, x, b, (W, n, b))
    finally:
        T.set_max_blocks(0)


def test_two_runs_give_identical_outputs_and_counts():
    from dinunet_implementations_amd.ops import TrimmedState
    W, n, b = 5, 70001, 1
    x = rows_for(W, n)
    buf = _device_rows(x, n)
    runs = []
    for _ in range(2):
        st = TrimmedState("cuda", n, W, b)
        out = torch.empty(n, device="cuda")
        st.combine(buf, out)
        c1 = st.counts()
        st.combine(buf, out)
        runs.append((out.view(torch.int32).clone(), c1, st.counts() - c1))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert torch.equal(runs[0][1], runs[0][2])  # the same increment every time


def test_combine_errors_on_the_gpu():
    from dinunet_implementations_amd.ops import TrimmedState
    st = TrimmedState("cuda", 6, 3, 1)
    rows, out = st.gather_buffer(), torch.zeros(6, device="cuda")
    assert rows.shape == (3, 8)
    for bad_rows, bad_out in ((rows.cpu(), out), (rows, out.cpu()), (rows[:, :5], out),
                              (torch.zeros(3, 7, device="cuda")[:, :6], out),
                              (rows.double(), out)):
        with pytest.raises(ValueError, match="TrimmedState.combine"):
            st.combine(bad_rows, bad_out)
    st.combine(rows[:, :7], out)  # (a narrower view of the same rows is fine)


def _engine(world=3, trim=1):
    import torch.nn as nn
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    torch.manual_seed(0)
    m = nn.Sequential(nn.Linear(100, 60), nn.ReLU(), nn.Linear(60, 3)).cuda()
    flat = FlatParams(m.parameters())
    grp = SiteGroup(rank=0, world=world, device=torch.device("cuda"))  # (no process group)
    return flat, make_engine("trimmedMean", m, flat, grp, {"trim_sites": trim})


def test_captured_combine_replays_on_fresh_rows():
    """What ``reduce()`` runs after its gather, captured on one rank: the gather buffer is filled
    by hand before every replay."""
    flat, eng = _engine()
    st = eng.state
    n, W = flat.grad.numel(), 3
    assert eng.b == 1 and eng.fast and n > 4096 and st.stride == n
    rows = st.gather_buffer()
    st.combine(rows, flat.grad)  # the kernel has run once before the capture
    torch.cuda.synchronize()
    base = st.counts()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st.combine(rows, flat.grad)
    torch.cuda.synchronize()
    assert torch.equal(st.counts(), base)  # the capture ran nothing
    gen = torch.Generator(device="cuda").manual_seed(3)
    total = np.zeros(W, np.int64)
    for t in range(3):
        fresh = torch.randn(W, n, device="cuda", generator=gen)
        fresh[1, ::7] = float("nan")
        fresh[t % W] *= 1e30
        rows.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        want, trimmed = ref.trimmed_mean(fresh.cpu().numpy(), 1)
        total += trimmed
        assert np.array_equal(_u32(flat.grad), _u32(want)), t
        assert bool(torch.isfinite(flat.grad).all())
        assert list(st.counts() - base) == list(total), t
    share = eng.trimmed_share()
    assert share == pytest.approx([float(c) / (4 * n) for c in (base.numpy() + total)])


def _trainer(use_graph):
    from dinunet_implementations_amd.models import ICALstm
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.step import TrainStep
    torch.manual_seed(0)
    m = ICALstm(input_size=64, hidden_size=128, num_comps=20, window_size=10).cuda().train()
    m.classifier[0].p = 0.0
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3)
    eng = make_engine("trimmedMean", m, flat, SiteGroup(device=torch.device("cuda")),
                      {"precision_bits": "32"})
    return flat, eng, TrainStep(m, flat, opt, eng, task="ica", use_graph=use_graph)


def test_train_step_forms_agree_bit_for_bit():
    """Host-fed eager, host-fed captured and device-fed steps of one site: after the warm-up
    steps every form has run 3 more steps (the captured ones as replays); the weights must be
    the same bits (at one site the engine leaves the gradient as it is)."""
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    g = torch.Generator(device="cuda").manual_seed(7)
    n, B = 6, 8
    xs = torch.randn(n, B, 12, 20, 10, device="cuda", generator=g).bfloat16().float()
    ys = torch.randint(0, 2, (n, B), device="cuda", generator=g)
    fe, ee, se = _trainer(False)
    fc, ec, sc = _trainer(True)
    fd, ed, sd = _trainer(True)
    for i in range(n):
        se(xs[i], ys[i])
        sc(xs[i], ys[i])
    feed = DeviceFeed(sd, xs.reshape(-1, *xs.shape[2:]).to(torch.bfloat16), ys.reshape(-1), B, n,
                      col=1, steps_per_graph=3)
    feed.run(3)
    feed.prepare(n - 3)
    feed.run(n - 3)
    torch.cuda.synchronize()
    assert sc.graph is not None and sc.graph_opt and sd._dgraphs
    assert se.opt.step_count == sc.opt.step_count == sd.opt.step_count == n
    for f in (fc, fd):
        assert torch.equal(f.data.view(torch.int32), fe.data.view(torch.int32))
    assert ee.comm_bytes == 4 * fe.grad.numel() and ee.last_scale == 1.0
    assert not ee.state.counts().any()
