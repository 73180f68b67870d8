"""Top-k sparsification on the GPU (``csrc/kernels/topk.hip``): select + compact and combine bit
for bit against the numpy mirror (``ops.reference.topk_select`` / ``topk_combine``), determinism,
graph capture of a one-site ``reduce()`` and the training step in its three forms."""
import numpy as np
import pytest
import torch

from dinunet_implementations_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

NS = (1, 7, 64, 257, 4099, 70001)


def _ks(n):
    return sorted({k for k in (1, 2, n // 3, n - 1, n) if 1 <= k <= n})


def _u32(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t).view(np.uint32)


def _from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def _inputs(n):
    """name -> (g, err) fp32 arrays (err: the residual the release starts from)."""
    rng = np.random.default_rng(n)
    z = np.zeros(n, np.float32)
    i = np.arange(n, dtype=np.uint32)
    special = rng.standard_normal(n).astype(np.float32)
    special[(n * 2) // 3] = np.inf
    special[n // 3] = np.nan  # (n = 1: the NaN alone)
    signs = _from_bits(rng.integers(0, 2, n).astype(np.uint32) << 31)
    return {
        "normal": (rng.standard_normal(n).astype(np.float32), z),
        # five values all over the range: every tie bucket spans the workgroups' ranges
        "ties": (rng.choice(np.array([0, 1, -1, 2, -2], np.float32), n), z),
        "zeros": (z, z),
        "equal": (np.full(n, -0.75, np.float32), z),
        # (-0 + -0 = -0, every other pair gives +0: both signs reach the accumulator)
        "signed_zeros": (signs, _from_bits(rng.integers(0, 2, n).astype(np.uint32) << 31)),
        "inf_nan": (special, z),
        # 1.0 + j ulp, j < 256: the first three digit passes see one bin
        "low_digit": (_from_bits(np.uint32(0x3F800000) | ((i * np.uint32(37)) % np.uint32(256))), z),
        # the top digit alone differs (0 .. 126: finite), the first pass decides
        "high_digit": (_from_bits(((i * np.uint32(7)) % np.uint32(127)) << np.uint32(24)
                                  | np.uint32(0x00123456)), z),
        "residual": (rng.standard_normal(n).astype(np.float32),
                     (rng.standard_normal(n) * 2).astype(np.float32)),
    }


def _state(n, k, err=None, idx_float=False):
    from dinunet_implementations_amd.ops import TopKState
    st = TopKState("cuda", n, k, idx_float=idx_float)
    if err is not None:
        st.err.copy_(torch.from_numpy(err))
    return st


def _check_release(st, g, err, k, what):
    st.select(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    idx, val, err_new = ref.topk_select(g, err, k)
    got_idx = st.idx.cpu().numpy()
    assert got_idx.dtype == np.int32 and np.array_equal(got_idx, idx), what
    assert np.array_equal(_u32(st.val), _u32(val)), what
    assert np.array_equal(_u32(st.err), _u32(err_new)), what
    assert not st.scratch[:1024].any(), what  # the histograms are left clear
    return err_new


@pytest.mark.parametrize("n", NS)
def test_select_and_compact_match_the_mirror(n):
    for name, (g, err) in _inputs(n).items():
        for k in _ks(n):
            st = _state(n, k, err)
            e1 = _check_release(st, g, err, k, (name, n, k))
            if name == "residual":  # a second release from the residual the first one left
                _check_release(st, np.roll(g, 3) * np.float32(0.5), e1, k, (name, n, k, 2))


def test_float_index_words_carry_the_same_release():
    n, k = 4099, 1366
    g, err = _inputs(n)["residual"]
    st = _state(n, k, err, idx_float=True)
    _check_release(st, g, err, k, "idx_float")
    assert st.send[:k].dtype == torch.float32
    assert torch.equal(st.send[:k].cpu(), st.idx.cpu().float())


def _pair_sets(kind, W, n, k, rng):
    base = np.sort(rng.choice(n, k, replace=False))
    out = []
    for w in range(W):
        if kind == "identical":
            idx = base
        elif kind == "disjoint":  # rank w takes the indices = w mod W
            idx = (np.arange(k) * W + w) if k * W <= n else base
        else:  # half shared with every rank, half its own
            own = np.sort(rng.choice(n, k, replace=False))
            idx = np.unique(np.concatenate([base[:k // 2], own]))[:k]
            while idx.size < k:
                idx = np.unique(np.concatenate([idx, rng.choice(n, k, replace=False)]))[:k]
        val = rng.standard_normal(k).astype(np.float32)
        val[::5] = -0.0
        out.append((np.sort(idx).astype(np.int32), val))
    return out


@pytest.mark.parametrize("W", [1, 2, 3, 16])
def test_combine_matches_the_mirror(W):
    n, k = 5003, 257  # three index ranges, the last one ragged
    rng = np.random.default_rng(W)
    for kind in ("disjoint", "identical", "overlap"):
        pairs = _pair_sets(kind, W, n, k, rng)
        assert all(np.unique(i).size == k for i, _ in pairs)
        want = ref.topk_combine(pairs, n)
        for fl in (False, True):
            st = _state(n, k, idx_float=fl)
            words = np.concatenate([np.concatenate(
                [i.astype(np.float32).view(np.uint32) if fl else i.view(np.uint32),
                 v.view(np.uint32)]) for i, v in pairs])
            gathered = torch.from_numpy(words.view(np.float32).copy()).cuda()
            out = torch.full((n,), 7.0, device="cuda")
            st.combine(W, out, gathered)
            torch.cuda.synchronize()
            assert np.array_equal(_u32(out), _u32(want)), (kind, W, fl)


def test_two_runs_give_identical_outputs():
    n, k = 70001, 23333
    g, err = _inputs(n)["ties"]
    outs = []
    for _ in range(2):
        st = _state(n, k, err)
        st.select(torch.from_numpy(g).cuda())
        out = torch.empty(n, device="cuda")
        st.combine(1, out)
        torch.cuda.synchronize()
        outs.append((st.send.clone(), st.err.clone(), out))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _small_engine():
    import torch.nn as nn
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    torch.manual_seed(0)
    m = nn.Sequential(nn.Linear(100, 60), nn.ReLU(), nn.Linear(60, 3)).cuda()
    flat = FlatParams(m.parameters())
    eng = make_engine("topK", m, flat, SiteGroup(device=torch.device("cuda")),
                      {"topk_ratio": 0.05})
    return flat, eng


def test_captured_reduce_replays_on_fresh_gradients():
    fe, ee = _small_engine()
    fg, eg = _small_engine()
    assert eg.capturable and eg.fast and fg.grad.numel() > 4096
    gen = torch.Generator(device="cuda").manual_seed(3)
    fresh = [torch.randn(fg.grad.numel(), device="cuda", generator=gen) for _ in range(3)]
    _small_engine()[1].reduce()  # every kernel has run once before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pre = eg.pre_reduce()
        scale = eg.reduce(factorized=True)
    assert pre is None and scale == 1.0
    torch.cuda.synchronize()
    assert not eg.state.err.any()  # the capture ran nothing
    for t in range(3):
        fg.grad.copy_(fresh[t])
        graph.replay()
        fe.grad.copy_(fresh[t])
        assert ee.reduce() == 1.0
        torch.cuda.synchronize()
        assert torch.equal(fg.grad.view(torch.int32), fe.grad.view(torch.int32)), t
        assert torch.equal(eg.state.err.view(torch.int32), ee.state.err.view(torch.int32)), t
        idx, val, _ = ref.topk_select(fresh[t].cpu().numpy(),
                                      np.zeros(fresh[t].numel(), np.float32), eg.k)
        if t == 0:
            want = ref.topk_combine([(idx, val)], fresh[t].numel())
            assert np.array_equal(_u32(fg.grad), _u32(want))
    assert eg.state.err.any()


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
    eng = make_engine("topK", m, flat, SiteGroup(device=torch.device("cuda")),
                      {"precision_bits": "32", "topk_ratio": 0.01})
    return flat, eng, TrainStep(m, flat, opt, eng, task="ica", use_graph=use_graph)


def test_train_step_forms_agree_bit_for_bit():
    """Host-fed eager, host-fed captured and device-fed steps of one site: after the warm-up
    steps every form has run 3 more steps (the captured ones as replays); weights and residual
    must be the same bits."""
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
    for f, e in ((fc, ec), (fd, ed)):
        assert torch.equal(f.data.view(torch.int32), fe.data.view(torch.int32))
        assert torch.equal(e.state.err.view(torch.int32), ee.state.err.view(torch.int32))
    assert ee.state.err.any() and ee.comm_bytes == 8 * ee.k
