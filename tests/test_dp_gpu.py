"""Differentially private gradient release on the GPU (csrc/kernels/dp.hip): the two launches
against the fp64 mirror ``ops.reference.dp_privatize``, the bit-exact cases, the device-side
release counter under HIP-graph replay, the non-finite guard, and the release inside the training
step (host-fed eager, device-fed K-step graphs, accumulation, a one-rank RCCL group)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"

# Largest |z_gpu - z_mirror| over the sizes and keys below, measured on an MI355X (zero gradient,
# sigma = c = 1, so the output IS z): 5.262e-07, at |z| = 4.40 (profiles/dp_noise_error.md).  The
# bound is that with a margin of 4x for math-library differences.
TOL_Z_OBSERVED = 5.262e-07
TOL_Z = 4 * TOL_Z_OBSERVED  # 2.105e-06

SIZES = (4, 1028, 262148)  # one thread; a partial wave; 256 * 256 * 4 + 4: the grid stride wraps
# (seed, stream, t): the second has a high seed word, a fold / phase / rank stream word and a
# release number past 2^32
KEYS = ((1234, 0, 1), ((0x9E3779B9 << 32) | 0x12345678, 3 * 4096 + 2048 + 5, 2 ** 32 + 7))
C, SIGMA = 1.0, 0.75
U = 2.0 ** -23


def _state(c=C, sigma=SIGMA, seed=1234, stream=0, t=1):
    from dinunet_implementations_amd.ops import DPState
    d = DPState(DEV, c, sigma, seed=seed, stream=stream)
    d.load_state_dict({"seed": seed, "stream": stream, "t": t - 1})
    return d


def _grad(n, norm, seed=0):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n + seed))
    return (g * (norm / float(torch.linalg.vector_norm(g.double())))).float()


def _ulp_apart(a: float, b: float) -> bool:
    ta, tb = torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)
    return bool(ta == tb) or bool(torch.nextafter(ta, tb) == tb)


@pytest.mark.parametrize("key", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_noise_matches_the_mirror(n, key):
    """Zero gradient, sigma = c = 1: the output is the generator's z itself."""
    from dinunet_implementations_amd.ops import reference
    seed, stream, t = KEYS[key]
    d = _state(1.0, 1.0, seed, stream, t)
    g = torch.zeros(n, device=DEV)
    d.privatize_(g)
    z = reference.dp_noise(n, seed, stream, t)
    err = float((g.cpu().double() - z).abs().max())
    print(f"n {n} key {key}: max |z_gpu - z_mirror| = {err:.3e}")
    assert d.releases == t and d.clipped == 0 and d.last_norm == 0.0
    assert err <= TOL_Z


@pytest.mark.parametrize("key", [0, 1])
@pytest.mark.parametrize("norm", [0.5, 3.0])  # G < c; G > c
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_the_fp64_mirror(n, norm, key):
    from dinunet_implementations_amd.ops import reference
    seed, stream, t = KEYS[key]
    g0 = _grad(n, norm)
    d = _state(C, SIGMA, seed, stream, t)
    g = g0.to(DEV)
    d.privatize_(g)
    got = g.cpu().double()
    want = reference.dp_privatize(g0, C, SIGMA, seed, stream, t)
    coef, G = reference.dp_coef(g0, C)
    z = reference.dp_noise(n, seed, stream, t)
    bound = TOL_Z * SIGMA * C + 4 * U * ((coef * g0.double()).abs() + (SIGMA * C * z).abs())
    err = (got - want).abs()
    print(f"n {n} G {G:.4f} key {key}: max err {float(err.max()):.3e}, "
          f"max err / bound {float((err / bound).max()):.3f}")
    assert (coef == 1.0) == (norm < C)
    assert _ulp_apart(d.last_norm, G) and d.clipped == int(norm > C) and d.releases == t
    assert bool((err <= bound).all())


@pytest.mark.parametrize("n", SIZES)
def test_sigma_zero_is_bit_exact(n):
    from dinunet_implementations_amd.ops import reference
    for norm in (0.5, 3.0):
        g0 = _grad(n, norm, seed=3)
        d = _state(C, 0.0)
        g = g0.to(DEV)
        d.privatize_(g)
        coef, G = reference.dp_coef(g0, C)
        if norm <= C:  # G <= c: the gradient comes back bit for bit
            assert coef == 1.0 and torch.equal(g.cpu(), g0) and d.clipped == 0
            continue
        # G > c: exactly fp32(coef) * g, coef at most one ulp from the mirror's
        cm = torch.tensor(coef, dtype=torch.float32)
        cands = [cm, torch.nextafter(cm, cm.new_tensor(0.0)), torch.nextafter(cm, cm.new_tensor(2.0))]
        hits = [bool(torch.equal(g.cpu(), k * g0)) for k in cands]
        print(f"n {n}: coef mirror {coef!r}, matched {hits}")
        assert any(hits) and d.clipped == 1
    assert d.releases == 1 and d.nonfinite == 0


def test_counter_lives_on_the_device(monkeypatch):
    """One captured graph replayed on a refilled gradient: releases t = 1, 2, 3 with three
    different noise vectors; a host write to the multiplier reaches the same graph."""
    from dinunet_implementations_amd.ops import reference
    n, seed, stream = 1028, 77, 9
    g0 = _grad(n, 3.0, seed=1)
    d = _state(C, SIGMA, seed, stream)
    g = g0.to(DEV)
    d.privatize_(g)  # (library loaded and the kernels resident before the capture)
    torch.cuda.synchronize()
    d.load_state_dict({"seed": seed, "stream": stream, "t": 0})
    src = g0.to(DEV)
    gr = torch.cuda.CUDAGraph()
    g.copy_(src)
    with torch.cuda.graph(gr):
        d.privatize_(g)
    assert d.releases == 0  # captured, not run
    coef, _ = reference.dp_coef(g0, C)
    z = reference.dp_noise
    noise = []
    for t in (1, 2, 3):
        g.copy_(src)
        gr.replay()
        got = g.cpu().double()
        want = reference.dp_privatize(g0, C, SIGMA, seed, stream, t)
        zt = z(n, seed, stream, t)
        bound = TOL_Z * SIGMA * C + 4 * U * ((coef * g0.double()).abs() + (SIGMA * C * zt).abs())
        assert bool(((got - want).abs() <= bound).all()), t
        noise.append(got - coef * g0.double())
    assert d.releases == 3 and d.clipped == 3
    for a in range(3):
        for b in range(a + 1, 3):
            assert float((noise[a] - noise[b]).abs().max()) > 0.1 * SIGMA * C
    d.noise_multiplier = 0.0  # the same graph, no noise now
    g.copy_(src)
    gr.replay()
    cm = torch.tensor(coef, dtype=torch.float32)
    cands = [cm, torch.nextafter(cm, cm.new_tensor(0.0)), torch.nextafter(cm, cm.new_tensor(2.0))]
    assert any(bool(torch.equal(g.cpu(), k * g0)) for k in cands)
    assert d.releases == 4
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        d.noise_multiplier = 1.0
    with pytest.raises(RuntimeError, match="capture"):
        d.clip_norm = 2.0
    monkeypatch.undo()
    assert d.noise_multiplier == 0.0 and d.clip_norm == C


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_releases_nothing(bad):
    n = 1028
    g = _grad(n, 0.5).to(DEV)
    g[n // 2] = bad
    d = _state()
    d.privatize_(g)
    assert bool(torch.isnan(g).all())
    assert d.nonfinite == 1 and d.clipped == 0 and d.releases == 1
    assert not math.isfinite(d.last_norm)


# ---- the release inside the training step --------------------------------------------------------
CLIP, NOISE = 0.05, 2e-3  # c below the small model's gradient norm (test_grad_clip_gpu's C1);
#                           sigma c = 1e-4 per element: the size of the clipped gradient's elements


def _ica(seed=0):
    from dinunet_implementations_amd.models import ICALstm
    torch.manual_seed(seed)
    m = ICALstm(input_size=64, hidden_size=128, num_comps=20, window_size=10).cuda().train()
    m.classifier[0].p = 0.0
    return m


def _trainer(group=None, dp_seed=11, **kw):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.step import TrainStep
    m = _ica(0)
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3)
    eng = make_engine("dSGD", m, flat, group or SiteGroup(device=torch.device("cuda")),
                      {"precision_bits": "32", "dp_clip_norm": CLIP, "dp_noise_multiplier": NOISE,
                       "dp_seed": dp_seed, "dp_fold": 1})
    return m, flat, TrainStep(m, flat, opt, eng, task="ica", **kw)


def _data(n=8):
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = torch.randn(n, 8, 12, 20, 10, device="cuda", generator=gen)
    ys = torch.randint(0, 2, (n, 8), device="cuda", generator=gen)
    return xs, ys, xs.reshape(-1, *xs.shape[2:]).to(torch.bfloat16), ys.reshape(-1)


def test_device_fed_graphs_match_the_host_fed_loop(monkeypatch):
    """Host-fed eager steps against device-fed 4-step graphs with the Adam-emitted pack over the
    same 8 batches, at test_grad_clip_gpu's tolerance for the same comparison without noise."""
    from dinunet_implementations_amd.ops import DeviceSource
    from dinunet_implementations_amd.runtime import step as step_mod
    monkeypatch.setattr(step_mod, "ADAM_PACK", True)
    _, _, X, Y = _data(8)
    B = 8
    src = DeviceSource(X, Y, B)

    def host(**kw):
        _, f, s = _trainer(use_graph=False, **kw)
        norms = []
        for c in range(8):
            xb, yb = src.batch(c)
            s(xb.float(), yb)
            norms.append(s.engine.dp.last_norm)
        torch.cuda.synchronize()
        return f, s, norms

    fh, sh, norms = host()
    _, fd, sd = _trainer(use_graph=True)
    assert sd.engine.dp.stream == sh.engine.dp.stream == 4096
    sd.bind(src, steps_per_graph=4)
    assert sd._apack is not None
    sd.run(8)
    torch.cuda.synchronize()
    assert 4 in sd._dgraphs and sd._dgraphs[4][2], "the release must be inside the 4-step graph"
    print("host norms", norms, "max |host - device-fed|", float((fh.data - fd.data).abs().max()))
    assert min(norms) > CLIP  # every release clipped
    assert sh.engine.dp.releases == sd.engine.dp.releases == 8
    assert sh.engine.dp.clipped == sd.engine.dp.clipped == 8
    assert torch.allclose(fh.data, fd.data, rtol=1e-6, atol=1e-7)
    fo, so, _ = host(dp_seed=12)  # another key: another trajectory
    assert so.engine.dp.releases == 8
    assert not torch.allclose(fo.data, fh.data, rtol=1e-6, atol=1e-7)


def test_accumulation_releases_once_per_update(monkeypatch):
    from dinunet_implementations_amd.runtime import step as step_mod
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    monkeypatch.setattr(step_mod, "ADAM_PACK", False)
    _, _, X, Y = _data(6)
    B, nb, accum = 8, 5, 2
    _, fh, sh = _trainer(use_graph=True, accum=accum)
    _, fd, sd = _trainer(use_graph=True, accum=accum)
    feed = DeviceFeed(sd, X, Y, B, nb, col=1, steps_per_graph=4)
    order = torch.randint(0, X.shape[0], (nb * accum * B,), device="cuda",
                          generator=torch.Generator(device="cuda").manual_seed(5))
    for c in range(nb * accum):
        rows = order[c * B:(c + 1) * B]
        sh(X[rows].float(), Y[rows], first=c % accum == 0, last=c % accum == accum - 1)
    feed.run_epoch(order)
    torch.cuda.synchronize()
    assert all(v[2] for v in sd._dgraphs.values()), "the update must be inside the replays"
    assert sd.opt.step_count == sh.opt.step_count == nb
    assert sd.engine.dp.releases == sh.engine.dp.releases == nb  # not nb * accum
    assert torch.allclose(fh.data, fd.data, rtol=1e-6, atol=1e-7), (fh.data - fd.data).abs().max()


@pytest.fixture
def loopback():
    """A one-rank RCCL group that takes every collective code path."""
    from dinunet_implementations_amd.parallel import init_sites, shutdown
    grp = init_sites(loopback=True)
    try:
        yield grp
    finally:
        shutdown()


def test_loopback_group_releases_before_anything_leaves(loopback, monkeypatch):
    """The captured step over a one-rank RCCL group (sum over one site = identity): the same
    trajectory as the non-distributed step at the same seed and stream, with every bucket
    started inside reduce() -- also when the split capture is forced."""
    xs, ys, _, _ = _data(6)

    def run(step):
        for i in range(xs.shape[0]):
            step(xs[i], ys[i])
        torch.cuda.synchronize()

    assert loopback.distributed and loopback.rank == 0
    _, f1, s1 = _trainer(use_graph=True)
    _, f2, s2 = _trainer(group=loopback, use_graph=True)
    assert not s2.engine.prefers_split and not s2.split and not s2.engine.overlap
    assert s2.engine.dp.stream == s1.engine.dp.stream
    run(s1)
    run(s2)
    assert s2.graph is not None and s1.engine.dp.releases == s2.engine.dp.releases == 6
    assert s2.engine.comm_bytes == f2.numel * 4  # the collective ran
    assert s2.engine.early_launches == 0
    assert torch.equal(f1.data, f2.data), (f1.data - f2.data).abs().max()
    monkeypatch.setenv("DINUNET_SPLIT_GRAPH", "1")
    _, f3, s3 = _trainer(group=loopback, use_graph=True)
    assert s3.split
    run(s3)
    assert s3.engine.early_launches == 0 and s3.engine.dp.releases == 6
    assert torch.allclose(f1.data, f3.data, rtol=1e-6, atol=1e-7), (f1.data - f3.data).abs().max()
