"""Secure aggregation on the GPU (``csrc/kernels/secagg.hip``, the ``u64`` wire of ``peer.hip``):
the mask and open kernels bit for bit against the numpy mirror, releases replayed from a captured
graph, the uint64 peer exchange across processes sharing the GPU, and two site processes through
the production step (``tools/secagg_check.py``)."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
DOM = 2 * 4096 + 2048
T0 = (1 << 32) + 4  # releases so far: the next release number has both halves set


def _sweep():
    """Blocks of one full sweep of the mask launch's grid (256 threads per workgroup)."""
    from dinunet_implementations_amd.ops import secagg
    return secagg.PARTS * 256


def _n_big():
    return 8 * (_sweep() + 1)


def tkey(i, j, distinct=True):
    a, b = min(i, j), max(i, j)
    if not distinct:  # the large case: three keys serve every pair (one generator run each)
        a, b = (a + b) % 3, 255
    return hashlib.sha256(b"secagg-gpu-test" + bytes([a, b])).digest()


def tkeys(W, rank, distinct=True):
    return [None if j == rank else tkey(rank, j, distinct) for j in range(W)]


@functools.lru_cache(maxsize=None)
def _prg(key, n, t, dom):
    from dinunet_implementations_amd.ops import reference
    return reference.secagg_prg(key, n, t, dom)


def mirror_wire(g, keys, rank, t, dom):
    """``reference.secagg_mask`` with the pair masks computed once per key."""
    from dinunet_implementations_amd.ops import reference
    wire, _, _ = reference.secagg_quantize(g)
    n = wire.size - 8
    with np.errstate(over="ignore"):
        for j, k in enumerate(keys):
            if j != rank:
                m = _prg(bytes(k), n, t, dom)
                wire = wire + m if j > rank else wire - m
    return wire


def _grad(n, seed, scale=0.3):
    g = torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale
    g[0], g[n - 1] = 3e5, -2.0 ** 18  # one clamped element; one at the clamp
    g[1], g[2] = 2.0 ** -41, -2.0 ** -40
    return g


def _state(W, rank, keys, t=T0, dom=DOM):
    from dinunet_implementations_amd.ops import SecAggState
    s = SecAggState(DEV, W, rank, keys, dom)
    s.load_state_dict({"t": t})
    return s


# ---- mask kernel --------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 8, 12, 2052, "sweep+1"])
@pytest.mark.parametrize("W", [2, 3, 16])
def test_mask_kernel_matches_the_mirror(W, n):
    from dinunet_implementations_amd.ops import reference
    big = n == "sweep+1"
    n = _n_big() if big else n
    g = _grad(n, seed=W)
    gd = g.to(DEV)
    plain = reference.secagg_quantize(g)[0]
    for rank in range(W):
        keys = tkeys(W, rank, distinct=not big)
        s = _state(W, rank, keys)
        wire = s.mask_(gd, s.wire_like(gd))
        got = wire.cpu().numpy().view(np.uint64)
        want = mirror_wire(g, keys, rank, T0 + 1, DOM)
        assert np.array_equal(got, want), (W, n, rank, int((got != want).sum()))
        assert not np.array_equal(got[n:], plain[n:])  # the tail block is masked too
        assert s.releases == T0  # the opening advances it
    assert torch.equal(gd.cpu(), g)


def test_mask_refuses_bad_shapes():
    s = _state(2, 0, tkeys(2, 0))
    g = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError):
        s.mask_(torch.zeros(6, device=DEV), torch.zeros(14, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        s.mask_(g, torch.zeros(8, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        s.mask_(torch.zeros(8), torch.zeros(16, dtype=torch.int64))


# ---- open kernel --------------------------------------------------------------------------------
def _release(W, grads, states):
    """One release of W simulated parties in this process: the opened means and the wires."""
    wires = [s.mask_(g, s.wire_like(g)) for s, g in zip(states, grads)]
    total = wires[0].clone()
    for w in wires[1:]:
        total += w  # torch's int64 add wraps
    outs = []
    for s, g in zip(states, grads):
        o = torch.empty_like(g)
        s.open_(total, o)
        outs.append(o)
    return outs, wires


@pytest.mark.parametrize("W,n", [(2, 12), (3, 2052), (16, 2052), (3, 300_004)])
def test_open_kernel_matches_the_mirror(W, n):
    from dinunet_implementations_amd.ops import reference
    grads = [_grad(n, seed=10 * W + r, scale=2.0 ** (r % 5 - 2)) for r in range(W)]
    for r in range(W):  # the summed magnitude at its largest, both signs
        grads[r][4], grads[r][5] = 2.0 ** 18, -2.0 ** 18
    states = [_state(W, r, tkeys(W, r), t=0) for r in range(W)]
    outs, _ = _release(W, [g.to(DEV) for g in grads], states)
    want, sat, bad = reference.secagg_mean(grads)
    assert sat == W and bad == 0
    for s, o in zip(states, outs):
        assert torch.equal(o.cpu(), want)  # bit for bit
        assert (s.releases, s.saturated, s.last_saturated, s.nonfinite) == (1, W, W, 0)
    m = torch.stack([g.clamp(-2.0 ** 18, 2.0 ** 18) for g in grads]).double().mean(0)
    bound = 2.0 ** -41 + (2.0 ** -24 + 2.0 ** -52) * m.abs()
    assert bool(((want.double() - m).abs() <= bound).all())


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_at_one_party_makes_every_mean_nan(bad):
    W, n = 3, 2052
    grads = [_grad(n, seed=r) for r in range(W)]
    grads[1][n // 2] = bad
    states = [_state(W, r, tkeys(W, r), t=0) for r in range(W)]
    outs, _ = _release(W, [g.to(DEV) for g in grads], states)
    for s, o in zip(states, outs):
        assert bool(torch.isnan(o).all())
        assert (s.nonfinite, s.saturated, s.releases) == (1, W, 1)
    # the next release is clean again
    grads[1][n // 2] = 0.5
    outs, _ = _release(W, [g.to(DEV) for g in grads], states)
    from dinunet_implementations_amd.ops import reference
    assert torch.equal(outs[0].cpu(), reference.secagg_mean(grads)[0])
    assert (states[0].nonfinite, states[0].saturated, states[0].releases) == (1, 2 * W, 2)


# ---- captured replay ----------------------------------------------------------------------------
def test_captured_graph_replays_fresh_masks(monkeypatch):
    from dinunet_implementations_amd.ops import reference
    W, n = 2, 2052
    grads = [_grad(n, seed=40 + r) for r in range(W)]
    gd = [g.to(DEV) for g in grads]
    states = [_state(W, r, tkeys(W, r), t=0) for r in range(W)]
    _release(W, gd, states)  # (library loaded and the kernels resident before the capture)
    torch.cuda.synchronize()
    for s in states:
        s.load_state_dict({"t": 0})
    wires = [s.wire_like(g) for s, g in zip(states, gd)]
    total = torch.zeros_like(wires[0])
    outs = [torch.empty_like(g) for g in gd]
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for s, g, w in zip(states, gd, wires):
            s.mask_(g, w)
        torch.add(wires[0], wires[1], out=total)
        for s, o in zip(states, outs):
            s.open_(total, o)
    assert states[0].releases == 0  # captured, not run
    want, _, _ = reference.secagg_mean(grads)
    seen = []
    for t in (1, 2, 3):
        gr.replay()
        torch.cuda.synchronize()
        w0 = wires[0].cpu().numpy().view(np.uint64).copy()
        assert np.array_equal(w0, mirror_wire(grads[0], tkeys(W, 0), 0, t, DOM)), t
        assert all(torch.equal(o.cpu(), want) for o in outs), t
        seen.append(w0)
    assert states[0].releases == states[1].releases == 3
    for a in range(3):
        for b in range(a + 1, 3):
            x = seen[a] ^ seen[b]
            assert np.unpackbits(x.view(np.uint8)).sum() / x.size > 28  # fresh masks
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="capture"):
        states[0].load_state_dict({"t": 0})
    with pytest.raises(RuntimeError, match="capture"):
        states[0].rekey(tkeys(W, 0))
    monkeypatch.undo()
    assert states[0].releases == 3


# ---- across processes ---------------------------------------------------------------------------
def _run_tool(world, args, wait="launch"):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mp_util import free_port
    env = dict(os.environ, DINUNET_BACKEND="gloo", PYTHONPATH=ROOT, OMP_NUM_THREADS="2",
               DINUNET_PEER_TIMEOUT_MS="20000", DINUNET_PEER_WAIT=wait)
    env.pop("DINUNET_SECURE_AGG", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tools", "secagg_check.py"), *args]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1])
    print(res)
    assert res["ok"], res
    assert r.returncode == 0, r.stderr[-3000:]
    return res


@pytest.mark.parametrize("world,wait", [(2, "launch"), (4, "launch"), (4, "inline")])
def test_peer_u64_wire_multiprocess(world, wait):
    res = _run_tool(world, ["--mode", "wire", "--reps", "3"], wait)
    assert len(res["cases"]) == 3
    for c in res["cases"]:
        assert c["exact"] and c["replicas_identical"] and c["error_word"] == 0


@pytest.mark.parametrize("feed", ["host", "device"])
def test_two_sites_end_to_end(feed):
    res = _run_tool(2, ["--mode", "site", "--feed", feed, "--on", "1", "--steps", "4"])
    assert res["state"] and res["peer"] and res["transport"] == "peer" and res["capturable"]
    assert res["graph"] and res["comm_graph"]
    assert res["mean_bit_equal"] and res["within_bound"] and res["off_on_within_bound"]
    assert res["replicas_identical"] and not any(res["error_words"])
    assert res["releases"] == 4 and res["nonfinite"] == 0
    assert res["secagg_calls"] > 0 and res["u64_launches"] > 0 and res["f32_launches"] == 0


def test_off_path_launches_nothing_new():
    """With the option off: no state, no secure-aggregation launch, no uint64 exchange -- the
    launchers the step calls are those of the fp32 peer exchange."""
    res = _run_tool(2, ["--mode", "site", "--feed", "host", "--on", "0", "--steps", "4",
                        "--collective", "peer"])
    assert res["state"] is False and res["peer"]
    assert res["secagg_calls"] == 0 and res["u64_launches"] == 0 and res["f32_launches"] > 0
    assert res["replicas_identical"]
