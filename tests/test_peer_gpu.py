"""The peer exchange (``parallel.peer``, ``csrc/kernels/peer.hip``) with real cross-process device
traffic: 2 / 4 site processes share one MI355X, map each other's uncached arenas through IPC
handles and run the site-mean (every wire type) and the factor all-gather eagerly and inside a
captured HIP graph replayed with fresh data, against an fp64 reference; every replica must hold
the bit-identical mean (``tools/peer_check.py``)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world,wire,wait", [(2, "all", "launch"), (4, "fp16", "launch"),
                                             (4, "all", "inline")])
def test_peer_exchange_multiprocess(world, wire, wait):
    """``wait``: the waits as one-workgroup launches of their own (what sites sharing a GPU use)
    or inside the data launches (one site per GPU, production; safe here: no other kernels)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mp_util import free_port
    env = dict(os.environ, DINUNET_BACKEND="gloo", PYTHONPATH=ROOT, OMP_NUM_THREADS="2",
               DINUNET_PEER_TIMEOUT_MS="20000", DINUNET_PEER_WAIT=wait)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tools", "peer_check.py"), "--wire", wire, "--reps", "3"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1])
    log = os.environ.get("DINUNET_ERR_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"test": "peer", **res}) + "\n")
    assert res["ok"], res
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("world,wire", [(2, "all"), (4, "fp16")])
def test_peer_exchange_equals_the_wire_model(world, wire, tmp_path):
    """``PeerMean`` and ``PeerGather`` on the edge and poisoned gradients of ``tests/wire_ref.py``
    (n = 12 * 2048 * world + 5: the last rank-block is nearly all padding; m = 5003), eagerly and
    in a captured graph: every fp32 result equals the exact model's in every bit (both-NaN
    positions apart), on every replica, with a clean error word."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mp_util import free_port
    import wire_ref as R
    n, m = 12 * R.SB * world + 5, 5003
    xs, planted = R.poisoned(R.edge_gradients(n, world, seed=world))
    assert sorted(planted.values()) == ["+inf", "-inf", "nan", "nan"]
    gs = R.edge_gradients(m, world, seed=7 + world)
    gs[world - 1][1234] = np.nan
    gs[0][4321] = -np.inf
    wires = list(R.WIRES) if wire == "all" else [wire]
    data = {f"mean_{r}": xs[r] for r in range(world)}
    data.update({f"gather_{r}": gs[r] for r in range(world)})
    for w in wires:
        data[f"mean_{w}"] = R.site_mean(xs, w)
        data[f"gather_{w}"] = np.stack([R.gathered(g, w) for g in gs])
        assert sorted(np.flatnonzero(np.isnan(data[f"mean_{w}"])).tolist()) == sorted(
            i for i, k in planted.items() if k == "nan")
    path = str(tmp_path / "wire_inputs.npz")
    np.savez(path, **data)
    env = dict(os.environ, DINUNET_BACKEND="gloo", PYTHONPATH=ROOT, OMP_NUM_THREADS="2",
               DINUNET_PEER_TIMEOUT_MS="20000", DINUNET_PEER_WAIT="launch")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tools", "peer_check.py"), "--wire", wire, "--inputs", path]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1])
    log = os.environ.get("DINUNET_ERR_LOG")
    if log:
        with open(log, "a") as f:
            f.write(json.dumps({"test": "peer-wire", **res}) + "\n")
    for w in wires:
        assert res[w]["mean_mismatches"] == {"eager": 0, "graph": 0}, res
        assert res[w]["gather_mismatches"] == {"eager": 0, "graph": 0}, res
        assert res[w]["replicas_identical"] and res[w]["error_word"] == 0, res
    assert res["ok"], res
    assert r.returncode == 0, r.stderr[-3000:]
