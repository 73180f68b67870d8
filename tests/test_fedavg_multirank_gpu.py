"""Federated-averaging rounds across 3 processes that share the one GPU (``tools/fedavg_check.py``
under ``torch.distributed.run``, ``DINUNET_BACKEND=gloo``; 3 so that a sum in site order differs
from a pairwise one): a small ICA model, ``fedavg_local_steps = 2`` and 3 updates -- one full
round and one partial.  Every rank all-gathers its pre-round parameters and evaluates the numpy
mirror (``tests/fedavg_ref.py``): its delta and its adopted parameters bit for bit, replicas
bit-identical after every round, and the mean it received against

* the fp32 sum in site order times 1/W, bit for bit (the peer exchange on the fp32 wire);
* the fp64 mean within ``2^-23 sum_s |d_s|`` per element (any fp32 mean: a W-term fp32 sum in any
  order plus the 1/W rounding errs by at most ``2^-24 sum |d|`` to first order);
* the fp64 mean within the bound ``tests/wire_ref.py`` derives for a 16-bit wire;
* the fp64 weighted mean (``--weighting samples``, unequal split sizes) under the fp32 bound."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "peer-fp32": ["--collective", "peer"],
    "auto-gloo-allreduce": ["--collective", "auto"],
    "peer-fp16": ["--collective", "peer", "--precision", "16"],
    "peer-samples": ["--collective", "peer", "--weighting", "samples"],
    "auto-samples-momentum": ["--collective", "auto", "--weighting", "samples", "--momentum",
                              "0.9", "--server-lr", "0.5"],
}


@pytest.mark.parametrize("case", list(CASES))
def test_three_ranks_rounds_match_the_mirror(case):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import wire_ref as wr
    from mp_util import free_port
    args = CASES[case]
    env = dict(os.environ, DINUNET_BACKEND="gloo", PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node",
           "3", "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tools", "fedavg_check.py")] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1])
    print(res)
    peer = "peer" in args
    wire = "fp16" if "16" in args else "fp32"
    assert res["world"] == 3 and res["rounds"] == 2 and res["round_updates"] == [2, 3], res
    assert res["peer"] is peer and res["wire"] == wire and res["steps"] == 3, res
    n = res["n"]
    if peer:  # what a site pushes per exchange: W rank-blocks of the wire's payload
        per_round = 3 * wr.numel(wr.chunk_for(n, 3)) * (2 if wire == "fp16" else 4)
    else:     # the fp32 all-reduce
        per_round = 4 * n
    assert res["comm_bytes"] == 2 * per_round, res
    checks = res["checks"]
    assert checks["replicas"] and checks["delta_bits"] and checks["adopt_bits"], res
    assert checks["grad_zero"] and checks["drift"] and checks["mean_bound"], res
    assert ("mean_bit_exact" in checks) == (peer and wire == "fp32"), res
    assert all(checks.values()) and res["ok"], res
    assert res["worst_err_over_bound"] <= 1.0, res
    if "samples" in args:
        assert res["weights"] == [float(w) for w in _weights((3, 5, 8))], res
    else:
        assert res["weights"] == [1.0, 1.0, 1.0], res
    assert r.returncode == 0, r.stderr[-3000:]


def _weights(sizes):
    import fedavg_ref as fr
    return fr.site_weights(sizes)
