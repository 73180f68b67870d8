"""The trimmed-mean engine across 3 processes that share the one GPU (``tools/multirank_check.py
--engine trimmedMean --trim 1 --oracle``; two ranks would make the median a plain mean): once
over gloo, where the all-gather of the gradients is issued from the host after the replay, and
once with ``dsgd_collective=peer``, where it runs inside the captured step.  Replicas must end
bit-identical, the first reduced gradient must equal the numpy mirror fed with every rank's own
local gradient bit for bit, and the per-site counters must equal the mirror's counts."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("collective", ["auto", "peer"])
def test_trimmed_mean_three_ranks_match_the_mirror(collective):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mp_util import free_port
    env = dict(os.environ, DINUNET_BACKEND="gloo", PYTHONPATH=ROOT, OMP_NUM_THREADS="2")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node",
           "3", "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tools", "multirank_check.py"), "--engine", "trimmedMean",
           "--trim", "1", "--precision", "32", "--oracle", "--collective", collective]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=110)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads(lines[-1])
    assert res["ok"] and res["max_abs_diff"] == 0.0, res  # bit-identical replicas
    assert res["grad_bit_exact"] is True and res["grad_mismatches"] == 0, res
    assert res["trimmed_counts_exact"] is True, res
    assert res["oracle_ok"] is True and res["graph"] and res["world"] == 3, res
    assert res["trim_sites"] == 1, res
    peer = collective == "peer"
    assert res["peer"] == peer and res["comm_graph"] == peer, res
    assert res["trim_exchange"].startswith("peer gather" if peer else "all-gather"), res
    assert r.returncode == 0, r.stderr[-3000:]
