"""Site runs with ``device_eval``: the validation and test passes device-fed
(``runtime.evalfeed``) log exactly what the host evaluation loop logs."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist

from mp_util import free_port, init_one_rank_rccl

pytestmark = pytest.mark.gpu

KEYS = ("train_log", "validation_log", "local_validation_log", "test_metrics", "best_val_epoch")


def _run_site(root, out, overrides, group=None):
    from dinunet_implementations_amd.config import build_config, load_inputspec
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.site import FederatedSite
    from dinunet_implementations_amd.tasks import get_task
    specs = load_inputspec(os.path.join(root, "inputspec.json"))
    cfg = build_config(site_input=specs[0], overrides=overrides)
    state = {"baseDirectory": os.path.join(root, "input", "local0", "simulatorRun")}
    T, D, H = get_task(cfg["task_id"])
    grp = group or SiteGroup(device=torch.device("cuda", 0))
    return FederatedSite(cfg, grp, T, D, H, state, out, verbose=False).run()[0]


def _ica_root(tmp_path, sites=1):
    from dinunet_implementations_amd.data.synthetic import make_ica_sites
    return make_ica_sites(str(tmp_path / "ica"), sites=sites, subjects=(64,) * sites, comps=16,
                          T=120, window_size=10, window_stride=10, hidden_size=64, input_size=32)


def _twins(root, tmp_path, ov, group=None):
    on = _run_site(root, str(tmp_path / "on"), dict(ov, device_eval=True), group)
    off = _run_site(root, str(tmp_path / "off"), dict(ov, device_eval=False), group)
    assert on.get("eval_feed") == "device" and "eval_feed" not in off
    for k in KEYS:
        assert on[k] == off[k], (k, on[k], off[k])
    assert len(on["validation_log"]) == ov["epochs"]
    return on, off


@pytest.mark.parametrize("device_feed", [True, False])
def test_ica_site_device_eval_logs_equal_host_eval(tmp_path, device_feed):
    on, _ = _twins(_ica_root(tmp_path), tmp_path,
                   {"epochs": 3, "batch_size": 8, "seed": 3, "device_feed": device_feed})
    assert (on.get("feed") == "device") == device_feed


def test_ica_site_device_eval_env_switch_and_eval_batch_size(tmp_path, monkeypatch):
    """``DINUNET_DEVICE_EVAL=1`` where the key is unset; ``eval_batch_size`` on both paths."""
    root = _ica_root(tmp_path)
    ov = {"epochs": 2, "batch_size": 8, "seed": 3, "eval_batch_size": 5}
    off = _run_site(root, str(tmp_path / "off"), ov)
    monkeypatch.setenv("DINUNET_DEVICE_EVAL", "1")
    on = _run_site(root, str(tmp_path / "on"), ov)
    assert on.get("eval_feed") == "device" and "eval_feed" not in off
    for k in KEYS:
        assert on[k] == off[k], k


def test_ica_site_device_eval_over_one_rank_rccl(tmp_path):
    from test_step_gpu import _OneRankGroup
    init_one_rank_rccl()
    try:
        _twins(_ica_root(tmp_path), tmp_path, {"epochs": 3, "batch_size": 8, "seed": 3},
               group=_OneRankGroup(dist.group.WORLD))
    finally:
        dist.destroy_process_group()


def test_fs_site_device_eval_logs_equal_host_eval(fs_data_root, tmp_path):
    _twins(fs_data_root, tmp_path, {"epochs": 3, "batch_size": 8, "seed": 3})


def test_ica_two_site_processes_over_gloo_on_one_gpu(tmp_path):
    """Two site processes (gloo, both on the one GPU), with and without ``device_eval``: each
    site's logs equal its twin's."""
    root = _ica_root(tmp_path, sites=2)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DINUNET_BACKEND="gloo", PYTHONPATH=repo, OMP_NUM_THREADS="2")
    env.pop("DINUNET_DEVICE_EVAL", None)
    procs = {}
    for tag, flag in (("on", "true"), ("off", "false")):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1",
               "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
               str(free_port()), "-m", "dinunet_implementations_amd.run", "--data-path", root,
               "--out", str(tmp_path / tag), "--set", "epochs=3", "--set", "batch_size=8",
               "--set", "seed=3", "--set", f"device_eval={flag}"]
        procs[tag] = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True)
    try:
        for tag, p in procs.items():
            _, err = p.communicate(timeout=150)
            assert p.returncode == 0, (tag, err[-4000:])
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()

    def logs(tag, site):
        d = str(tmp_path / tag / site)
        f = next(os.path.join(r, x) for r, _, fs in os.walk(d) for x in fs if x == "logs.json")
        with open(f) as fh:
            return json.load(fh)

    for site in ("local0", "local1"):
        on, off = logs("on", site), logs("off", site)
        assert on.get("eval_feed") == "device" and "eval_feed" not in off
        for k in KEYS:
            assert on[k] == off[k], (site, k)
