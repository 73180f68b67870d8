"""A tiny ICA site run with the weight average on (``ema_decay``): what it logs and checkpoints,
that the logged validation is the evaluation of the checkpointed average, that the feeds and the
evaluation paths agree, that a resume continues the same average, and that a run with the
average off writes none of it."""
import json
import os

import pytest
import torch

from test_eval_site_gpu import KEYS, _twins
from test_runtime_gpu import _ica_root, _run_site

pytestmark = pytest.mark.gpu

TASK = "ICA-Classification"
# test_ica_site_logs_the_scheduled_rate_device_fed_and_host_fed's sizes, 2 epochs
OV = {"epochs": 2, "batch_size": 8, "seed": 3, "ema_decay": 0.9}

_RUNS = {}


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("DINUNET_EMA_DECAY", raising=False)
    monkeypatch.delenv("DINUNET_DEVICE_EVAL", raising=False)


@pytest.fixture
def runs(tmp_path_factory):
    """ONE device-fed and ONE host-fed run, made by the first test that asks."""
    if not _RUNS:
        tmp = tmp_path_factory.mktemp("ema_site")
        root = _ica_root(tmp)
        _RUNS.update(root=root, tmp=tmp)
        for name, fed in (("dev", True), ("host", False)):
            out = str(tmp / name)
            _RUNS[name] = (_run_site(root, out, dict(OV, device_feed=fed))[0], out)
    return _RUNS


def _fold(out):
    return os.path.join(out, "local0", TASK, "fold_0")


def _ckpt(out, name):
    return torch.load(os.path.join(_fold(out), name), map_location="cpu", weights_only=True)


def _json_logs(out):
    with open(os.path.join(_fold(out), "logs.json")) as f:
        return json.load(f)


def _mirror():
    import torch.nn as nn
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    return FusedAdam(FlatParams([nn.Parameter(torch.zeros(4))]), ema_decay=OV["ema_decay"])


def test_logs_and_checkpoints_carry_the_average(runs):
    logs, out = runs["dev"]
    assert logs.get("feed") == "device"
    on_disk = _json_logs(out)
    steps = logs["split_sizes"]["train"] // 8
    mirror = _mirror()
    want = [float(torch.tensor(mirror.ema_decay_at(e * steps), dtype=torch.float32)) for e in (1, 2)]
    for lg in (logs, on_disk):
        assert lg["ema_decay"] == 0.9
        assert lg["ema_applied_decay"] == want
    from dinunet_implementations_amd.config import build_config
    from dinunet_implementations_amd.tasks import get_task
    from dinunet_implementations_amd.config import load_inputspec
    cfg = build_config(site_input=load_inputspec(os.path.join(runs["root"], "inputspec.json"))[0],
                       overrides=OV)
    T, _, _ = get_task(TASK)
    tr = T(cache=cfg, state={}, device=torch.device("cpu"))
    tr.init_nn()
    for name in ("checkpoint_best.pt", "checkpoint_last.pt"):
        ck = _ckpt(out, name)
        assert ck["ema"].dtype == torch.float32 and ck["ema"].numel() == tr.flat.data.numel()
        # the model section: the reference's state_dict keys (the module's own), nothing more
        assert set(ck["models"]) == set(tr.nn)
        for k, net in tr.nn.items():
            assert list(ck["models"][k]) == list(net.state_dict())
        assert torch.equal(ck["optimizer"]["ema"], ck["ema"])
        assert ck["optimizer"]["ema_decay"] == 0.9 and ck["optimizer"]["ema_warmup"] is True
        # and the model section is the raw weights, not the average
        tr.load_state(ck)
        assert torch.equal(tr.optimizer.ema, ck["ema"])
        assert not torch.equal(tr.flat.data, ck["ema"])


def test_logged_validation_is_the_evaluation_of_the_checkpointed_average(runs):
    from dinunet_implementations_amd.config import build_config, load_inputspec, site_seed
    from dinunet_implementations_amd.data.splits import make_splits
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.site import FederatedSite
    from dinunet_implementations_amd.runtime.trainer import set_seed
    from dinunet_implementations_amd.tasks import get_task
    from dinunet_implementations_amd.utils.metrics import metric_value
    logs, out = runs["dev"]
    root = runs["root"]
    # a model without the average that HOLDS the checkpointed average as its weights
    cfg = build_config(site_input=load_inputspec(os.path.join(root, "inputspec.json"))[0],
                       overrides=dict(OV, ema_decay=0))
    state = {"baseDirectory": os.path.join(root, "input", "local0", "simulatorRun")}
    T, D, H = get_task(TASK)
    site = FederatedSite(cfg, SiteGroup(device=torch.device("cuda", 0)), T, D, H, state,
                         str(runs["tmp"] / "unused"), verbose=False)
    set_seed(site_seed(cfg, 0))
    files = H(cache=cfg, state=state).list_files()
    split = make_splits(files, cfg, site_seed(cfg, 0), base=state["baseDirectory"])[0]
    data = site._datasets(split)
    assert data["validation"][1].shape[0] == logs["split_sizes"]["validation"]
    va = site._loader(*data["validation"], "validation", 8, 0)
    tr = T(cache=cfg, state=state, device=torch.device("cuda", 0))
    tr.init_nn()
    assert tr.optimizer.ema is None
    ck = _ckpt(out, "checkpoint_last.pt")  # (written after the last epoch's validation)
    assert ck["epoch"] == 2
    tr.load_state(ck)
    tr.flat.data.copy_(ck["ema"].cuda())
    res = tr.evaluate(va)
    got = [round(res["averages"].average, 6), round(metric_value(res["metrics"].scores(), "auc"), 6)]
    print("manual", got, "logged", logs["local_validation_log"][-1], logs["validation_log"][-1])
    assert got == logs["local_validation_log"][-1]
    assert got[1] == logs["validation_log"][-1][1]
    # the raw weights of the same checkpoint score differently
    tr.load_state(ck)
    raw = tr.evaluate(va)
    assert round(raw["averages"].average, 6) != got[0]


def test_device_fed_and_host_fed_runs_log_equal_values(runs):
    dev, host = runs["dev"][0], runs["host"][0]
    assert dev.get("feed") == "device" and "feed" not in host
    assert dev["ema_decay"] == host["ema_decay"] == 0.9
    assert dev["ema_applied_decay"] == host["ema_applied_decay"]
    print("validation dev", dev["validation_log"], "host", host["validation_log"])
    # the two feeds train the same curve to rounding (test_device_fed_multistep_graph_matches_
    # host_fed), so the scores of the averages agree to the logs' digits or nearly
    for a, b in zip(dev["validation_log"], host["validation_log"]):
        assert a == pytest.approx(b, abs=2e-5)


def test_device_eval_on_and_off_log_equal_values(runs, tmp_path):
    on, off = _twins(runs["root"], tmp_path, dict(OV, device_feed=True))
    for k in ("ema_decay", "ema_applied_decay"):
        assert on[k] == off[k]
    for k in KEYS:  # and both equal the shared device-fed run (host evaluation)
        assert off[k] == runs["dev"][0][k], k


def test_resume_continues_a_bit_identical_average(runs, tmp_path):
    out = str(tmp_path / "resumed")
    first = _run_site(runs["root"], out, dict(OV, epochs=1, device_feed=True))[0]
    assert len(first["validation_log"]) == 1
    e1 = _ckpt(out, "checkpoint_last.pt")["ema"].clone()
    again = _run_site(runs["root"], out, dict(OV, device_feed=True, resume=True))[0]
    whole, whole_out = runs["dev"]
    a, b = _ckpt(whole_out, "checkpoint_last.pt"), _ckpt(out, "checkpoint_last.pt")
    assert a["epoch"] == b["epoch"] == 2 and a["optimizer"]["step"] == b["optimizer"]["step"]
    assert not torch.equal(b["ema"], e1)
    assert torch.equal(a["ema"], b["ema"]) and torch.equal(a["optimizer"]["ema"], b["optimizer"]["ema"])
    for name in a["models"]:
        for p in a["models"][name]:
            assert torch.equal(a["models"][name][p], b["models"][name][p]), (name, p)
    for k in ("validation_log", "ema_applied_decay", "ema_decay", "test_metrics"):
        assert again[k] == whole[k], k


def test_average_off_writes_none_of_the_new_keys(runs, tmp_path):
    out = str(tmp_path / "off")
    logs = _run_site(runs["root"], out, dict(OV, ema_decay=0, device_feed=True))[0]
    assert not [k for k in logs if "ema" in k]
    assert not [k for k in _json_logs(out) if "ema" in k]
    for name in ("checkpoint_best.pt", "checkpoint_last.pt"):
        ck = _ckpt(out, name)
        assert "ema" not in ck and not [k for k in ck["optimizer"] if "ema" in k]
    # and the average changes what is validated, not what is trained
    on = runs["dev"][0]
    assert logs["train_log"] == on["train_log"]
    assert logs["validation_log"] != on["validation_log"]
