"""Device-fed evaluation, the parts that need no GPU: the batch partition, the two configuration
keys, the FS refusal of a different evaluation batch size, and the host fallback of a CPU site."""
import os

import pytest
import torch


@pytest.mark.parametrize("bs", [1, 2, 8])
def test_partition_is_the_unshuffled_loaders(bs):
    from dinunet_implementations_amd.data.loader import DeviceLoader
    from dinunet_implementations_amd.runtime.evalfeed import eval_partition, eval_spans
    for n in range(1, 41):
        dl = DeviceLoader(torch.zeros(n, 3), torch.zeros(n, dtype=torch.long), bs, shuffle=False,
                          drop_last=False, merge_singleton=True)
        want = [(s, e) for s, e, _ in dl._spans()]
        assert eval_spans(n, bs) == want, (n, bs)
        full, tail = eval_partition(n, bs)
        assert full == sum(e - s == bs for s, e in want)
        assert full + (1 if tail else 0) == len(want) == len(dl)
        assert tail in (0, want[-1][1] - want[-1][0]) and full * bs + tail == n


def test_partition_edges():
    from dinunet_implementations_amd.runtime.evalfeed import eval_partition
    assert eval_partition(21, 8) == (2, 5)
    assert eval_partition(17, 8) == (1, 9)    # trailing singleton merged: batch_size + 1
    assert eval_partition(8, 8) == (1, 0)
    assert eval_partition(5, 8) == (0, 5)     # fewer rows than a batch: one short batch
    assert eval_partition(9, 8) == (0, 9)
    assert eval_partition(0, 8) == (0, 0)


def _cfg(**ov):
    from dinunet_implementations_amd.config import build_config
    return build_config(overrides=ov)


def test_validate_accepts_and_rejects_the_keys():
    c = _cfg()
    assert c["device_eval"] is False and c["eval_batch_size"] is None
    assert _cfg(device_eval=True)["device_eval"] is True
    assert _cfg(device_eval=None)["device_eval"] is False
    assert _cfg(eval_batch_size=256)["eval_batch_size"] == 256
    for bad in (1, "yes", 0.5):
        with pytest.raises(ValueError, match="device_eval"):
            _cfg(device_eval=bad)
    for bad in (0, -4, 2.5, "32", True):
        with pytest.raises(ValueError, match="eval_batch_size"):
            _cfg(eval_batch_size=bad)
    # framework keys: not inputs of the generated compspec
    from dinunet_implementations_amd.config import generate_compspec
    inputs = generate_compspec()["computation"]["input"]
    assert "device_eval" not in inputs and "eval_batch_size" not in inputs


def test_fs_refuses_another_eval_batch_size():
    from dinunet_implementations_amd.runtime.site import check_eval_batch_size
    from dinunet_implementations_amd.tasks import get_task
    cfg = _cfg(task_id="FS-Classification", batch_size=16, eval_batch_size=64)
    T, _, _ = get_task(cfg["task_id"])
    tr = T(cache=cfg, state={}, device="cpu")
    tr.init_nn(seed=0)
    with pytest.raises(ValueError, match="batch statistics"):
        check_eval_batch_size(cfg, tr)
    check_eval_batch_size(dict(cfg, eval_batch_size=16), tr)    # the same size: fine
    check_eval_batch_size(dict(cfg, eval_batch_size=None), tr)
    # LayerNorm does not couple rows
    cfg2 = _cfg(task_id="FS-Classification", batch_size=16, eval_batch_size=64, norm_layer="layer")
    tr2 = T(cache=cfg2, state={}, device="cpu")
    tr2.init_nn(seed=0)
    check_eval_batch_size(cfg2, tr2)
    # ICA: BatchNorm with running statistics
    ica = _cfg(task_id="ICA-Classification", batch_size=8, eval_batch_size=64, num_components=4,
               window_size=5, temporal_size=20, input_size=8, hidden_size=8)
    Ti, _, _ = get_task(ica["task_id"])
    ti = Ti(cache=ica, state={}, device="cpu")
    ti.init_nn(seed=0)
    check_eval_batch_size(ica, ti)


def _run_cpu_site(root, out, overrides, capsys=None):
    from dinunet_implementations_amd.config import build_config, load_inputspec
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.site import FederatedSite
    from dinunet_implementations_amd.tasks import get_task
    specs = load_inputspec(os.path.join(root, "inputspec.json"))
    cfg = build_config(site_input=specs[0], overrides=overrides)
    state = {"baseDirectory": os.path.join(root, "input", "local0", "simulatorRun")}
    T, D, H = get_task(cfg["task_id"])
    grp = SiteGroup(device=torch.device("cpu"))
    return FederatedSite(cfg, grp, T, D, H, state, out, verbose=True).run()[0]


KEYS = ("train_log", "validation_log", "local_validation_log", "test_metrics", "best_val_epoch",
        "local_test_metrics", "test_scores")


def test_cpu_site_with_device_eval_takes_the_host_loop(fs_data_root, tmp_path, capsys):
    ov = {"epochs": 2, "batch_size": 16, "seed": 1}
    on = _run_cpu_site(fs_data_root, str(tmp_path / "on"), dict(ov, device_eval=True))
    said = capsys.readouterr().out
    off = _run_cpu_site(fs_data_root, str(tmp_path / "off"), dict(ov, device_eval=False))
    assert said.count("device_eval off") == 1 and "not on a GPU" in said  # logged once
    assert "device_eval off" not in capsys.readouterr().out
    assert "eval_feed" not in on and "eval_feed" not in off
    for k in KEYS:
        assert on[k] == off[k], k


def test_cpu_site_env_switch_and_eval_batch_size(fs_data_root, tmp_path, capsys, monkeypatch):
    """``DINUNET_DEVICE_EVAL=1`` stands in for an unset key; ``eval_batch_size`` sets the batch of
    the validation and test loaders on the host path (a LayerNorm FS model: rows independent, so
    the scores do not move -- the loss average only by its summation order)."""
    ov = {"epochs": 2, "batch_size": 16, "seed": 1, "norm_layer": "layer"}
    monkeypatch.setenv("DINUNET_DEVICE_EVAL", "1")
    a = _run_cpu_site(fs_data_root, str(tmp_path / "a"), ov)
    assert "device_eval off" in capsys.readouterr().out
    monkeypatch.delenv("DINUNET_DEVICE_EVAL")
    b = _run_cpu_site(fs_data_root, str(tmp_path / "b"), dict(ov, eval_batch_size=5))
    assert "device_eval off" not in capsys.readouterr().out
    assert a["train_log"] == b["train_log"]
    assert a["test_scores"] == b["test_scores"]
    for x, y in zip(a["validation_log"], b["validation_log"]):
        assert abs(x[0] - y[0]) < 1e-5 and x[1] == y[1]
    with pytest.raises(ValueError, match="batch statistics"):
        _run_cpu_site(fs_data_root, str(tmp_path / "c"),
                      {"epochs": 1, "batch_size": 16, "eval_batch_size": 8})
