"""Class-weighted / label-smoothed loss, CPU side: the oracle in ``ops.reference``, config
validation, the models' CPU branches, ``class_weights="balanced"`` across gloo sites
(``runtime.site``), checkpoints and the COINSTAC phase machines."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from mp_util import run_world

W = {2: [0.3, 2.5], 3: [0.5, 1.0, 3.0], 5: [0.2, 0.7, 1.0, 1.9, 3.0]}


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    monkeypatch.delenv("DINUNET_CLASS_WEIGHTS", raising=False)
    monkeypatch.delenv("DINUNET_LABEL_SMOOTHING", raising=False)


# ---- the oracle and the closed form the kernels implement ---------------------------------------
def _closed_form(z, y, w, eps):
    """loss and d loss / d z of the closed form in csrc/kernels/loss_opt.h, in fp64."""
    z, w = z.double(), w.double()
    B, C = z.shape
    p = torch.softmax(z, 1)
    logp = torch.log_softmax(z, 1)
    wy = w[y]
    D = wy.sum()
    onehot = F.one_hot(y, C).double()
    loss = ((1 - eps) * wy * -(logp * onehot).sum(1) + (eps / C) * (-(logp * w).sum(1))).sum() / D
    g = (p * ((1 - eps) * wy + (eps / C) * w.sum())[:, None] - (1 - eps) * wy[:, None] * onehot
         - (eps / C) * w[None, :]) / D
    return loss, g


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("C", [2, 3, 5])
@pytest.mark.parametrize("fs", [False, True])
def test_reference_heads_equal_torch_and_the_closed_form(C, eps, fs):
    from dinunet_implementations_amd.ops import reference as ref
    g = torch.Generator().manual_seed(C)
    z = torch.randn(11, C, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.randint(0, C, (11,), generator=g)
    w = torch.tensor(W[C], dtype=torch.float64)
    out, loss, pred = (ref.log_softmax_nll if fs else ref.softmax_ce)(z, y, w, eps)
    loss.backward()
    zt = z.detach().clone().requires_grad_()
    lt = F.cross_entropy(zt, y, weight=w, label_smoothing=eps)
    lt.backward()
    assert torch.equal(loss, lt) and torch.equal(z.grad, zt.grad)
    want = torch.log_softmax(zt, 1) if fs else torch.softmax(zt, 1)
    assert torch.equal(out, want.detach()) and torch.equal(pred, want.argmax(1))
    lc, gc = _closed_form(z.detach(), y, w, eps)
    assert abs(float(lc) - float(lt.detach())) < 1e-12
    assert (gc - zt.grad).abs().max() < 1e-12
    # ops.heads takes the same arguments and is the oracle on CPU
    from dinunet_implementations_amd import ops
    _, l2, _ = (ops.log_softmax_nll if fs else ops.softmax_ce)(z.detach(), y, weight=W[C],
                                                               label_smoothing=eps)
    assert abs(float(l2) - float(lt.detach())) < 1e-12


def test_defaults_are_the_plain_loss():
    from dinunet_implementations_amd.ops import reference as ref
    z = torch.randn(7, 2)
    y = torch.randint(0, 2, (7,))
    assert torch.equal(ref.softmax_ce(z, y)[1], F.cross_entropy(z, y))
    assert torch.equal(ref.log_softmax_nll(z, y)[1], F.nll_loss(F.log_softmax(z, 1), y))


def test_loss_block_layout():
    from dinunet_implementations_amd.ops.heads import LOSS_W0, loss_block_values
    blk = loss_block_values([0.5, 1.0, 3.0], 0.1, 3)
    assert blk.dtype == torch.float32 and blk.numel() == LOSS_W0 + 16
    e = torch.tensor(0.1 / 3, dtype=torch.float32)
    assert blk[0] == torch.tensor(0.9) and blk[1] == e and blk[3] == torch.tensor(0.1)
    assert blk[2] == e * torch.tensor(4.5)
    assert blk[LOSS_W0:LOSS_W0 + 3].tolist() == [0.5, 1.0, 3.0] and blk[LOSS_W0 + 3:].sum() == 0
    ones = loss_block_values(None, 0.0, 2)  # the values that make the kernels' on path exact
    assert ones[:LOSS_W0 + 2].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 1.0]
    assert loss_block_values(None, 0.0, 40).numel() == LOSS_W0 + 40
    with pytest.raises(ValueError):
        loss_block_values([1.0], 0.0, 2)


# ---- configuration -----------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [[1.0], [1.0, 2.0, 3.0], [0, 1], [-1.0, 1.0], [float("nan"), 1.0],
                                 [float("inf"), 1.0], [True, 1.0], "inverse", 2.0, ["a", "b"]])
def test_config_refuses_bad_class_weights(bad):
    from dinunet_implementations_amd.config import build_config
    with pytest.raises(ValueError) as e:
        build_config(overrides={"class_weights": bad})
    assert "class_weights" in str(e.value)


@pytest.mark.parametrize("bad", [1.0, -0.1, True, "0.1", float("nan")])
def test_config_refuses_bad_label_smoothing(bad):
    from dinunet_implementations_amd.config import build_config
    with pytest.raises(ValueError) as e:
        build_config(overrides={"label_smoothing": bad})
    assert "label_smoothing" in str(e.value)


def test_config_defaults_and_good_values():
    from dinunet_implementations_amd.config import (EXTRA_INPUT_KEYS, build_config,
                                                    generate_compspec)
    cfg = build_config()
    assert cfg["class_weights"] is None and cfg["label_smoothing"] == 0
    got = build_config(overrides={"class_weights": [1, 2.5], "label_smoothing": 0.1})
    assert got["class_weights"] == [1.0, 2.5] and got["label_smoothing"] == 0.1
    assert build_config(overrides={"class_weights": "balanced"})["class_weights"] == "balanced"
    three = build_config(overrides={"num_class": 3, "class_weights": [1, 2, 3]})
    assert three["class_weights"] == [1.0, 2.0, 3.0]
    # every other key is as before, and the GUI contract does not grow
    assert {k: v for k, v in got.items() if k not in ("class_weights", "label_smoothing")} == \
        {k: v for k, v in cfg.items() if k not in ("class_weights", "label_smoothing")}
    assert "class_weights" not in EXTRA_INPUT_KEYS and "label_smoothing" not in EXTRA_INPUT_KEYS
    inputs = generate_compspec()["computation"]["input"]
    assert "class_weights" not in inputs and "label_smoothing" not in inputs


def test_environment_switches_apply_only_where_unset(monkeypatch):
    from dinunet_implementations_amd.models import MSANNet
    monkeypatch.setenv("DINUNET_CLASS_WEIGHTS", "1,4")
    monkeypatch.setenv("DINUNET_LABEL_SMOOTHING", "0.2")
    spec = MSANNet(6, [4], 2).head_spec()
    assert spec.loss_on and spec.class_weights == [1.0, 4.0] and spec.label_smoothing == 0.2
    spec = MSANNet(6, [4], 2, class_weights=[2.0, 1.0], label_smoothing=0.1).head_spec()
    assert spec.class_weights == [2.0, 1.0] and spec.label_smoothing == 0.1
    monkeypatch.setenv("DINUNET_CLASS_WEIGHTS", "1,x")
    with pytest.raises(ValueError):
        MSANNet(6, [4], 2).head_spec()


# ---- the models' CPU branches ------------------------------------------------------------------
def test_models_honour_the_options_on_cpu():
    from dinunet_implementations_amd.models import ICALstm, MSANNet
    torch.manual_seed(0)
    w = torch.tensor(W[2])
    kw = dict(input_size=16, hidden_size=32, num_comps=6, window_size=5)
    plain, ica = ICALstm(**kw), ICALstm(class_weights=W[2], label_smoothing=0.1, **kw)
    assert set(ica.state_dict()) == set(plain.state_dict())
    ica.load_state_dict(plain.state_dict())
    ica.eval()
    x = torch.randn(9, 4, 6, 5)
    y = torch.randint(0, 2, (9,))
    out, loss, pred = ica.forward_loss(x, y)
    logits, _ = ica(x)
    assert torch.allclose(loss, F.cross_entropy(logits, y, weight=w, label_smoothing=0.1))
    assert torch.equal(out, torch.softmax(logits, 1))
    # body_loss / proj-free halves use the same objective
    _, l2, _ = ica.body_loss(ica.stem(x), y)
    assert torch.equal(l2, loss)

    fplain = MSANNet(66, [16, 8], 3)
    fs = MSANNet(66, [16, 8], 3, class_weights=W[3], label_smoothing=0.1)
    assert set(fs.state_dict()) == set(fplain.state_dict())
    xf, yf = torch.rand(10, 66), torch.randint(0, 3, (10,))
    out, loss, pred = fs.forward_loss(xf, yf)
    z = fs(xf)
    assert torch.allclose(loss, F.cross_entropy(z, yf, weight=torch.tensor(W[3]),
                                                label_smoothing=0.1))
    assert torch.equal(out, torch.log_softmax(z, 1))
    # set_loss: new values in place; refused when the options were off at construction
    fs.set_loss([1.0, 1.0, 1.0], 0.0)
    assert torch.allclose(fs.forward_loss(xf, yf)[1], F.cross_entropy(z, yf))
    with pytest.raises(RuntimeError):
        fplain.set_loss([1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        MSANNet(66, [16], 2, class_weights=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        ICALstm(label_smoothing=1.0, **kw)


# ---- "balanced" across sites -------------------------------------------------------------------
def _write_site(root, site, labels, seed):
    """One FS site in the simulator layout: a covariate CSV and one aseg-stats file per subject."""
    base = os.path.join(root, "input", f"local{site}", "simulatorRun")
    os.makedirs(base, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    with open(os.path.join(base, "site_covariates.csv"), "w") as f:
        f.write("freesurferfile,isControl\n")
        for i, lab in enumerate(labels):
            name = f"subject{site}_{i}_aseg_stats.txt"
            f.write(f"{name},{'True' if lab else 'False'}\n")
            vals = torch.rand(66, generator=g) * 1000 + (300.0 if lab else 0.0)
            with open(os.path.join(base, name), "w") as s:
                s.write(f"Measure:volume\tsubject{site}_{i}\n")
                for j, v in enumerate(vals.tolist()):
                    s.write(f"region{j}\t{v:.4f}\n")
    return base


def _make_cohort(root, ratios):
    """``ratios``: per site (controls, patients)."""
    for site, (n1, n0) in enumerate(ratios):
        _write_site(root, site, [1] * n1 + [0] * n0, seed=site)
    return root


def w_balanced(grp, root, out, overrides):
    from dinunet_implementations_amd.config import build_config
    from dinunet_implementations_amd.runtime.site import FederatedSite
    from dinunet_implementations_amd.tasks import get_task
    cfg = build_config(overrides=dict({"task_id": "FS-Classification", "batch_size": 8,
                                       "split_ratio": [0.7, 0.15, 0.15], "patience": 100,
                                       "hidden_sizes": [16, 8]}, **overrides))
    state = {"baseDirectory": os.path.join(root, "input", f"local{grp.site}", "simulatorRun")}
    T, D, H = get_task(cfg["task_id"])
    counts = []

    class Site(FederatedSite):  # records this rank's own training label counts
        def _datasets(self, split):
            data = super()._datasets(split)
            counts.append(torch.bincount(data["train"][1].cpu(), minlength=2).tolist())
            return data

    logs = Site(cfg, grp, T, D, H, state, out, verbose=False).run()
    return [{"class_weights": l.get("class_weights"), "label_smoothing": l.get("label_smoothing"),
             "test_metrics": l.get("test_metrics"), "counts": c} for l, c in zip(logs, counts)]


RATIOS = [(30, 10), (8, 24)]  # site 0: 3:1 controls, site 1: 1:3


def _expected(res):
    n = [sum(r[0]["counts"][c] for r in res) for c in (0, 1)]
    return [sum(n) / (2 * c) for c in n]


def test_balanced_weights_from_the_pooled_counts(tmp_path):
    root = _make_cohort(str(tmp_path / "data"), RATIOS)
    res = run_world(w_balanced, 2, root, str(tmp_path / "one"),
                    {"epochs": 1, "class_weights": "balanced", "label_smoothing": 0.1})
    assert res[0][0]["counts"] != res[1][0]["counts"]  # the sites' ratios differ
    want = _expected(res)
    for r in res:
        assert r[0]["class_weights"] == pytest.approx(want, rel=1e-12)
        assert r[0]["label_smoothing"] == 0.1
    assert res[0][0]["class_weights"] == res[1][0]["class_weights"]
    # two replicas per site: the same weights (their shards are disjoint and cover the sites)
    rep = run_world(w_balanced, 4, root, str(tmp_path / "rep"),
                    {"epochs": 1, "class_weights": "balanced", "label_smoothing": 0.1},
                    replicas=2)
    for r in rep:
        assert r[0]["class_weights"] == res[0][0]["class_weights"]
    # off: the keys are absent from logs.json
    off = run_world(w_balanced, 2, root, str(tmp_path / "off"), {"epochs": 1})
    assert off[0][0]["class_weights"] is None and off[0][0]["label_smoothing"] is None
    with open(os.path.join(str(tmp_path / "off"), "local0", "FS-Classification", "fold_0",
                           "logs.json")) as f:
        logs = json.load(f)
    assert "class_weights" not in logs and "label_smoothing" not in logs


def test_balanced_raises_everywhere_when_a_class_is_missing(tmp_path):
    root = _make_cohort(str(tmp_path / "data"), [(20, 0), (24, 0)])
    with pytest.raises(AssertionError) as e:
        run_world(w_balanced, 2, root, str(tmp_path / "out"),
                  {"epochs": 1, "class_weights": "balanced"})
    msg = str(e.value)
    assert "rank 0 failed" in msg and "rank 1 failed" in msg
    assert msg.count("class_weights='balanced'") >= 2


def test_checkpoint_carries_the_resolved_options(tmp_path):
    """A resume continues with the saved weights and eps, and ``mode: test`` from the checkpoint
    reports the training run's test loss, both without the keys in the configuration."""
    root = _make_cohort(str(tmp_path / "data"), RATIOS)
    out = str(tmp_path / "out")
    first = run_world(w_balanced, 2, root, out, {"epochs": 2, "class_weights": "balanced",
                                                 "label_smoothing": 0.1, "seed": 3})
    w = first[0][0]["class_weights"]
    ck = torch.load(os.path.join(out, "local0", "FS-Classification", "fold_0",
                                 "checkpoint_last.pt"), weights_only=True)
    assert ck["loss_options"] == {"class_weights": w, "label_smoothing": 0.1}
    assert not any("loss" in k or "class_weight" in k for k in ck["models"]["fs_net"])
    again = run_world(w_balanced, 2, root, out, {"epochs": 3, "resume": True, "seed": 3})
    for r in again:
        assert r[0]["class_weights"] == w and r[0]["label_smoothing"] == 0.1
    test = run_world(w_balanced, 2, root, out, {"mode": "test", "seed": 3})
    for r, a in zip(test, again):
        assert r[0]["class_weights"] == w and r[0]["label_smoothing"] == 0.1
        assert r[0]["test_metrics"] == a[0]["test_metrics"]
    # the objective matters to that number: the same checkpoint without it reports another loss
    plain = run_world(w_plain_test, 2, root, out, {"mode": "test", "seed": 3})
    assert plain[0][0]["test_metrics"][0] != test[0][0]["test_metrics"][0]


def w_plain_test(grp, root, out, overrides):
    """``mode: test`` on checkpoints whose loss options are stripped."""
    fdir = os.path.join(out, f"local{grp.site}", "FS-Classification", "fold_0")
    path = os.path.join(fdir, "checkpoint_best.pt")
    ck = torch.load(path, weights_only=True)
    ck.pop("loss_options", None)
    stripped = os.path.join(fdir, "checkpoint_plain.pt")
    torch.save(ck, stripped)
    return w_balanced(grp, root, out + "_plain", dict(overrides, pretrained_path=stripped))


# ---- COINSTAC phase machines -------------------------------------------------------------------
def test_coinstac_nodes_take_the_list_and_refuse_balanced(fs_data_root, tmp_path):
    from dinunet_implementations_amd.compat.nodes import LocalNode, RemoteNode
    from dinunet_implementations_amd.compat.simulator import simulate
    it, locs, rem = simulate(fs_data_root, str(tmp_path / "a"), lambda: LocalNode(device="cpu"),
                             RemoteNode, overrides={"epochs": 1, "class_weights": [0.3, 2.5],
                                                    "label_smoothing": 0.1})
    for s in locs:
        assert locs[s].trainer.loss_options() == {"class_weights": [0.3, 2.5],
                                                  "label_smoothing": 0.1}
        assert locs[s].trainer.optimizer.step_count > 0
    with pytest.raises(ValueError) as e:
        simulate(fs_data_root, str(tmp_path / "b"), lambda: LocalNode(device="cpu"), RemoteNode,
                 overrides={"epochs": 1, "class_weights": "balanced"})
    assert "in-process runtime" in str(e.value)
