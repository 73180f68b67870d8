"""Federated averaging with local steps (``agg_engine: fedAvg``) on the CPU: the torch path of
``ops.fedavg`` against the numpy mirror ``tests/fedavg_ref.py`` bit for bit, the site weights, the
configuration keys, the refusals, the file-transport pieces against ``round()``, two gloo sites
against a one-process simulation that steps two trainers separately and combines them with the
mirror, the round cadence of the site loop, and an exact resume with server momentum."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import fedavg_ref as fr
from mp_util import run_world

W_ODD = float(np.float32(1.3))


def _flat(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return SimpleNamespace(data=torch.randn(n, generator=g), grad=torch.zeros(n))


# ---- the torch path against the mirror -----------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 2053])
@pytest.mark.parametrize("eta", [1.0, 0.5])
@pytest.mark.parametrize("beta", [0.0, 0.9])
@pytest.mark.parametrize("w", [1.0, W_ODD])
def test_torch_path_equals_the_mirror_bit_for_bit(n, eta, beta, w):
    from dinunet_implementations_amd.ops import FedAvgState
    flat = _flat(n, seed=n)
    st = FedAvgState(flat, beta)
    assert (st.u is None) == (beta == 0.0)
    st.begin()
    a = flat.data.numpy().copy()
    u = np.zeros(n, dtype=np.float32) if beta > 0 else None
    g = torch.Generator().manual_seed(7)
    for rnd in range(3):  # the momentum and the moved anchor enter the later rounds
        flat.data.add_(torch.randn(n, generator=g) * 0.01 * (rnd + 1))
        p = flat.data.numpy().copy()
        d, drift = fr.delta(p, a, w)
        got_d = st.delta(w)
        assert fr.same_bits(got_d.numpy(), d)
        m = d  # a world of one: the mean is the site's own delta
        a, p2, u, g0 = fr.adopt(m, a, u, eta, beta)
        st.adopt(eta)
        assert fr.same_bits(st.anchor.numpy(), a) and fr.same_bits(flat.data.numpy(), p2)
        assert fr.same_bits(flat.grad.numpy(), g0) and not flat.grad.any()
        if beta > 0:
            assert fr.same_bits(st.u.numpy(), u)
        assert float(st.drift) == pytest.approx(drift, rel=1e-12, abs=0)


def test_non_finite_parameters_pass_through():
    from dinunet_implementations_amd.ops import FedAvgState
    flat = _flat(8)
    st = FedAvgState(flat, 0.0)
    st.begin()
    flat.data[1], flat.data[2], flat.data[3] = float("nan"), float("inf"), float("-inf")
    d = st.delta(1.0).clone()
    assert torch.isnan(d[1]) and d[2] == float("inf") and d[3] == float("-inf")
    st.adopt(1.0)
    p = flat.data
    assert torch.isnan(p[1]) and p[2] == float("inf") and p[3] == float("-inf")
    assert torch.isfinite(p[[0, 4, 5, 6, 7]]).all()


def test_state_refuses_bad_buffers():
    from dinunet_implementations_amd.ops import FedAvgState
    with pytest.raises(ValueError, match="FedAvgState"):
        FedAvgState(SimpleNamespace(data=torch.zeros(4), grad=torch.zeros(5)))
    with pytest.raises(ValueError, match="FedAvgState"):
        FedAvgState(SimpleNamespace(data=torch.zeros(4).double(), grad=torch.zeros(4)))
    with pytest.raises(ValueError, match="momentum"):
        FedAvgState(_flat(4), 1.0)
    st = FedAvgState(_flat(4), 0.5)
    with pytest.raises(ValueError, match="momentum buffer"):
        st.load_state_dict({"u": torch.zeros(5)})


# ---- site weights -----------------------------------------------------------------------------------
def test_samples_weights():
    from dinunet_implementations_amd.ops.fedavg import site_weights
    sizes = (3, 5, 8)
    got = site_weights(sizes)
    want = [np.float32(3 * n / 16) for n in sizes]
    assert [np.float32(v) for v in got] == want == fr.site_weights(sizes)
    assert all(isinstance(v, float) and float(np.float32(v)) == v for v in got)
    # equal deltas: the weighted mean gives the delta back to within 1 ulp
    g = torch.Generator().manual_seed(3)
    d = (torch.randn(4096, generator=g) * 0.01).numpy()
    m = fr.mean_site_order([d * np.float32(w) for w in got])
    ulp = np.spacing(np.abs(d))
    assert np.all(np.abs(m.astype(np.float64) - d.astype(np.float64)) <= ulp)
    # sizes such as (1, 2) give weights that are not fp32 numbers before rounding
    assert fr.site_weights((1, 2)) == [np.float32(2 / 3), np.float32(4 / 3)]
    assert [np.float32(v) for v in site_weights((1, 2))] == fr.site_weights((1, 2))
    with pytest.raises(ValueError, match="samples"):
        site_weights((0, 0))


# ---- configuration --------------------------------------------------------------------------------
def test_config_keys_and_refusals():
    from dinunet_implementations_amd.config import (AGG_ENGINES, build_config, generate_compspec,
                                                    load_compspec)
    assert "fedAvg" in AGG_ENGINES
    cfg = build_config(overrides={"agg_engine": "fedAvg"})
    assert (cfg["fedavg_local_steps"], cfg["fedavg_weighting"], cfg["fedavg_server_lr"],
            cfg["fedavg_server_momentum"]) == (4, "uniform", 1.0, 0.0)
    ok = build_config(overrides={"agg_engine": "fedAvg", "fedavg_local_steps": 1,
                                 "fedavg_weighting": "samples", "fedavg_server_lr": 0.5,
                                 "fedavg_server_momentum": 0.9})
    assert ok["fedavg_local_steps"] == 1 and ok["fedavg_weighting"] == "samples"
    bad = {"fedavg_local_steps": (0, -1, 2.0, True, "4"),
           "fedavg_weighting": ("mean", 1, True),
           "fedavg_server_lr": (0, -1.0, float("inf"), float("nan"), True, "1"),
           "fedavg_server_momentum": (1.0, -0.1, 2, True, "0.9", float("nan"))}
    for key, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=f"{key} must"):
                build_config(overrides={key: v})
    for spec in (generate_compspec(), load_compspec()):
        inputs = spec["computation"]["input"]
        assert "fedAvg" in inputs["agg_engine"]["values"]
        for key in bad:
            assert key not in inputs
            assert all(key not in (v.get("default") or {}) for v in inputs.values()
                       if isinstance(v.get("default"), dict))
    assert generate_compspec() == load_compspec()


# ---- engine ------------------------------------------------------------------------------------------
def _fs_model():
    from dinunet_implementations_amd.models.fs import MSANNet
    torch.manual_seed(0)
    return MSANNet(66, [64, 32], 2)


def test_engine_refusals(monkeypatch):
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import ENGINES, FedAvgEngine, make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    for k in ("DINUNET_DP_CLIP_NORM", "DINUNET_SECURE_AGG", "DINUNET_EMA_DECAY"):
        monkeypatch.delenv(k, raising=False)
    m = _fs_model()
    flat = FlatParams(m.parameters())
    assert ENGINES["fedAvg"] is FedAvgEngine and FedAvgEngine.name == "fedAvg"
    assert not FedAvgEngine.supports_dp and not FedAvgEngine.supports_secure_agg
    assert FedAvgEngine.releases == "parameter differences, not a gradient"
    with pytest.raises(ValueError, match="dp_clip_norm.*parameter differences"):
        make_engine("fedAvg", m, flat, SiteGroup(), {"dp_clip_norm": 1.0})
    with pytest.raises(ValueError, match="secure_agg.*parameter differences"):
        make_engine("fedAvg", m, flat, SiteGroup(), {"secure_agg": True})
    with pytest.raises(ValueError, match="ema_decay.*differ between the sites"):
        make_engine("fedAvg", m, flat, SiteGroup(), {"ema_decay": 0.9})
    with pytest.raises(ValueError, match="GPUs per site"):
        make_engine("fedAvg", m, flat, SiteGroup(rank=0, world=4, replicas=2), {})
    for key, v in (("fedavg_local_steps", 0), ("fedavg_weighting", "mean"),
                   ("fedavg_server_lr", 0), ("fedavg_server_momentum", 1.0)):
        with pytest.raises(ValueError, match=key):
            make_engine("fedAvg", m, flat, SiteGroup(), {key: v})
    eng = make_engine("fedAvg", m, flat, SiteGroup(), {})
    assert eng.local.name == "dSGD" and not eng.local.group.distributed and not eng.local.overlap
    assert (eng.local_steps, eng.weighting, eng.eta, eng.beta) == (4, "uniform", 1.0, 0.0)
    assert [u for u in range(1, 11) if eng.round_due(u, 10)] == [4, 8, 10]
    samples = make_engine("fedAvg", m, flat, SiteGroup(), {"fedavg_weighting": "samples"})
    with pytest.raises(RuntimeError, match="set_samples"):
        samples.round()
    samples.set_samples(17)
    assert samples.weight == 1.0  # one site: W n / n


def test_coinstac_nodes_refuse_fedavg(fs_data_root, tmp_path):
    from dinunet_implementations_amd.compat.nodes import LocalNode, RemoteNode
    from dinunet_implementations_amd.compat.simulator import simulate
    with pytest.raises(ValueError, match="fedAvg.*in-process runtime"):
        simulate(fs_data_root, str(tmp_path), lambda: LocalNode(device="cpu"), RemoteNode,
                 overrides={"agg_engine": "fedAvg", "epochs": 1})


def _engine(cfg):
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    m = _fs_model()
    flat = FlatParams(m.parameters())
    eng = make_engine("fedAvg", m, flat, SiteGroup(), cfg)
    eng.begin()
    return eng, flat


@pytest.mark.parametrize("beta", [0.0, 0.9])
def test_file_transport_pieces_equal_round_on_a_world_of_one(beta):
    from dinunet_implementations_amd.parallel import FedAvgEngine
    cfg = {"fedavg_server_lr": 0.5, "fedavg_server_momentum": beta}
    (a, fa), (b, fb) = _engine(cfg), _engine(cfg)
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        step = torch.randn(fa.data.numel(), generator=g) * 0.01
        fa.data.add_(step)
        fb.data.add_(step)
        a.round()
        pay = b.payload()
        assert set(pay) == {"delta"} and not fb.grad.any()
        b.apply(FedAvgEngine.aggregate([pay], cfg))
        assert fr.same_bits(fa.data.numpy(), fb.data.numpy())
        assert fr.same_bits(a.state.anchor.numpy(), b.state.anchor.numpy())
        assert not fa.grad.any() and not fb.grad.any()
        if beta:
            assert fr.same_bits(a.state.u.numpy(), b.state.u.numpy())
    assert a.rounds == b.rounds == 2 and a.drift == b.drift > 0
    # three sites: the fp32 sum in site order times 1/W
    ds = [torch.randn(9, generator=g) for _ in range(3)]
    agg = FedAvgEngine.aggregate([{"delta": d} for d in ds])
    assert fr.same_bits(agg["delta"].numpy(), fr.mean_site_order([d.numpy() for d in ds]))


def test_state_dict_round_trip():
    cfg = {"fedavg_server_momentum": 0.9}
    (a, fa), (b, fb) = _engine(cfg), _engine(cfg)
    fa.data.add_(0.01)
    a.round()
    sd = a.state_dict()
    assert sd["rounds"] == 1 and torch.equal(sd["u"], a.state.u)
    fb.data.copy_(fa.data)
    b.load_state_dict(sd)
    b.begin()  # after a resume: the restored momentum stays
    assert torch.equal(b.state.u, a.state.u) and b.rounds == 1
    assert torch.equal(b.state.anchor, a.state.anchor)
    b.begin()  # a fresh phase: zero again
    assert not b.state.u.any()
    assert _engine({})[0].state_dict() == {"rounds": 0}


# ---- two gloo sites against a one-process simulation ----------------------------------------------------
K_LOCAL, STEPS, EPOCHS = 3, 4, 2
FED_CFG = {"fedavg_local_steps": K_LOCAL, "fedavg_server_lr": 0.5, "fedavg_server_momentum": 0.9}


def _batch(rank, upd):
    g = torch.Generator().manual_seed(1000 * rank + upd)
    return torch.randn(16, 66, generator=g), torch.randint(0, 2, (16,), generator=g)


def _trainer():
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    m = _fs_model().train()
    flat = FlatParams(m.parameters())
    return m, flat, FusedAdam(flat, lr=1e-2)


def _update(m, flat, opt, rank, upd, scale=1.0):
    x, y = _batch(rank, upd)
    flat.zero_grad()
    _, loss, _ = m.forward_loss(x, y)
    loss.backward()
    opt.step(grad_scale=scale)


def w_fedavg(grp, cfg):
    from dinunet_implementations_amd.parallel import make_engine
    m, flat, opt = _trainer()
    eng = make_engine("fedAvg", m, flat, grp, cfg)
    eng.begin()
    rec, total = [], 0
    for _ in range(EPOCHS):
        for upd in range(1, STEPS + 1):
            total += 1
            _update(m, flat, opt, grp.rank, total, eng.local.reduce())
            if eng.round_due(upd, STEPS):
                pre = flat.data.clone()
                eng.round()
                rec.append((total, pre, flat.data.clone(), eng.drift, bool(flat.grad.any())))
    return rec, opt.exp_avg.clone(), eng.rounds, eng.comm_bytes, eng.state.u.clone()


def test_two_gloo_sites_equal_the_simulation():
    outs = run_world(w_fedavg, 2, FED_CFG)
    recs = [o[0] for o in outs]
    assert [r[0] for r in recs[0]] == [r[0] for r in recs[1]] == [3, 4, 7, 8]
    threads = torch.get_num_threads()
    torch.set_num_threads(2)  # as the site processes
    try:
        sites = [_trainer() for _ in range(2)]
        a = sites[0][1].data.numpy().copy()
        us = [np.zeros_like(a), np.zeros_like(a)]
        total, k = 0, 0
        for _ in range(EPOCHS):
            for upd in range(1, STEPS + 1):
                total += 1
                for r, (m, flat, opt) in enumerate(sites):
                    _update(m, flat, opt, r, total)
                if upd % K_LOCAL and upd != STEPS:
                    continue
                ps = [s[1].data.numpy().copy() for s in sites]
                a, us, _, drifts = fr.round_(ps, a, us, eta=0.5, beta=0.9)
                for r, (m, flat, opt) in enumerate(sites):
                    at, pre, post, drift, dirty = recs[r][k]
                    assert at == total and not dirty
                    assert fr.same_bits(pre.numpy(), ps[r]), (k, r)
                    assert fr.same_bits(post.numpy(), a), (k, r)
                    assert drift == pytest.approx(drifts[r], rel=1e-12)
                    flat.data.copy_(torch.from_numpy(a))
                assert torch.equal(recs[0][k][2], recs[1][k][2])  # one model on both sites
                k += 1
    finally:
        torch.set_num_threads(threads)
    assert k == 4
    n = sites[0][1].data.numel()
    for r in range(2):
        assert outs[r][2] == 4 and outs[r][3] == 4 * 4 * n  # rounds; fp32 wire bytes, added up
        assert fr.same_bits(outs[r][4].numpy(), us[r])
        assert fr.same_bits(outs[r][1].numpy(), sites[r][2].exp_avg.numpy())
    assert not torch.equal(outs[0][1], outs[1][1])  # Adam's moments stayed local to a site


# ---- the site loop ------------------------------------------------------------------------------------
FS_OVERRIDES = {"agg_engine": "fedAvg", "hidden_sizes": [64, 32], "batch_size": 14,
                "patience": 100, "seed": 3, "check_replicas": True}


def w_fed_site(grp, data_path, out, overrides):
    from dinunet_implementations_amd.ops import FusedAdam
    from dinunet_implementations_amd.parallel import FedAvgEngine
    from test_runtime_e2e import w_site
    seen = {"updates": 0, "rounds": []}
    step, rnd = FusedAdam.step, FedAvgEngine.round

    def counting_step(self, *a, **k):
        seen["updates"] += 1
        return step(self, *a, **k)

    def recording_round(self):
        rnd(self)
        seen["rounds"].append((seen["updates"], self.flat.data.clone(), bool(self.flat.grad.any())))
    FusedAdam.step, FedAvgEngine.round = counting_step, recording_round
    try:
        res = w_site(grp, data_path, out, overrides)
    finally:
        FusedAdam.step, FedAvgEngine.round = step, rnd
    return res, seen["rounds"]


def _logs(out, site):
    with open(os.path.join(out, site, "FS-Classification", "fold_0", "logs.json")) as f:
        return json.load(f)


def test_site_loop_rounds_after_every_kth_and_the_last_update(fs_data_root, tmp_path):
    out = str(tmp_path)
    res = run_world(w_fed_site, 2, fs_data_root, out,
                    dict(FS_OVERRIDES, epochs=2, fedavg_local_steps=3))
    rounds = [r[1] for r in res]
    assert [u for u, _, _ in rounds[0]] == [u for u, _, _ in rounds[1]] == [3, 4, 7, 8]
    for (_, p0, d0), (_, p1, d1) in zip(*rounds):
        assert torch.equal(p0, p1) and not d0 and not d1
    for r in range(2):
        assert all(res[r][0][0]["replica_check"])
        logs = _logs(out, f"local{r}")
        assert logs["fedavg_rounds"] == [2, 2] and len(logs["fedavg_drift"]) == 2
        assert all(v > 0 for v in logs["fedavg_drift"])
        assert (logs["fedavg_local_steps"], logs["fedavg_weighting"], logs["fedavg_server_lr"],
                logs["fedavg_server_momentum"]) == (3, "uniform", 1.0, 0.0)
    assert res[0][0][0]["test_metrics"] == res[1][0][0]["test_metrics"]
    drifts = [_logs(out, f"local{r}")["fedavg_drift"] for r in range(2)]
    assert drifts[0] != drifts[1]  # each site's own
    # other engines log none of it
    other = str(tmp_path / "dsgd")
    run_world(w_fed_site, 2, fs_data_root, other, dict(FS_OVERRIDES, agg_engine="dSGD", epochs=1))
    assert not [k for k in _logs(other, "local0") if k.startswith("fedavg")]


def test_site_loop_samples_weighting_keeps_one_model(fs_data_root, tmp_path):
    out = str(tmp_path)
    res = run_world(w_fed_site, 2, fs_data_root, out,
                    dict(FS_OVERRIDES, epochs=1, fedavg_weighting="samples"))
    for (_, p0, _), (_, p1, _) in zip(res[0][1], res[1][1]):
        assert torch.equal(p0, p1)
    assert all(res[0][0][0]["replica_check"]) and _logs(out, "local0")["fedavg_rounds"] == [1]


def test_resume_with_server_momentum_bitwise(fs_data_root, tmp_path):
    from test_resume import _check_same
    from test_runtime_e2e import w_site
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    base = dict(FS_OVERRIDES, fedavg_local_steps=3, fedavg_server_momentum=0.9,
                fedavg_server_lr=0.5)
    run_world(w_site, 2, fs_data_root, a, dict(base, epochs=2))
    run_world(w_site, 2, fs_data_root, b, dict(base, epochs=1))
    run_world(w_site, 2, fs_data_root, b, dict(base, epochs=2, resume=True))
    _check_same(a, b, "FS-Classification")
    for site in ("local0", "local1"):
        la, lb = _logs(a, site), _logs(b, site)
        assert la["fedavg_rounds"] == lb["fedavg_rounds"] == [2, 2]
        assert la["fedavg_drift"] == lb["fedavg_drift"]
