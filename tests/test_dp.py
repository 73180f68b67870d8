"""Differentially private gradient release, CPU side: the Philox known answers and the statistics
of the fp64 mirror in ``ops.reference``, the accountant (``parallel.privacy``), config validation,
engine gating, the state round trip, dSGD over two gloo sites and the site loop's logs."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from mp_util import run_world


# ---- generator --------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    from dinunet_implementations_amd.ops.reference import philox4x32_10
    got = " ".join(f"{int(v):08x}" for v in philox4x32_10(counter, key))
    assert got == want


N = 2 ** 20


@pytest.fixture(scope="module")
def draws():
    """The mirror's release of a zero gradient at sigma c = 1 (the noise itself): the reference
    draw, the next release and the next stream.  Computed once."""
    from dinunet_implementations_amd.ops.reference import dp_privatize
    zero = torch.zeros(N)
    out = {k: dp_privatize(zero, 1.0, 1.0, 1234, s, t).numpy()
           for k, (s, t) in {"ref": (0, 1), "t2": (0, 2), "s1": (1, 1)}.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def test_mirror_statistics(draws):
    z = draws["ref"]
    n = z.size
    m, v = z.mean(), z.var()
    kurt = ((z - m) ** 4).mean() / v ** 2
    stats = {
        "mean": m * math.sqrt(n),
        "variance": (v - 1.0) / math.sqrt(2.0 / n),
        "kurtosis": (kurt - 3.0) / math.sqrt(24.0 / n),
        "lag1": _corr(z[:-1], z[1:]) * math.sqrt(n),
        "lag2": _corr(z[:-2], z[2:]) * math.sqrt(n),
        "next release": _corr(z, draws["t2"]) * math.sqrt(n),
        "next stream": _corr(z, draws["s1"]) * math.sqrt(n),
    }
    print(stats, "max |z|", float(np.abs(z).max()))
    for k, s in stats.items():
        assert abs(s) < 5, (k, s)
    # 24-bit uniforms: the tail ends at sqrt(2 * 24 ln 2) = 5.77
    assert np.abs(z).max() <= math.sqrt(48 * math.log(2.0)) + 1e-12


def test_mirror_clips_and_scales(draws):
    from dinunet_implementations_amd.ops.reference import dp_coef, dp_noise, dp_privatize
    g = torch.randn(1028, generator=torch.Generator().manual_seed(3))
    coef, G = dp_coef(g, 2.0)
    assert G > 2.0 and coef == float(torch.tensor(2.0 / (G + 1e-6), dtype=torch.float32))
    assert dp_coef(g * (1.0 / G), 2.0)[0] == 1.0
    out = dp_privatize(g, 2.0, 0.5, 1234, 0, 1)
    z = dp_noise(1028, 1234, 0, 1)
    assert torch.equal(z, torch.from_numpy(draws["ref"][:1028].copy()))  # counter = float4 index
    assert torch.allclose(out, coef * g.double() + 1.0 * z, rtol=0, atol=1e-15)
    assert torch.equal(dp_privatize(g, 2.0, 0.0, 1, 2, 3), coef * g.double())
    g[7] = float("inf")
    assert bool(torch.isnan(dp_privatize(g, 2.0, 0.5, 1234, 0, 1)).all())


# ---- accountant -------------------------------------------------------------------------------
def test_accountant():
    from dinunet_implementations_amd.parallel import privacy
    for T, sigma, delta in ((1, 1.0, 1e-5), (1000, 4.0, 1e-6), (37, 0.5, 1e-3)):
        r = 2.0 * T / sigma ** 2
        assert privacy.rho(T, sigma) == pytest.approx(r, rel=1e-15)
        assert privacy.epsilon(T, sigma, delta) == pytest.approx(
            r + 2.0 * math.sqrt(r * math.log(1.0 / delta)), rel=1e-14)
    eps = [privacy.epsilon(T, 2.0, 1e-5) for T in range(0, 50)]
    assert eps[0] == 0.0 and all(b > a for a, b in zip(eps, eps[1:]))
    # rho adds across two phases (their own multipliers); epsilon comes from the total
    r = privacy.rho(30, 2.0) + privacy.rho(70, 2.0)
    assert r == pytest.approx(privacy.rho(100, 2.0), rel=1e-15)
    assert privacy.epsilon_of_rho(r, 1e-5) == pytest.approx(privacy.epsilon(100, 2.0, 1e-5))
    mixed = privacy.rho(30, 1.0) + privacy.rho(70, 2.0)
    assert mixed == pytest.approx(60.0 + 35.0)
    assert privacy.epsilon(10, 0.0, 1e-5) == math.inf and privacy.loggable(math.inf) is None
    assert privacy.epsilon(0, 0.0, 1e-5) == 0.0
    for bad in (0.0, 1.0, -1.0):
        with pytest.raises(ValueError):
            privacy.epsilon(1, 1.0, bad)


# ---- configuration ----------------------------------------------------------------------------
def test_config_validation():
    from dinunet_implementations_amd.config import REFERENCE_INPUT_KEYS, build_config
    cfg = build_config()
    assert cfg["dp_clip_norm"] == 0 and cfg["dp_noise_multiplier"] == 0
    assert cfg["dp_delta"] == 1e-5 and cfg["dp_seed"] is None
    assert not any(k.startswith("dp_") for k in REFERENCE_INPUT_KEYS)
    ok = build_config(overrides={"dp_clip_norm": 1.5, "dp_noise_multiplier": 0.7, "dp_delta": 1e-6,
                                 "dp_seed": 5})
    assert (ok["dp_clip_norm"], ok["dp_noise_multiplier"], ok["dp_delta"], ok["dp_seed"]) == \
        (1.5, 0.7, 1e-6, 5)
    for bad in ({"dp_noise_multiplier": 1.0},                      # noise without clip
                {"dp_clip_norm": -1.0}, {"dp_clip_norm": 1.0, "dp_noise_multiplier": -0.1},
                {"dp_clip_norm": float("inf")}, {"dp_clip_norm": float("nan")},
                {"dp_clip_norm": "1"}, {"dp_clip_norm": True},
                {"dp_clip_norm": 1.0, "dp_delta": 0.0}, {"dp_clip_norm": 1.0, "dp_delta": 1.0},
                {"dp_clip_norm": 1.0, "dp_delta": -1e-5}, {"dp_seed": -1}, {"dp_seed": 1.5},
                {"pretrain_args": {"dp_noise_multiplier": 1.0}},  # the phase's own keys
                {"dp_clip_norm": 1.0, "pretrain_args": {"dp_clip_norm": -2.0}}):
        with pytest.raises(ValueError):
            build_config(overrides=bad)
    build_config(overrides={"dp_clip_norm": 1.0, "dp_noise_multiplier": 1.0,
                            "pretrain_args": {"dp_noise_multiplier": 2.0}})


# ---- engines ----------------------------------------------------------------------------------
def _model(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(33, 17), nn.ReLU(), nn.Linear(17, 5))


def _engine(name, cfg, group=None):
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    m = _model()
    flat = FlatParams(m.parameters())
    return m, flat, make_engine(name, m, flat, group or SiteGroup(), {"precision_bits": "32", **cfg})


ON = {"dp_clip_norm": 0.5, "dp_noise_multiplier": 0.3, "dp_seed": 21}


def test_engine_gating(monkeypatch):
    monkeypatch.delenv("DINUNET_DP_CLIP_NORM", raising=False)
    monkeypatch.delenv("DINUNET_DP_NOISE", raising=False)
    for name in ("rankDAD", "powerSGD"):
        with pytest.raises(ValueError, match="dSGD only"):
            _engine(name, ON)
        assert _engine(name, {})[2].dp is None
    _, _, off = _engine("dSGD", {})
    assert off.dp is None and off.state_dict() == {}  # nothing allocated, the present path
    _, _, eng = _engine("dSGD", dict(ON, dp_fold=3, dp_phase=1, dp_rank=5))
    assert eng.dp is not None and eng.dp.stream == 3 * 4096 + 2048 + 5 and eng.dp.seed == 21
    assert (eng.dp.clip_norm, eng.dp.noise_multiplier) == (0.5, 0.3)
    assert not eng.prefers_split and not eng.overlap
    with pytest.raises(RuntimeError, match="file transport"):
        eng.payload()  # the file transport would ship the gradient as computed
    with pytest.raises(ValueError, match="stream word"):
        _engine("dSGD", dict(ON, dp_rank=2048))
    with pytest.raises(ValueError, match="dp_clip_norm"):
        _engine("dSGD", {"dp_noise_multiplier": 1.0})
    # the switches apply where the keys are unset
    monkeypatch.setenv("DINUNET_DP_CLIP_NORM", "2")
    monkeypatch.setenv("DINUNET_DP_NOISE", "1.5")
    _, _, env = _engine("dSGD", {})
    assert (env.dp.clip_norm, env.dp.noise_multiplier) == (2.0, 1.5)
    assert _engine("dSGD", ON)[2].dp.clip_norm == 0.5
    with pytest.raises(ValueError, match="dSGD only"):
        _engine("powerSGD", {})


def test_one_site_reduce_privatises_first():
    from dinunet_implementations_amd.ops import reference
    _, flat, eng = _engine("dSGD", ON)
    g = torch.randn(flat.numel, generator=torch.Generator().manual_seed(1)) * 0.2
    flat.grad.copy_(g)
    assert eng.reduce() == 1.0
    want = reference.dp_privatize(g, 0.5, 0.3, 21, 0, 1).float()
    assert torch.equal(flat.grad, want) and not torch.equal(flat.grad, g)
    assert eng.dp.releases == 1 and eng.dp.clipped == 1
    assert eng.dp.last_norm == pytest.approx(float(torch.linalg.vector_norm(g.double())), rel=1e-6)


def test_coinstac_phase_machines_refuse(fs_data_root, tmp_path, monkeypatch):
    from dinunet_implementations_amd.compat.nodes import LocalNode, RemoteNode
    from dinunet_implementations_amd.compat.simulator import simulate
    monkeypatch.delenv("DINUNET_DP_CLIP_NORM", raising=False)
    for i, ov in enumerate(({"dp_clip_norm": 1.0}, {"pretrain_args": {"dp_clip_norm": 1.0}})):
        with pytest.raises(ValueError, match="in-process runtime"):
            simulate(fs_data_root, str(tmp_path / str(i)), lambda: LocalNode(device="cpu"),
                     RemoteNode, overrides=dict(ov, epochs=1))


# ---- state ------------------------------------------------------------------------------------
def test_state_round_trip_continues_the_counter():
    from dinunet_implementations_amd.ops import DPState, reference
    g = torch.randn(260, generator=torch.Generator().manual_seed(2)) * 0.01  # G < c: coef 1
    a = DPState("cpu", 1.0, 0.5, seed=(9 << 32) + 4, stream=4097)
    outs = []
    for _ in range(2):
        x = g.clone()
        a.privatize_(x)
        outs.append(x)
    sd = json.loads(json.dumps(a.state_dict()))  # plain values
    assert sd["t"] == 2 and sd["seed"] == (9 << 32) + 4 and sd["stream"] == 4097
    b = DPState("cpu", 1.0, 0.5, seed=0, stream=0)
    b.load_state_dict(sd)
    x = g.clone()
    b.privatize_(x)
    assert b.releases == 3 and (b.seed, b.stream) == (a.seed, a.stream)
    assert torch.equal(x, reference.dp_privatize(g, 1.0, 0.5, a.seed, a.stream, 3).float())
    for prev in outs:  # no repeated draw
        assert float((x - prev).abs().max()) > 0.1
    # through the engine
    _, flat, e1 = _engine("dSGD", ON)
    flat.grad.normal_()
    e1.reduce()
    e1.reduce()
    _, flat2, e2 = _engine("dSGD", dict(ON, dp_seed=99))
    e2.load_state_dict(e1.state_dict())
    assert e2.dp.releases == 2 and e2.dp.seed == 21 and e2.dp.clipped == e1.dp.clipped
    _, _, off = _engine("dSGD", {})
    off.load_state_dict(e1.state_dict())  # (a run resumed with the option off ignores it)
    assert off.dp is None


def test_host_words_and_refusals(monkeypatch):
    from dinunet_implementations_amd.ops import DPState
    d = DPState("cpu", 1.0, 0.0)
    g = torch.full((8,), 0.1)
    d.privatize_(g)
    assert torch.equal(g, torch.full((8,), 0.1))  # sigma 0, G <= c: bit for bit
    d.noise_multiplier = 2.0
    d.clip_norm = 0.25
    assert float(d._f[0]) == 0.25 and float(d._f[1]) == 2.0
    for bad in (-1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError):
            d.noise_multiplier = bad
        with pytest.raises(ValueError):
            d.clip_norm = bad
    with pytest.raises(ValueError):
        d.clip_norm = 0.0
    with pytest.raises(ValueError):
        d.privatize_(torch.zeros(6))
    with pytest.raises(ValueError):
        DPState("cpu", 1.0, 0.0, stream=2 ** 32)


# ---- two gloo sites ---------------------------------------------------------------------------
def w_dsgd_sites(grp, cfg):
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    m = _model()
    flat = FlatParams(m.parameters())
    eng = make_engine("dSGD", m, flat, grp, {"precision_bits": "32", "dsgd_bucket_mb": 0.001, **cfg})
    own = torch.randn(flat.numel, generator=torch.Generator().manual_seed(100 + grp.rank)) * 0.1
    flat.grad.copy_(own)
    eng.launch_bucket(0)  # ready before reduce(): nothing may leave yet
    early = (len(eng._handles), eng.early_launches, bool(torch.equal(flat.grad, own)))
    scale = eng.reduce()
    return {"own": own, "applied": flat.grad * scale, "stream": eng.dp.stream, "early": early,
            "buckets": len(eng.buckets), "prefers_split": eng.prefers_split,
            "overlap": eng.overlap, "releases": eng.dp.releases, "comm_bytes": eng.comm_bytes}


def test_two_gloo_sites_release_the_mirrored_gradients():
    from dinunet_implementations_amd.ops import reference
    res = run_world(w_dsgd_sites, 2, dict(ON, dp_fold=2))
    want = None
    for r, out in enumerate(res):
        assert out["stream"] == 2 * 4096 + r and out["releases"] == 1
        assert out["buckets"] > 1 and out["early"] == (0, 0, True)
        assert out["prefers_split"] is False and out["overlap"] is False
        assert out["comm_bytes"] == out["own"].numel() * 4
        rel = reference.dp_privatize(out["own"], 0.5, 0.3, 21, out["stream"], 1).float()
        want = rel if want is None else want + rel
    want = want * 0.5
    for out in res:  # (fp32 sum of two releases in either order, then the 1 / world scale)
        assert torch.allclose(out["applied"], want, rtol=0, atol=1e-7)
    assert torch.equal(res[0]["applied"], res[1]["applied"])
    # the releases differ between the sites (their own streams) and from the raw gradients
    raw = 0.5 * (res[0]["own"] + res[1]["own"])
    assert float((res[0]["applied"] - raw).abs().max()) > 0.05


# ---- the site loop ----------------------------------------------------------------------------
def w_fs_site(grp, data_path, out, overrides):
    from dinunet_implementations_amd.config import build_config, load_inputspec
    from dinunet_implementations_amd.runtime.site import FederatedSite
    from dinunet_implementations_amd.tasks import get_task
    specs = load_inputspec(os.path.join(data_path, "inputspec.json"))
    cfg = build_config(site_input=specs[grp.rank], overrides=overrides)
    state = {"baseDirectory": os.path.join(data_path, "input", f"local{grp.rank}", "simulatorRun")}
    T, D, H = get_task(cfg["task_id"])
    logs = FederatedSite(cfg, grp, T, D, H, state, out, verbose=False).run()
    return [{k: v for k, v in l.items() if k.startswith("dp") or k.startswith("pretrain_dp")
             or k in ("replica_check", "pretrain_site")} for l in logs]


def test_site_loop_logs_the_guarantee(fs_data_root, tmp_path, monkeypatch):
    from dinunet_implementations_amd.parallel import privacy
    monkeypatch.delenv("DINUNET_DP_CLIP_NORM", raising=False)
    monkeypatch.delenv("DINUNET_DP_NOISE", raising=False)
    out = str(tmp_path)
    res = run_world(w_fs_site, 2, fs_data_root, out, {
        "epochs": 2, "check_replicas": True, "dp_clip_norm": 0.05, "dp_noise_multiplier": 1.5,
        "dp_delta": 1e-6, "pretrain": True,
        "pretrain_args": {"epochs": 1, "dp_noise_multiplier": 3.0}})
    src = int(res[0][0]["pretrain_site"][len("local"):])
    for r in range(2):
        l = res[r][0]
        assert all(l["replica_check"])  # the same mean of the two releases on both sites
        with open(os.path.join(out, f"local{r}", "FS-Classification", "fold_0", "logs.json")) as f:
            logs = json.load(f)
        dp = logs["dp"]
        assert dp["clip_norm"] == 0.05 and dp["noise_multiplier"] == 1.5 and dp["delta"] == 1e-6
        assert dp["adjacency"] == "replace-one-subject" and dp["nonfinite"] == 0
        assert len(logs["dp_epsilon"]) == len(logs["dp_grad_norm"]) == 2
        assert all(g > 0 for g in logs["dp_grad_norm"])
        rho = 0.0
        fed = dp["releases"]
        if r == src:  # its pretraining releases count too, at that phase's multiplier
            pre = logs["dp_pretrain"]
            assert pre["noise_multiplier"] == 3.0 and pre["releases"] > 0
            assert len(logs["pretrain_dp_epsilon"]) == 1
            assert logs["pretrain_dp_epsilon"][0] == pytest.approx(
                privacy.epsilon(pre["releases"], 3.0, 1e-6))
            rho += privacy.rho(pre["releases"], 3.0)
            fed -= pre["releases"]
        else:
            assert "dp_pretrain" not in logs
        assert fed > 0 and fed % 2 == 0
        rho += privacy.rho(fed, 1.5)
        assert dp["epsilon"] == pytest.approx(privacy.epsilon_of_rho(rho, 1e-6))
        assert logs["dp_epsilon"][-1] == pytest.approx(dp["epsilon"])
        assert logs["dp_epsilon"][0] < logs["dp_epsilon"][1]
    # both sites took the same number of federated releases
    assert (res[0][0]["dp"]["releases"] - res[0][0].get("dp_pretrain", {}).get("releases", 0)
            == res[1][0]["dp"]["releases"] - res[1][0].get("dp_pretrain", {}).get("releases", 0))


def test_site_loop_off_logs_nothing(fs_data_root, tmp_path, monkeypatch):
    monkeypatch.delenv("DINUNET_DP_CLIP_NORM", raising=False)
    res = run_world(w_fs_site, 2, fs_data_root, str(tmp_path), {"epochs": 1})
    assert all(not any(k.startswith("dp") for k in l[0]) for l in res)
