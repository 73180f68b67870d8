"""Global-norm gradient clipping of the fused Adam (``FusedAdam(max_grad_norm=c)``): CPU path.

Semantics under test (ops.optim.FusedAdam): ``G = grad_scale * ||grad||_2`` from an fp64 sum of
squares, ``coef = grad_scale * min(1, c / (G + 1e-6))`` (``torch.nn.utils.clip_grad_norm_``), a
non-finite ``G`` skips the update but consumes a step number.
"""
import json
import os

import pytest
import torch
import torch.nn as nn

from mp_util import run_world

SCALES = (1.0, 0.02, 3.0, 0.02, 1.0, 0.02)  # pre-clip norms 20.6, 7.5, 155.1, 5.9, 19.7, 4.4
ATOL, RTOL = 1e-5, 1e-4  # test_fused_adam_matches_torch's


def _pair():
    torch.manual_seed(1)
    mods = nn.Sequential(nn.Linear(33, 17), nn.Linear(17, 5))
    ref = nn.Sequential(nn.Linear(33, 17), nn.Linear(17, 5))
    ref.load_state_dict(mods.state_dict())
    return mods, ref


def _torch_run(ref, xs, clip):
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-4)
    norms = []
    for x in xs:
        ropt.zero_grad()
        ref(x).square().sum().backward()
        if clip:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)))
        ropt.step()
    return torch.cat([p.detach().reshape(-1) for p in ref.parameters()]), norms


def _flat_values(mods):
    return torch.cat([p.detach().reshape(-1) for p in mods.parameters()])


def test_clipped_adam_matches_torch_and_differs_from_unclipped():
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    mods, ref = _pair()
    _, ref_free = _pair()
    flat = FlatParams(mods.parameters())
    opt = FusedAdam(flat, lr=1e-2, weight_decay=1e-4, max_grad_norm=10)
    xs = [torch.randn(8, 33) * s for s in SCALES]
    norms = []
    for x in xs:
        opt.zero_grad()
        mods(x).square().sum().backward()
        opt.step()
        norms.append(float(opt.grad_norm))
    want, tnorms = _torch_run(ref, xs, 10)
    print("grad norms", norms, "torch", tnorms)
    assert sum(n > 10 for n in tnorms) == 3 and sum(n < 10 for n in tnorms) == 3
    for a, b in zip(norms, tnorms):
        assert abs(a - b) <= ATOL + RTOL * abs(b), (a, b)
    got = _flat_values(mods)
    assert torch.allclose(got, want, atol=ATOL, rtol=RTOL)
    assert int(opt.skipped_steps) == 0 and opt.step_count == 6
    # negative control: Adam is nearly invariant to a uniform gradient scale, so agreement alone
    # could hide a clip that is not applied -- the unclipped run must be far away
    free, _ = _torch_run(ref_free, xs, None)
    far = (got - free).abs() > 10 * (ATOL + RTOL * free.abs())
    print("fraction of elements away from the unclipped run", float(far.float().mean()))
    assert far.float().mean() >= 0.9


def _small(max_grad_norm=None, seed=3):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    torch.manual_seed(seed)
    m = nn.Sequential(nn.Linear(7, 5), nn.Linear(5, 3))
    flat = FlatParams(m.parameters())
    return m, flat, FusedAdam(flat, lr=1e-2, weight_decay=1e-4, max_grad_norm=max_grad_norm)


def _backward(m, opt, seed):
    g = torch.Generator().manual_seed(seed)
    opt.zero_grad()
    m(torch.randn(6, 7, generator=g)).square().sum().backward()


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_skips_the_update(bad):
    m, flat, opt = _small(max_grad_norm=1.0)
    _backward(m, opt, 0)
    opt.step()
    before = [t.clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)]
    _backward(m, opt, 1)
    flat.grad[5] = bad
    opt.step()
    for t, b in zip((flat.data, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(t, b)
    assert int(opt.skipped_steps) == 1 and opt.step_count == 2
    assert not torch.isfinite(opt.grad_norm)
    _backward(m, opt, 2)
    opt.step()
    assert int(opt.skipped_steps) == 1 and opt.step_count == 3
    assert torch.isfinite(flat.data).all() and not torch.equal(flat.data, before[0])
    assert torch.isfinite(opt.grad_norm)


def test_threshold_not_reached_is_bit_identical_to_unclipped():
    m1, f1, o1 = _small(max_grad_norm=1e30)
    m2, f2, o2 = _small(max_grad_norm=None)
    assert o2.max_grad_norm is None and o2.grad_norm is None and o2.skipped_steps is None
    for s in range(5):
        _backward(m1, o1, s)
        _backward(m2, o2, s)
        o1.step(grad_scale=0.5)
        o2.step(grad_scale=0.5)
    assert torch.equal(f1.data, f2.data)
    assert torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
    assert float(o1.grad_norm) > 0


def test_reference_adam_clips_like_the_optimizer():
    from dinunet_implementations_amd.ops import reference as ref
    m, flat, opt = _small(max_grad_norm=0.5)
    p, ea, es = flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    for s in range(3):
        _backward(m, opt, s)
        ref.adam_(p, flat.grad.clone(), ea, es, s + 1, 1e-2, weight_decay=1e-4, max_grad_norm=0.5)
        opt.step()
        assert float(opt.grad_norm) > 0.5
    assert torch.allclose(flat.data, p, atol=1e-7, rtol=1e-6)


def test_state_dict_round_trip_and_old_checkpoints():
    m, flat, opt = _small(max_grad_norm=2.5)
    _backward(m, opt, 0)
    flat.grad[0] = float("inf")
    opt.step()
    sd = opt.state_dict()
    assert sd["max_grad_norm"] == 2.5 and sd["skipped"] == 1
    _, _, other = _small(max_grad_norm=7.0, seed=4)
    other.load_state_dict(sd)
    assert other.max_grad_norm == 2.5 and int(other.skipped_steps) == 1
    assert other.step_count == 1
    old = {k: v for k, v in sd.items() if k not in ("max_grad_norm", "skipped")}
    _, _, third = _small(max_grad_norm=7.0, seed=4)
    third.load_state_dict(old)
    assert third.max_grad_norm == 7.0 and int(third.skipped_steps) == 0
    # an optimizer without clipping saves what it saved before, and loads either kind
    _, _, off = _small()
    assert "max_grad_norm" not in off.state_dict() and "skipped" not in off.state_dict()
    off.load_state_dict(sd)
    assert off.max_grad_norm is None


def test_threshold_setter_and_on_off_is_fixed():
    _, _, opt = _small(max_grad_norm=1.0)
    opt.max_grad_norm = 3.0
    assert opt.max_grad_norm == 3.0 and float(opt._clip_f[0]) == 3.0
    with pytest.raises(ValueError):
        opt.max_grad_norm = None
    with pytest.raises(ValueError):
        opt.max_grad_norm = -2.0
    _, _, off = _small()
    with pytest.raises(ValueError):
        off.max_grad_norm = 1.0


def test_config_key(monkeypatch):
    from dinunet_implementations_amd.config import EXTRA_INPUT_KEYS, build_config, generate_compspec
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    monkeypatch.delenv("DINUNET_MAX_GRAD_NORM", raising=False)
    cfg = build_config()
    assert cfg["max_grad_norm"] == 0
    with pytest.raises(ValueError):
        build_config(overrides={"max_grad_norm": -1})
    assert build_config(overrides={"max_grad_norm": 2.0})["max_grad_norm"] == 2.0
    assert "max_grad_norm" not in EXTRA_INPUT_KEYS
    assert "max_grad_norm" not in generate_compspec()["computation"]["input"]
    flat = FlatParams(nn.Linear(3, 2).parameters())
    with pytest.raises(ValueError):
        FusedAdam(flat, max_grad_norm=-1)
    assert FusedAdam(flat).max_grad_norm is None
    assert FusedAdam(flat, max_grad_norm=cfg["max_grad_norm"]).max_grad_norm is None
    # the A/B switch is read only when the argument is None
    monkeypatch.setenv("DINUNET_MAX_GRAD_NORM", "1e30")
    assert FusedAdam(flat).max_grad_norm == 1e30
    assert FusedAdam(flat, max_grad_norm=0).max_grad_norm is None
    assert FusedAdam(flat, max_grad_norm=4.0).max_grad_norm == 4.0


def test_trainer_passes_the_threshold(monkeypatch):
    from dinunet_implementations_amd.config import build_config
    from dinunet_implementations_amd.runtime.trainer import NNTrainer
    monkeypatch.delenv("DINUNET_MAX_GRAD_NORM", raising=False)

    class _T(NNTrainer):
        def _init_nn_model(self):
            self.nn["net"] = nn.Linear(4, 2)

    for c, want in ((0, None), (1.5, 1.5)):
        cfg = build_config(overrides={"max_grad_norm": c, "gpus": []})
        t = _T(cfg)
        if getattr(t, "optimizer", None) is None:
            t.init_nn()
        assert t.optimizer.max_grad_norm == want


# ---- two gloo sites ---------------------------------------------------------------------------
SITE_SCALES = (1.0, 0.02, 3.0, 0.02)
SITE_CLIP = 0.4


def _site_model():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(12, 8), nn.Linear(8, 3))


def _site_data(rank, s):
    g = torch.Generator().manual_seed(100 + 10 * rank + s)
    return torch.randn(10, 12, generator=g) * SITE_SCALES[s]


def w_clipped_sites(grp, clip):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    m = _site_model()
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-2, max_grad_norm=clip)
    eng = make_engine("dSGD", m, flat, grp, {})
    norms = []
    for s in range(len(SITE_SCALES)):
        flat.zero_grad()
        with eng.step_context():
            m(_site_data(grp.rank, s)).square().mean().backward()
        opt.step(grad_scale=eng.reduce())
        norms.append(float(opt.grad_norm) if clip else 0.0)
    return flat.data.clone(), norms


def _single_process(clip):
    """Both sites' gradients summed in one process, the mean (scale 1/2) clipped."""
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    m = _site_model()
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-2, max_grad_norm=clip)
    for s in range(len(SITE_SCALES)):
        flat.zero_grad()
        for r in range(2):
            m(_site_data(r, s)).square().mean().backward()
        opt.step(grad_scale=0.5)
    return flat.data.clone()


def test_two_gloo_sites_clip_the_mean_gradient_identically():
    outs = run_world(w_clipped_sites, 2, SITE_CLIP)
    (p0, n0), (p1, n1) = outs
    print("site grad norms", n0)
    assert torch.equal(p0, p1) and n0 == n1
    assert any(n > SITE_CLIP for n in n0) and any(n < SITE_CLIP for n in n0)
    # fp32 sums of two sites' gradients in either order are the same bits; the tolerance only
    # covers an engine that scales its buckets before adding them
    assert torch.allclose(p0, _single_process(SITE_CLIP), atol=1e-6, rtol=1e-5)
    # and the clip was applied: the unclipped computation ends somewhere else
    assert not torch.allclose(p0, _single_process(None), atol=1e-4, rtol=1e-3)


# ---- the runtimes get it from the optimizer: site loop and COINSTAC nodes ------------------------
def w_fs_site(grp, data_path, out, overrides):
    from dinunet_implementations_amd.config import build_config, load_inputspec
    from dinunet_implementations_amd.runtime.site import FederatedSite
    from dinunet_implementations_amd.tasks import get_task
    specs = load_inputspec(os.path.join(data_path, "inputspec.json"))
    cfg = build_config(site_input=specs[grp.rank], overrides=overrides)
    state = {"baseDirectory": os.path.join(data_path, "input", f"local{grp.rank}", "simulatorRun")}
    T, D, H = get_task(cfg["task_id"])
    logs = FederatedSite(cfg, grp, T, D, H, state, out, verbose=False).run()
    return [{k: v for k, v in l.items() if k in ("replica_check", "grad_norm", "skipped_steps")}
            for l in logs]


@pytest.mark.parametrize("clip", [0.05, 0])
def test_site_loop_clips_and_logs_the_norm(fs_data_root, tmp_path, monkeypatch, clip):
    monkeypatch.delenv("DINUNET_MAX_GRAD_NORM", raising=False)
    out = str(tmp_path)
    res = run_world(w_fs_site, 2, fs_data_root, out,
                    {"epochs": 2, "check_replicas": True, "max_grad_norm": clip})
    assert all(res[0][0]["replica_check"])
    with open(os.path.join(out, "local0", "FS-Classification", "fold_0", "logs.json")) as f:
        logs = json.load(f)
    if not clip:  # logs.json as before
        assert "grad_norm" not in logs and "skipped_steps" not in logs
        return
    assert len(logs["grad_norm"]) == 2 and logs["skipped_steps"] == [0, 0]
    assert all(g > clip for g in logs["grad_norm"])  # the threshold was in force
    assert res[0][0]["grad_norm"] == res[1][0]["grad_norm"]  # the same mean gradient on both


def test_coinstac_nodes_clip(fs_data_root, tmp_path, monkeypatch):
    from dinunet_implementations_amd.compat.nodes import LocalNode, RemoteNode
    from dinunet_implementations_amd.compat.simulator import simulate
    monkeypatch.delenv("DINUNET_MAX_GRAD_NORM", raising=False)
    it, locs, rem = simulate(fs_data_root, str(tmp_path), lambda: LocalNode(device="cpu"), RemoteNode,
                             overrides={"epochs": 1, "max_grad_norm": 0.05})
    opts = [locs[s].trainer.optimizer for s in sorted(locs)]
    assert all(o.max_grad_norm == 0.05 and o.step_count > 0 for o in opts)
    assert all(float(o.grad_norm) > 0.05 and int(o.skipped_steps) == 0 for o in opts)
    assert all(float(o.grad_norm) == float(opts[0].grad_norm) for o in opts)
    ws = [locs[s].trainer.flat.data for s in sorted(locs)]
    assert all(torch.equal(w, ws[0]) for w in ws)
