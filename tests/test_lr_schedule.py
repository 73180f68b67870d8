"""Learning-rate schedule of the fused Adam (``FusedAdam(lr_schedule=...)``): CPU path.

Semantics under test (ops.optim.FusedAdam.lr_at, optim.hip sched_lr), from the fp32 words the
device block holds, in double, rounded to fp32 once::

    w(t) = t / W if t < W else 1
    u(t) = clamp((t - W) / (T - W), 0, 1)
    d(t) = 1 | 1 - (1 - r) u | r + (1 - r) 0.5 (1 + cos(pi u)),   r = lr_min / base
    lr(t) = fp32(((base * scale) * w) * d)

plus the reduce-on-plateau multiplier ``scale`` the site loop drives.
"""
import json
import math
import os
import struct

import pytest
import torch
import torch.nn as nn

from mp_util import run_world

ATOL, RTOL = 1e-5, 1e-4  # test_fused_adam_matches_torch's
KINDS = ("constant", "linear", "cosine")
LR = 1e-3


def f32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def closed_form(kind, t, W, T, lr=LR, lr_min=0.0, scale=1.0):
    base, lo, scale = f32(lr), f32(lr_min), f32(scale)
    w = t / W if t < W else 1.0
    u = min(max((t - W) / (T - W), 0.0), 1.0)
    r = lo / base
    d = {"constant": 1.0, "linear": 1.0 - (1.0 - r) * u,
         "cosine": r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * u))}[kind]
    return f32(base * scale * w * d)


def _opt(schedule=None, lr=LR, n=8, **kw):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    flat = FlatParams([nn.Parameter(torch.zeros(n))])
    return flat, FusedAdam(flat, lr=lr, lr_schedule=schedule, **kw)


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("DINUNET_LR_SCHEDULE", raising=False)
    monkeypatch.delenv("DINUNET_MAX_GRAD_NORM", raising=False)


# ---- the formula --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lr_at_matches_the_closed_form(kind):
    _, opt = _opt({"kind": kind, "warmup_steps": 3, "decay_steps": 10, "lr_min": 0.1 * LR})
    for t in (1, 2, 3, 4, 7, 10, 11, 1000):
        assert opt.lr_at(t) == closed_form(kind, t, 3, 10, lr_min=0.1 * LR), (kind, t)
    # warmup: thirds of the base rate, then the whole of it at t = W
    assert opt.lr_at(1) == f32(f32(LR) / 3) and opt.lr_at(3) == closed_form(kind, 3, 3, 10, lr_min=0.1 * LR)
    # after T the rate stays at its end value
    end = f32(LR) if kind == "constant" else f32(f32(LR) * (f32(0.1 * LR) / f32(LR)))
    for t in (10, 11, 1000):
        assert opt.lr_at(t) == pytest.approx(end, rel=1e-6), (kind, t)
        assert opt.lr_at(t) == opt.lr_at(10)
    if kind != "constant":  # strictly decreasing between W and T
        rates = [opt.lr_at(t) for t in range(3, 11)]
        assert all(a > b for a, b in zip(rates, rates[1:]))
    if kind == "linear":  # t = 4 is one seventh of the way from W to T
        assert opt.lr_at(4) == pytest.approx(LR * (1 - 0.9 / 7), rel=1e-6)
    if kind == "cosine":
        assert opt.lr_at(4) == pytest.approx(LR * (0.1 + 0.9 * 0.5 * (1 + math.cos(math.pi / 7))), rel=1e-6)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", [0, 1])
def test_no_warmup_and_one_step_warmup_start_at_the_full_rate(kind, W):
    _, opt = _opt({"kind": kind, "warmup_steps": W, "decay_steps": 10, "lr_min": 0.1 * LR})
    for t in (1, 2, 5, 10, 11):
        assert opt.lr_at(t) == closed_form(kind, t, W, 10, lr_min=0.1 * LR)
    # warmup factor 1 at t = 1: only the decay acts (u = 0 at W = 1, u = 0.1 at W = 0)
    if kind == "constant" or W == 1:
        assert opt.lr_at(1) == f32(LR)
    else:
        assert f32(0.9 * LR) < opt.lr_at(1) < f32(LR)


def test_scale_and_base_multiply_the_schedule():
    _, opt = _opt({"kind": "cosine", "warmup_steps": 3, "decay_steps": 10})
    opt.lr_scale = 0.5
    assert opt.lr_at(5) == closed_form("cosine", 5, 3, 10, scale=0.5)
    opt.lr = 4e-3
    assert opt.lr_at(5) == closed_form("cosine", 5, 3, 10, lr=4e-3, scale=0.5)
    _, off = _opt(None, lr=7e-4)
    assert off.lr_at(1) == off.lr_at(99) == 7e-4 and off.applied_lr is None


# ---- against torch ------------------------------------------------------------------------------
def _pair():
    torch.manual_seed(1)
    mods = nn.Sequential(nn.Linear(33, 17), nn.Linear(17, 5))
    ref = nn.Sequential(nn.Linear(33, 17), nn.Linear(17, 5))
    ref.load_state_dict(mods.state_dict())
    return mods, ref


def _fused_run(mods, xs, schedule, lr=1e-2):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    flat = FlatParams(mods.parameters())
    opt = FusedAdam(flat, lr=lr, weight_decay=1e-4, lr_schedule=schedule)
    applied = []
    for x in xs:
        opt.zero_grad()
        mods(x).square().sum().backward()
        opt.step()
        applied.append(None if opt.applied_lr is None else float(opt.applied_lr))
    return opt, torch.cat([p.detach().reshape(-1) for p in mods.parameters()]), applied


def test_scheduled_adam_matches_torch_lambda_lr_and_differs_from_unscheduled():
    mods, ref = _pair()
    free, _ = _pair()
    torch.manual_seed(2)
    xs = [torch.randn(8, 33) for _ in range(12)]
    sched = {"kind": "cosine", "warmup_steps": 3, "decay_steps": 10}
    opt, got, applied = _fused_run(mods, xs, sched)
    assert applied == [opt.lr_at(t) for t in range(1, 13)]
    ropt = torch.optim.Adam(ref.parameters(), lr=1e-2, weight_decay=1e-4)
    rs = torch.optim.lr_scheduler.LambdaLR(ropt, lambda s: opt.lr_at(s + 1) / 1e-2)
    for x in xs:
        ropt.zero_grad()
        ref(x).square().sum().backward()
        ropt.step()
        rs.step()
    want = torch.cat([p.detach().reshape(-1) for p in ref.parameters()])
    assert torch.allclose(got, want, atol=ATOL, rtol=RTOL)
    # negative control: the same run with the schedule off ends measurably elsewhere
    _, off, none = _fused_run(free, xs, None)
    assert none == [None] * 12
    far = (got - off).abs() > 10 * (ATOL + RTOL * off.abs())
    print("fraction of elements away from the unscheduled run", float(far.float().mean()))
    assert far.float().mean() >= 0.9


def test_constant_schedule_is_bit_identical_to_off():
    """The rate is an fp32 word (the kernels take the unscheduled rate as an fp32 argument too);
    the CPU path of the unscheduled optimizer keeps its Python double, so the identity on the CPU
    is for a rate fp32 holds exactly (2^-7)."""
    lr = 2.0 ** -7
    torch.manual_seed(2)
    xs = [torch.randn(8, 33) for _ in range(6)]
    a, _ = _pair()
    b, _ = _pair()
    oa, pa, applied = _fused_run(a, xs, "constant", lr=lr)
    ob, pb, _ = _fused_run(b, xs, None, lr=lr)
    assert applied == [lr] * 6
    assert torch.equal(pa, pb)
    assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)


def test_skipped_update_advances_the_schedule():
    flat, opt = _opt({"kind": "linear", "warmup_steps": 0, "decay_steps": 10}, max_grad_norm=1.0)
    for bad in (False, True, False):
        flat.grad.fill_(float("inf") if bad else 1.0)
        opt.step()
    assert int(opt.skipped_steps) == 1
    assert float(opt.applied_lr) == opt.lr_at(3) != opt.lr_at(2)


# ---- state dict, setters, validation --------------------------------------------------------------
def test_state_dict_round_trip_and_old_checkpoints():
    sched = {"kind": "cosine", "warmup_steps": 2, "decay_steps": 9, "lr_min": 1e-4}
    flat, opt = _opt(sched)
    opt.lr_scale = 0.25
    opt.plateau_wait = 2
    flat.grad.fill_(1.0)
    opt.step()
    sd = opt.state_dict()
    assert sd["lr_schedule"] == sched and sd["lr_scale"] == 0.25 and sd["plateau_wait"] == 2
    _, other = _opt({"kind": "linear", "warmup_steps": 0, "decay_steps": 50})
    other.load_state_dict(sd)
    assert other.lr_schedule.kind == "cosine" and other.lr_schedule.decay_steps == 9
    assert other.lr_scale == 0.25 and other.plateau_wait == 2 and other.step_count == 1
    assert [other.lr_at(t) for t in range(1, 12)] == [opt.lr_at(t) for t in range(1, 12)]
    # the words the update reads were rewritten, not only the host mirror
    assert float(other._lrs_f[1]) == 0.25 and int(other._lrs[5]) == 9 and int(other._lrs[3]) == 2
    # an old checkpoint keeps the built values
    old = {k: v for k, v in sd.items() if k not in ("lr_schedule", "lr_scale", "plateau_wait")}
    _, third = _opt({"kind": "linear", "warmup_steps": 0, "decay_steps": 50})
    third.load_state_dict(old)
    assert third.lr_schedule.kind == "linear" and third.lr_scale == 1.0 and third.plateau_wait == 0
    # an optimizer without a schedule saves what it saved before, and loads either kind
    _, off = _opt(None)
    assert not {"lr_schedule", "lr_scale", "plateau_wait"} & set(off.state_dict())
    off.load_state_dict(sd)
    assert off.lr_schedule is None and off.applied_lr is None and off.lr == LR


def test_setters_and_on_off_is_fixed(monkeypatch):
    _, opt = _opt({"kind": "cosine", "warmup_steps": 3, "decay_steps": 10, "lr_min": 1e-4})
    opt.lr = 2e-3
    assert opt.lr == 2e-3 and float(opt._lrs_f[0]) == f32(2e-3)
    opt.lr_scale = 0.5
    assert opt.lr_scale == 0.5 and float(opt._lrs_f[1]) == 0.5
    opt.set_decay_steps(20)
    assert opt.lr_schedule.decay_steps == 20 and int(opt._lrs[5]) == 20
    assert opt.lr_at(20) == pytest.approx(1e-4 * 0.5, rel=1e-6)
    for bad in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            opt.lr_scale = bad
    with pytest.raises(ValueError):
        opt.set_decay_steps(3)  # <= warmup
    with pytest.raises(ValueError):
        opt.lr = 1e-5  # below lr_min
    assert opt.lr == 2e-3 and opt.lr_schedule.decay_steps == 20  # refused writes changed nothing
    # off: lr is the plain host float it was, the schedule's knobs refuse
    _, off = _opt(None)
    off.lr = 5e-4
    assert off.lr == 5e-4 and off.lr_scale == 1.0
    with pytest.raises(ValueError):
        off.lr_scale = 0.5
    with pytest.raises(ValueError):
        off.set_decay_steps(10)
    # the A/B switch is read only when the argument is None
    monkeypatch.setenv("DINUNET_LR_SCHEDULE", "cosine")
    assert _opt(None)[1].lr_schedule.kind == "cosine"
    assert _opt("linear")[1].lr_schedule.kind == "linear"


@pytest.mark.parametrize("bad", [
    {"kind": "step"},
    {"kind": "linear", "warmup_steps": -1},
    {"kind": "linear", "decay_steps": -5},
    {"kind": "cosine", "lr_min": -1e-4},
    {"kind": "cosine", "lr_min": 2 * LR},
    {"kind": "linear", "warmup_steps": 5, "decay_steps": 5},
    {"kind": "cosine", "warmup_steps": 5, "decay_steps": 3},
    {"kind": "cosine", "steps": 3},
])
def test_constructor_validation(bad):
    with pytest.raises(ValueError):
        _opt(bad)


def test_config_keys_and_trainer():
    from dinunet_implementations_amd.config import build_config, generate_compspec, lr_schedule_of
    from dinunet_implementations_amd.runtime.trainer import NNTrainer
    cfg = build_config()
    assert cfg["lr_schedule"] is None and cfg["lr_warmup_steps"] == 0 and cfg["lr_decay_steps"] is None
    assert cfg["lr_min"] == 0.0 and cfg["lr_plateau_factor"] == 0 and cfg["lr_plateau_patience"] == 2
    assert lr_schedule_of(cfg) is None
    inputs = generate_compspec()["computation"]["input"]
    assert not [k for k in inputs if k.startswith("lr_")]
    for bad in ({"lr_schedule": "step"}, {"lr_warmup_steps": -1}, {"lr_warmup_steps": 1.5},
                {"lr_decay_steps": -1}, {"lr_min": -1.0}, {"lr_min": 1.0, "learning_rate": 0.1},
                {"lr_schedule": "cosine", "lr_warmup_steps": 4, "lr_decay_steps": 4},
                {"lr_plateau_factor": 1.0}, {"lr_plateau_factor": -0.5}, {"lr_plateau_patience": -1},
                {"pretrain_args": {"lr_schedule": "nope"}}):
        with pytest.raises(ValueError):
            build_config(overrides=bad)
    # on when a kind is set, a warmup is asked for, or the plateau reduction is
    assert lr_schedule_of(build_config(overrides={"lr_warmup_steps": 4})) == {
        "kind": "constant", "warmup_steps": 4, "decay_steps": None, "lr_min": 0.0}
    assert lr_schedule_of(build_config(overrides={"lr_plateau_factor": 0.5}))["kind"] == "constant"

    class _T(NNTrainer):
        def _init_nn_model(self):
            self.nn["net"] = nn.Linear(4, 2)

    def trainer(**ov):
        t = _T(build_config(overrides=dict(ov, gpus=[])))
        if getattr(t, "optimizer", None) is None:
            t.init_nn()
        return t

    assert trainer().optimizer.lr_schedule is None
    sc = trainer(lr_schedule="cosine", lr_warmup_steps=2, lr_decay_steps=30, lr_min=1e-5,
                 learning_rate=1e-3).optimizer.lr_schedule
    assert (sc.kind, sc.warmup_steps, sc.decay_steps, sc.lr_min) == ("cosine", 2, 30, 1e-5)


# ---- plateau reduction ----------------------------------------------------------------------------
def test_plateau_counter_reduces_after_patience_and_stops_at_the_floor():
    from dinunet_implementations_amd.utils.metrics import improved
    _, opt = _opt({"kind": "constant", "lr_min": 0.2 * LR})
    scores = [0.50, 0.60, 0.60, 0.59, 0.58, 0.61, 0.60, 0.60, 0.60, 0.60, 0.60, 0.60, 0.60, 0.60]
    best, reduced, scales = None, [], []
    for epoch, s in enumerate(scores, 1):
        better = improved(s, best, "maximize")
        if better:
            best = s
        if opt.plateau_step(better, 0.5, patience=2):
            reduced.append(epoch)
        scales.append(opt.lr_scale)
    # epochs 3, 4, 5 do not improve: the counter exceeds 2 at epoch 5; 6 improves (reset);
    # 7, 8, 9 -> 9; 10, 11, 12 -> 12 (0.125 < the floor lr_min / lr = 0.2)
    assert reduced == [5, 9, 12]
    assert scales[3] == 1.0 and scales[4] == 0.5 and scales[8] == 0.25
    assert scales[11] == scales[13] == pytest.approx(0.2)
    assert opt.lr_at(1) == pytest.approx(0.2 * LR, rel=1e-6)  # never below lr_min
    assert float(opt._lrs_f[1]) == f32(scales[-1])
    _, off = _opt(None)
    with pytest.raises(ValueError):
        off.plateau_step(False, 0.5, 0)


def w_fs_site(grp, data_path, out, overrides):
    from dinunet_implementations_amd.config import build_config, load_inputspec
    from dinunet_implementations_amd.runtime.site import FederatedSite
    from dinunet_implementations_amd.tasks import get_task
    specs = load_inputspec(os.path.join(data_path, "inputspec.json"))
    cfg = build_config(site_input=specs[grp.rank], overrides=overrides)
    state = {"baseDirectory": os.path.join(data_path, "input", f"local{grp.rank}", "simulatorRun")}
    T, D, H = get_task(cfg["task_id"])
    logs = FederatedSite(cfg, grp, T, D, H, state, out, verbose=False).run()
    return [{k: v for k, v in l.items() if k in ("replica_check", "learning_rate",
                                                  "lr_reduced_epochs", "validation_log")}
            for l in logs]


def _logs(out, site, task="FS-Classification"):
    with open(os.path.join(out, site, task, "fold_0", "logs.json")) as f:
        return json.load(f)


PLATEAU_EPOCHS, PLATEAU_LR = 8, 1e-2


_PLATEAU_RUN = {}


@pytest.fixture
def plateau_run(fs_data_root, tmp_path_factory):
    """ONE two-site gloo run of the FS fixture with the plateau reduction on (patience 0, factor
    0.5) and replica checks, made by the first test that asks and shared with the others."""
    if not _PLATEAU_RUN:
        out = str(tmp_path_factory.mktemp("plateau"))
        res = run_world(w_fs_site, 2, fs_data_root, out,
                        {"epochs": PLATEAU_EPOCHS, "learning_rate": PLATEAU_LR, "patience": 100,
                         "check_replicas": True, "lr_plateau_factor": 0.5,
                         "lr_plateau_patience": 0})
        _PLATEAU_RUN.update(out=out, res=res)
    return _PLATEAU_RUN["out"], _PLATEAU_RUN["res"]


def test_site_loop_halves_the_rate_after_every_validation_without_improvement(plateau_run):
    from dinunet_implementations_amd.utils.metrics import improved
    out, _ = plateau_run
    logs = _logs(out, "local0")
    rates, val = logs["learning_rate"], logs["validation_log"]
    assert len(rates) == len(val) == PLATEAU_EPOCHS
    best, k, reduced = None, 0, []
    for e in range(PLATEAU_EPOCHS):  # epoch e + 1 trains before its validation
        assert rates[e] == f32(PLATEAU_LR) * 0.5 ** k, (e, k, rates)
        if improved(val[e][1], best, "maximize"):
            best = val[e][1]
        else:
            k += 1
            reduced.append(e + 1)
    print("validation scores", [v[1] for v in val], "reduced after epochs", reduced)
    assert logs["lr_reduced_epochs"] == reduced
    assert len(reduced) >= 1 and reduced[0] < PLATEAU_EPOCHS  # a reduction took effect


def test_two_gloo_sites_reduce_alike_and_stay_bit_identical(plateau_run):
    _, res = plateau_run
    a, b = res[0][0], res[1][0]
    assert len(a["replica_check"]) == PLATEAU_EPOCHS and all(a["replica_check"])
    assert all(b["replica_check"])
    assert a["learning_rate"] == b["learning_rate"]
    assert a["lr_reduced_epochs"] == b["lr_reduced_epochs"]


def test_schedule_off_logs_as_before(fs_data_root, tmp_path):
    run_world(w_fs_site, 2, fs_data_root, str(tmp_path), {"epochs": 1})
    logs = _logs(str(tmp_path), "local0")
    assert "learning_rate" not in logs and "lr_reduced_epochs" not in logs


def test_pretraining_runs_its_own_schedule_and_the_federated_phase_starts_anew(fs_data_root, tmp_path):
    """``pretrain_args`` overrides the keys for the pretraining phase (here: a linear decay where
    the federated phase warms up at a constant rate); the optimizer is rebuilt afterwards, so the
    federated schedule starts at update 1."""
    out = str(tmp_path)
    run_world(w_fs_site, 2, fs_data_root, out,
              {"epochs": 2, "learning_rate": 1e-3, "lr_warmup_steps": 1000, "pretrain": True,
               "pretrain_args": {"epochs": 2, "learning_rate": 1e-2, "batch_size": 16,
                                 "lr_schedule": "linear", "lr_warmup_steps": 0}})
    l0, l1 = _logs(out, "local0"), _logs(out, "local1")
    assert l0["pretrain_site"] == "local0" and "pretrain_learning_rate" not in l1
    pre = l0["pretrain_learning_rate"]
    assert len(pre) == 2 and pre[0] < f32(1e-2) and pre[1] == 0.0  # decays to 0 with the phase
    fed = l0["learning_rate"]
    assert fed == l1["learning_rate"] and len(fed) == 2
    # still warming up from update 1: t / 1000 of the federated rate after t updates
    t1 = round(fed[0] / f32(1e-3) * 1000)
    assert t1 >= 1 and fed[0] == f32(f32(1e-3) * (t1 / 1000)) and fed[1] == f32(f32(1e-3) * (2 * t1 / 1000))


# ---- resume ---------------------------------------------------------------------------------------
def test_resume_mid_schedule_reproduces_the_uninterrupted_run(fs_data_root, tmp_path):
    """Cosine decay and the plateau reduction both on; stopped after epoch 3 of 6 (the decay's
    length is given, so the shorter first leg runs the same schedule)."""
    from test_runtime_e2e import w_site
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    base = {"patience": 100, "seed": 3, "learning_rate": PLATEAU_LR, "lr_schedule": "cosine",
            "lr_warmup_steps": 3, "lr_decay_steps": 40, "lr_min": 1e-4,
            "lr_plateau_factor": 0.5, "lr_plateau_patience": 0}
    run_world(w_site, 2, fs_data_root, a, dict(base, epochs=6))
    run_world(w_site, 2, fs_data_root, b, dict(base, epochs=3))
    run_world(w_site, 2, fs_data_root, b, dict(base, epochs=6, resume=True))
    for site in ("local0", "local1"):
        la, lb = _logs(a, site), _logs(b, site)
        for k in ("train_log", "validation_log", "best_val_epoch", "learning_rate"):
            assert la[k] == lb[k], (site, k, la[k], lb[k])
        assert la.get("lr_reduced_epochs") == lb.get("lr_reduced_epochs")
        assert len(la["learning_rate"]) == 6 and len(set(la["learning_rate"])) == 6
        ca, cb = (torch.load(os.path.join(o, site, "FS-Classification", "fold_0",
                                          "checkpoint_last.pt"), weights_only=True) for o in (a, b))
        for name in ca["models"]:
            for p in ca["models"][name]:
                assert torch.equal(ca["models"][name][p], cb["models"][name][p]), (site, name, p)
        oa, ob = ca["optimizer"], cb["optimizer"]
        assert oa["step"] == ob["step"] and oa["lr_scale"] == ob["lr_scale"]
        assert oa["plateau_wait"] == ob["plateau_wait"] and oa["lr_schedule"] == ob["lr_schedule"]
    print("learning_rate", la["learning_rate"], "reduced", la.get("lr_reduced_epochs"))


# ---- COINSTAC phase machines ----------------------------------------------------------------------
def test_coinstac_nodes_follow_the_schedule(fs_data_root, tmp_path):
    from dinunet_implementations_amd.compat.nodes import LocalNode, RemoteNode
    from dinunet_implementations_amd.compat.simulator import simulate
    it, locs, rem = simulate(fs_data_root, str(tmp_path), lambda: LocalNode(device="cpu"), RemoteNode,
                             overrides={"epochs": 1, "lr_schedule": "linear", "lr_warmup_steps": 2,
                                        "lr_decay_steps": 12, "lr_min": 1e-4})
    opts = [locs[s].trainer.optimizer for s in sorted(locs)]
    for o in opts:
        assert o.step_count > 2 and o.lr_schedule.kind == "linear"
        assert float(o.applied_lr) == o.lr_at(o.step_count) < o.lr
    ws = [locs[s].trainer.flat.data for s in sorted(locs)]
    assert all(torch.equal(w, ws[0]) for w in ws)


@pytest.mark.parametrize("overrides", [
    {"lr_schedule": "cosine"},  # a decaying kind without lr_decay_steps
    {"lr_schedule": "linear", "lr_warmup_steps": 2},
    {"lr_plateau_factor": 0.5},
    {"lr_schedule": "cosine", "lr_decay_steps": 12, "lr_plateau_factor": 0.5},
])
def test_coinstac_nodes_refuse_what_they_cannot_run(fs_data_root, tmp_path, overrides):
    from dinunet_implementations_amd.compat.nodes import LocalNode, RemoteNode
    from dinunet_implementations_amd.compat.simulator import simulate
    with pytest.raises(ValueError, match="lr_decay_steps|lr_plateau_factor"):
        simulate(fs_data_root, str(tmp_path), lambda: LocalNode(device="cpu"), RemoteNode,
                 overrides=dict(overrides, epochs=1))
