"""The packing Adam summing the split-K weight-gradient partials itself (``DINUNET_ADAM_SLABS``,
``optim.hip slab_grad``) against the ``gemm_splitk_reduce`` launch it replaces: device-fed K-step
graph replays of the small ICA model, once armed and once with the switch off, from the same
seed -- parameters, both Adam moments, every persistent operand image and the train-record rings
must agree bit for bit, and the steps that must not arm (clipping, rank-dAD) must keep the reduce
launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

K, WARM, REPLAYS = 2, 3, 3


def _data(B, S, n=6):
    g = torch.Generator(device="cuda").manual_seed(7)
    xs = torch.randn(n * B, S, 20, 10, device="cuda", generator=g)
    ys = torch.randint(0, 2, (n * B,), device="cuda", generator=g)
    return xs.to(torch.bfloat16), ys, n


def _snapshot(step, feed):
    pp = step._apack
    t = {"data": step.flat.data, "m": step.opt.exp_avg, "v": step.opt.exp_avg_sq,
         "wih": pp.wih_p, "bias": pp.bias_p, "whh": pp.whh_p, "whhT": pp.whhT_p,
         "losses": feed.rec.losses, "scores": feed.rec.scores}
    for i, c in enumerate(pp.casts + pp.extra):
        t[f"image{i}"] = c
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in t.items()}


def _train(monkeypatch, armed, splits, B, S, hidden=128, engine="dSGD", clip=None, reload=False,
           sched=None):
    """Warm-up + 3 replays of a 2-step graph (+ 2 more after a parameter change); returns the
    state snapshots, the reduce launches (after warm-up, at the end) and whether the step armed."""
    from dinunet_implementations_amd.models import ICALstm
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.ops import gemm as gemm_mod
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime import step as step_mod
    from dinunet_implementations_amd.runtime.feed import DeviceFeed
    monkeypatch.setattr(step_mod, "ADAM_SLABS", armed)
    monkeypatch.setattr(gemm_mod, "_GROUP_SPLITS", splits)
    torch.manual_seed(0)
    m = ICALstm(input_size=64, hidden_size=hidden, num_comps=20, window_size=10).cuda().train()
    m.classifier[0].p = 0.0
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3, max_grad_norm=clip, lr_schedule=sched)
    eng = make_engine(engine, m, flat, SiteGroup(device=torch.device("cuda")),
                      {"precision_bits": "32"})
    step = step_mod.TrainStep(m, flat, opt, eng, task="ica", use_graph=True)
    X, Y, nb = _data(B, S)
    feed = DeviceFeed(step, X, Y, B, nb, col=1, steps_per_graph=K)
    assert step._apack is not None
    feed.run(WARM)
    torch.cuda.synchronize()
    r_warm = gemm_mod.reduce_launches()
    feed.run(K * REPLAYS)
    snaps = [_snapshot(step, feed)]
    if reload:
        # a load_state-style change of the parameters and moments in place: the captured graph
        # (and the slab addresses baked into it) is replayed again on the new state
        g = torch.Generator(device="cuda").manual_seed(3)
        flat.data.add_(torch.randn(flat.data.shape, device="cuda", generator=g) * 1e-2)
        opt.exp_avg.mul_(0.5)
        graphs = dict(step._dgraphs)
        feed.run(K * 2)
        assert all(step._dgraphs[k][0] is graphs[k][0] for k in graphs), "no recapture"
        snaps.append(_snapshot(step, feed))
    assert opt.step_count == WARM + K * REPLAYS + (K * 2 if reload else 0)
    return snaps, (r_warm, gemm_mod.reduce_launches()), step._slabs_ok()


def _same(a, b):
    for sa, sb in zip(a, b):
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (k, (sa[k].float() - sb[k].float()).abs().max())


@pytest.mark.parametrize("splits,B,S,hidden", [
    (3, 8, 24, 128),   # K = 192 = 3 x 64: the headline's split count (all remainder loads)
    (2, 8, 24, 128),
    (5, 8, 40, 128),   # K = 320: one round of four plus a remainder
    (3, 8, 24, 88),    # 44 units per direction padded to 64: row_map = -1 rows, the map's edge
])
def test_slab_sum_matches_reduce_kernel_bitwise(monkeypatch, splits, B, S, hidden):
    on, (w1, e1), a1 = _train(monkeypatch, True, splits, B, S, hidden, reload=True)
    off, (w0, e0), a0 = _train(monkeypatch, False, splits, B, S, hidden, reload=True)
    assert a1 and not a0
    assert e1 == w1, "armed: no gemm_splitk_reduce in the captured steps"
    assert e0 > w0, "switch off: the reduce launch is captured"
    _same(on, off)
    assert float(on[0]["data"].sub(on[1]["data"]).abs().max()) > 0  # the replays did train


def test_scheduled_rate_launch_sums_slabs_too(monkeypatch):
    """The learning-rate schedule is another instantiation of the Adam launch: armed there too."""
    sched = {"kind": "cosine", "warmup_steps": 4, "decay_steps": 40, "lr_min": 1e-5}
    on, (w1, e1), a1 = _train(monkeypatch, True, 3, 8, 24, sched=sched)
    off, (w0, e0), _ = _train(monkeypatch, False, 3, 8, 24, sched=sched)
    assert a1 and e1 == w1 and e0 > w0
    _same(on, off)


def test_one_split_is_a_no_op(monkeypatch):
    on, (w1, e1), _ = _train(monkeypatch, True, 1, 8, 24)
    off, (w0, e0), _ = _train(monkeypatch, False, 1, 8, 24)
    assert e1 == w1 and e0 == w0  # no slabs, no reduce, either way
    _same(on, off)


@pytest.mark.parametrize("engine,clip", [("dSGD", 1.0), ("rankDAD", None)])
def test_steps_that_read_the_gradient_keep_the_reduce(monkeypatch, engine, clip):
    """Global-norm clipping and rank-dAD read ``flat.grad`` between the backward and the update:
    the armed switch must change nothing -- same results, reduce launch captured."""
    on, (w1, e1), a1 = _train(monkeypatch, True, 3, 8, 24, engine=engine, clip=clip)
    off, (w0, e0), _ = _train(monkeypatch, False, 3, 8, 24, engine=engine, clip=clip)
    assert not a1
    assert e1 > w1 and e1 - w1 == e0 - w0
    _same(on, off)
