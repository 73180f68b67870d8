"""Class weights and label smoothing in the fused classifier heads (``csrc/kernels/loss_opt.h``):
``dn_softmax_xent``, ``mlp_head.hip`` (B <= 64), ``head_big.hip`` (B > 64) and the one-launch
``head_rep.hip``, against ``F.cross_entropy(weight=, label_smoothing=)`` on the module chain with
the kernels' rounding points (the helpers of tests/test_head_layernorm_gpu.py), plus the exact
properties: off == all-ones weights bitwise, one launch == three launches bitwise, captured graphs
follow ``set_loss``."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

W = {2: [0.3, 2.5], 3: [0.5, 1.0, 3.0], 16: [0.25 + 0.25 * i for i in range(16)],
     40: [0.5 + 0.05 * i for i in range(40)]}


def rel(a, b):
    a, b = a.float(), b.float()
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


def _ica_head(norm="batch", p=0.0, hidden=384, ncls=2):
    n = nn.BatchNorm1d(256) if norm == "batch" else nn.LayerNorm(256)
    return nn.Sequential(nn.Dropout(p), nn.Linear(hidden, 256), n, nn.ReLU(),
                         nn.Linear(256, 64), nn.ReLU(), nn.Linear(64, ncls))


def _perturb_norm(head):
    with torch.no_grad():
        head[2].weight.uniform_(0.5, 1.5)
        head[2].bias.uniform_(-0.3, 0.3)


class _RoundFwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, d):
        return d


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, d):
        return d.to(torch.bfloat16).float()


def _emulated(mods, x):
    """The module chain with the kernels' rounding points (bf16 MFMA operands, fp32 elsewhere)."""
    from dinunet_implementations_amd.ops.head import HeadSpec
    spec = HeadSpec(mods)
    a = x
    for L in spec.layers:
        lin = L.linear
        z = _RoundBwd.apply(_RoundFwd.apply(a) @ _RoundFwd.apply(lin.weight).t())
        if lin.bias is not None:
            z = z + lin.bias
        if L.bn is not None:
            z = L.bn(z)
        if L.relu:
            z = torch.relu(z)
        a = z
    return a


def _labels(B, C, mode, gen):
    """mixed: every class may occur; absent: the last class never occurs; single: one class."""
    if mode == "single":
        return torch.full((B,), C - 1, device=DEV, dtype=torch.long)
    hi = C - 1 if mode == "absent" else C
    return torch.randint(0, max(hi, 1), (B,), device=DEV, generator=gen)


def _ref_loss(logits, y, w, eps, log_out):
    from dinunet_implementations_amd.ops import reference as ref
    wt = None if w is None else torch.tensor(w, device=logits.device)
    return (ref.log_softmax_nll if log_out else ref.softmax_ce)(logits, y, wt, eps)


def _head_run(mods, x, y, log_out, w=None, eps=0.0, hint=None):
    """One fused forward + backward; returns (out, loss, pred, dx, [param grads])."""
    from dinunet_implementations_amd.ops import head as H
    spec = H.HeadSpec(mods, class_weights=w, label_smoothing=eps)
    assert spec.ok and spec.supported(x)
    xi = x.clone().requires_grad_()
    with H.loss_grad_hint(hint):
        out, loss, pred = H.head_loss(xi, spec, y, log_out=log_out)
    if hint is not None:
        torch.autograd.backward(loss, hint)
    else:
        loss.backward()
    torch.cuda.synchronize()
    return (out.detach().clone(), loss.detach().clone(), pred.clone(), xi.grad.clone(),
            [q.grad.clone() for m in mods for q in m.parameters()])


def _flat(r):
    return list(r[:4]) + list(r[4])


# ---- 1. dn_softmax_xent alone ------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("C", [2, 3, 16, 40])
@pytest.mark.parametrize("B", [1, 5, 64, 200])
def test_softmax_xent_options(B, C, eps):
    """Loss and dz against fp32 torch on the same logits, at test_kernels_gpu.py::test_softmax_xent's
    tolerances (out 1e-5, loss 1e-5, dz 1e-6 absolute)."""
    from dinunet_implementations_amd.ops import heads
    gen = torch.Generator(device=DEV).manual_seed(100 * B + C)
    log_out = (B + C) % 2 == 1
    z = torch.randn(B, C, device=DEV, generator=gen).requires_grad_()
    y = torch.randint(0, C, (B,), device=DEV, generator=gen)
    fn = heads.log_softmax_nll if log_out else heads.softmax_ce
    out, loss, pred = fn(z, y, weight=W[C], label_smoothing=eps)
    zr = z.detach().clone().requires_grad_()
    ro, rl, rp = _ref_loss(zr, y, W[C], eps, log_out)
    loss.backward()
    rl.backward()
    print(f"B={B} C={C} eps={eps} loss {loss.item():.7f} ref {rl.item():.7f} "
          f"max|dz - ref| {(z.grad - zr.grad).abs().max().item():.3e}")
    assert torch.allclose(out, ro, atol=1e-5) and abs(loss.item() - rl.item()) < 1e-5
    assert torch.equal(pred, rp)
    assert torch.allclose(z.grad, zr.grad, atol=1e-6)
    # outputs and pred do not depend on the options
    o0, _, p0 = fn(z.detach(), y)
    assert torch.equal(o0, out) and torch.equal(p0, pred)


# ---- 2. fused heads against the weighted emulation ---------------------------------------------
CASES = [(2, 0.0, "mixed"), (2, 0.1, "single"), (3, 0.1, "absent"), (3, 0.0, "mixed")]


def _check_head(mods, ref_mods, x, y, log_out, w, eps, skip=()):
    got = _head_run(mods, x, y, log_out, w, eps)
    off = _head_run([copy.deepcopy(m) for m in ref_mods], x, y, log_out)
    xr = x.clone().requires_grad_()
    ro, rl, _ = _ref_loss(_emulated(ref_mods, xr), y, w, eps, log_out)
    rl.backward()
    out, loss, pred, dx, grads = got
    print(f"B={x.shape[0]} loss {loss.item():.6f} ref {rl.item():.6f} rel(out) {rel(out, ro):.3e} "
          f"rel(dx) {rel(dx, xr.grad):.3e}")
    names = [f"{i}.{n}" for i, m in enumerate(ref_mods) for n, _ in m.named_parameters()]
    refg = [q.grad for m in ref_mods for q in m.parameters()]
    errs = {n: rel(g, r) for n, g, r in zip(names, grads, refg) if n not in skip}
    print("  grads", {n: f"{e:.3e}" for n, e in errs.items()})
    # out and pred are bitwise those of the same head with the options off
    assert torch.equal(out, off[0]) and torch.equal(pred, off[2])
    assert torch.equal(pred, out.argmax(1))
    assert abs(loss.item() - rl.item()) < 2e-2 * max(1.0, abs(rl.item()))
    assert rel(out, ro) < 2e-2
    assert rel(dx, xr.grad) < 2e-2
    for n, e in errs.items():
        assert e < 2e-2, (n, e)
    for n, g in zip(names, grads):
        if n in skip:  # feeds a batch-statistics BatchNorm: the true gradient is 0
            assert g.abs().max() < 1e-5
    return got


@pytest.mark.parametrize("C,eps,mode", CASES)
@pytest.mark.parametrize("B", [2, 7, 32, 33, 64, 65, 200])
def test_ica_batchnorm_head_matches_weighted_emulation(B, C, eps, mode):
    torch.manual_seed(B)
    gen = torch.Generator(device=DEV).manual_seed(B + 17 * C)
    head = _ica_head("batch", ncls=C).to(DEV).train()
    _perturb_norm(head)
    ref_head = copy.deepcopy(head)
    x = torch.randn(B, 384, device=DEV, generator=gen)
    y = _labels(B, C, mode, gen)
    _check_head(list(head), list(ref_head), x, y, False, W[C], eps, skip=("1.bias",))


@pytest.mark.parametrize("C,eps,mode", CASES)
@pytest.mark.parametrize("B", [1, 2, 7, 32, 33, 64, 65, 200])
def test_ica_layernorm_head_matches_weighted_emulation(B, C, eps, mode):
    torch.manual_seed(B)
    gen = torch.Generator(device=DEV).manual_seed(B + 17 * C)
    head = _ica_head("layer", ncls=C).to(DEV).train()
    _perturb_norm(head)
    ref_head = copy.deepcopy(head)
    x = torch.randn(B, 384, device=DEV, generator=gen)
    y = _labels(B, C, mode, gen)
    _check_head(list(head), list(ref_head), x, y, False, W[C], eps)


@pytest.mark.parametrize("B", [32, 200])
def test_ica_head_sixteen_classes(B):
    torch.manual_seed(B)
    gen = torch.Generator(device=DEV).manual_seed(B)
    head = _ica_head("layer", ncls=16).to(DEV).train()
    ref_head = copy.deepcopy(head)
    x = torch.randn(B, 384, device=DEV, generator=gen)
    y = _labels(B, 16, "absent", gen)
    _check_head(list(head), list(ref_head), x, y, False, W[16], 0.1)


@pytest.mark.parametrize("C,eps,mode", CASES)
@pytest.mark.parametrize("B", [5, 48, 130])
def test_fs_network_matches_weighted_emulation(B, C, eps, mode):
    from dinunet_implementations_amd.models import MSANNet
    torch.manual_seed(3)
    gen = torch.Generator(device=DEV).manual_seed(B + 17 * C)
    net = MSANNet(66, [256, 128, 64, 32], C).to(DEV).train()
    ref_net = copy.deepcopy(net)
    mods = [m for blk in net.layers for m in blk] + [net.fc_out]
    ref_mods = [m for blk in ref_net.layers for m in blk] + [ref_net.fc_out]
    x = torch.rand(B, 66, device=DEV, generator=gen)
    y = _labels(B, C, mode, gen)
    _check_head(mods, ref_mods, x, y, True, W[C], eps)


# ---- 3. negative control -----------------------------------------------------------------------
def test_weighted_gradients_differ_from_the_unweighted_emulation():
    """The bound of the comparisons above is 2e-2; the weighted gradients are further than ten
    times that from the UNWEIGHTED emulation, so those tests can tell the two apart."""
    torch.manual_seed(0)
    head = _ica_head("batch").to(DEV).train()
    ref_head = copy.deepcopy(head)
    x = torch.randn(32, 384, device=DEV)
    y = torch.randint(0, 2, (32,), device=DEV)
    got = _head_run(list(head), x, y, False, W[2], 0.0)
    xr = x.clone().requires_grad_()
    _, rl, _ = _ref_loss(_emulated(list(ref_head), xr), y, None, 0.0, False)
    rl.backward()
    e = rel(got[3], xr.grad)
    ew = rel(got[4][-2], ref_head[6].weight.grad)
    print(f"weighted vs unweighted: rel(dx) {e:.3e} rel(dW_last) {ew:.3e}")
    assert e > 10 * 2e-2 and ew > 10 * 2e-2


# ---- 4. all-ones weights with eps = 0 are bitwise the off path ---------------------------------
@pytest.mark.parametrize("B,norm,hinted", [(32, "batch", False), (65, "batch", False),
                                           (200, "batch", False), (200, "layer", False),
                                           (4, "batch", True), (32, "batch", True),
                                           (32, "layer", True)])
def test_unit_weights_are_bitwise_the_off_path(B, norm, hinted):
    from dinunet_implementations_amd.ops import head as H
    torch.manual_seed(1)
    head = _ica_head(norm).to(DEV).train()
    x = torch.randn(B, 384, device=DEV)
    y = torch.randint(0, 2, (B,), device=DEV)
    one = torch.ones((), device=DEV) if hinted else None
    n0 = H.REP_LAUNCHES
    a = _head_run(list(copy.deepcopy(head)), x, y, False, hint=one)
    b = _head_run(list(copy.deepcopy(head)), x, y, False, [1.0, 1.0], 0.0, hint=one)
    if hinted:
        assert H.REP_LAUNCHES == n0 + 2, "the replicated head did not run"
    for u, v in zip(_flat(a), _flat(b)):
        assert torch.equal(u, v)


def test_unit_weights_are_bitwise_the_off_path_fs():
    from dinunet_implementations_amd.models import MSANNet
    torch.manual_seed(2)
    net = MSANNet(66, [256, 128, 64, 32], 2).to(DEV).train()
    for B in (48, 130):
        x = torch.rand(B, 66, device=DEV)
        y = torch.randint(0, 2, (B,), device=DEV)
        res = []
        for w in (None, [1.0, 1.0]):
            n = copy.deepcopy(net)
            res.append(_head_run([m for blk in n.layers for m in blk] + [n.fc_out], x, y, True, w))
        for u, v in zip(_flat(res[0]), _flat(res[1])):
            assert torch.equal(u, v)


@pytest.mark.parametrize("B,C", [(5, 2), (200, 3), (37, 40)])
def test_unit_weights_are_bitwise_the_off_path_softmax_xent(B, C):
    from dinunet_implementations_amd.ops import heads
    torch.manual_seed(B)
    z = torch.randn(B, C, device=DEV)
    y = torch.randint(0, C, (B,), device=DEV)
    res = []
    for w in (None, [1.0] * C):
        zi = z.clone().requires_grad_()
        out, loss, pred = heads.softmax_ce(zi, y, weight=w)
        loss.backward()
        res.append((out.detach(), loss.detach(), pred, zi.grad))
    for u, v in zip(*res):
        assert torch.equal(u, v)


# ---- 5. one launch against three launches, options on ------------------------------------------
@pytest.mark.parametrize("norm", ["batch", "layer"])
@pytest.mark.parametrize("B,p", [(4, 0.0), (32, 0.0), (32, 0.25)])
def test_one_launch_equals_three_launch_with_options(B, p, norm):
    from dinunet_implementations_amd.ops import head as H
    torch.manual_seed(11)
    base = _ica_head(norm, p=p).to(DEV).train()
    _perturb_norm(base)
    x = torch.randn(B, 384, device=DEV)
    y = torch.randint(0, 2, (B,), device=DEV)
    one = torch.ones((), device=DEV)
    res, seed0 = [], None
    n0 = H.REP_LAUNCHES
    for one_launch in (True, False):
        ms = list(copy.deepcopy(base))
        old = H._HEAD_STEP
        H._HEAD_STEP = one_launch
        try:
            spec = H.HeadSpec(ms, class_weights=W[2], label_smoothing=0.1)
            assert spec.ok and spec.supported(x)
            r = spec.rng(x.device)
            if seed0 is None:
                seed0 = r.clone()
            else:
                r.copy_(seed0)
            for _ in range(2):  # twice: the gradients accumulate
                xi = x.clone().requires_grad_()
                with H.loss_grad_hint(one):
                    out, loss, pred = H.head_loss(xi, spec, y, log_out=False)
                torch.autograd.backward(loss, one)
            torch.cuda.synchronize()
        finally:
            H._HEAD_STEP = old
        res.append((out.clone(), loss.clone(), pred.clone(), xi.grad.clone(),
                    [q.grad.clone() for m in ms for q in m.parameters()]))
    assert H.REP_LAUNCHES == n0 + 2, "the replicated head did not run"
    for u, v in zip(_flat(res[0]), _flat(res[1])):
        assert torch.equal(u, v)
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in res[0][4])


# ---- 6. row duplication ------------------------------------------------------------------------
# Measured on the parent's code path (the options off; profiles/loss_options_bench.md): the
# unweighted LayerNorm head on the 36-row batch below against four row permutations of it differs
# by at most PERM_DIFF relative in the loss and in any parameter gradient; the identity is held to
# twice that.
PERM_DIFF = 2.18e-7


def _ln_grads(head, x, y, w=None):
    r = _head_run(list(copy.deepcopy(head)), x, y, False, w)
    return r[1], r[4]


def _dup_batch(seed=9):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(24, 384, device=DEV, generator=gen)
    y = torch.cat([torch.zeros(12, dtype=torch.long), torch.ones(12, dtype=torch.long)]).to(DEV)
    y = y[torch.randperm(24, device=DEV, generator=gen)]
    ones = (y == 1).nonzero().flatten()
    return x, y, torch.cat([x, x[ones]]), torch.cat([y, y[ones]])


def measure_permutation_difference():
    """Unweighted head on the 36-row duplicated batch against a row permutation of it."""
    torch.manual_seed(9)
    head = _ica_head("layer").to(DEV).train()
    _perturb_norm(head)
    _, _, xd, yd = _dup_batch()
    worst = 0.0
    for s in range(4):
        perm = torch.randperm(36, device=DEV, generator=torch.Generator(device=DEV).manual_seed(s))
        la, ga = _ln_grads(head, xd, yd)
        lb, gb = _ln_grads(head, xd[perm], yd[perm])
        worst = max([worst, abs(la.item() - lb.item()) / abs(la.item())]
                    + [rel(u, v) for u, v in zip(ga, gb)])
    return worst


def test_weighted_batch_equals_unweighted_duplicated_batch():
    """w = [1, 2], eps = 0 on 24 rows == no weights on the batch with every class-1 row twice
    (LayerNorm head: rows are independent); only the summation order differs."""
    torch.manual_seed(9)
    head = _ica_head("layer").to(DEV).train()
    _perturb_norm(head)
    x, y, xd, yd = _dup_batch()
    lw, gw = _ln_grads(head, x, y, [1.0, 2.0])
    lu, gu = _ln_grads(head, xd, yd)
    errs = [abs(lw.item() - lu.item()) / abs(lu.item())] + [rel(u, v) for u, v in zip(gw, gu)]
    print("row duplication: rel errors", [f"{e:.3e}" for e in errs],
          "permutation difference now", measure_permutation_difference())
    assert max(errs) <= 2 * PERM_DIFF, errs


# ---- 7. captured steps -------------------------------------------------------------------------
def _ica(seed=0, w=None, eps=0.0):
    from dinunet_implementations_amd.models import ICALstm
    torch.manual_seed(seed)
    m = ICALstm(input_size=64, hidden_size=128, num_comps=20, window_size=10, class_weights=w,
                label_smoothing=eps).cuda().train()
    m.classifier[0].p = 0.0
    return m


def _trainer(w, eps=0.0, **kw):
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.step import TrainStep
    m = _ica(0, w, eps)
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3)
    eng = make_engine("dSGD", m, flat, SiteGroup(device=torch.device("cuda")),
                      {"precision_bits": "32"})
    return m, flat, TrainStep(m, flat, opt, eng, task="ica", **kw)


def _data(n=8):
    gen = torch.Generator(device="cuda").manual_seed(7)
    xs = torch.randn(n, 8, 12, 20, 10, device="cuda", generator=gen)
    ys = torch.randint(0, 2, (n, 8), device="cuda", generator=gen)
    return xs, ys, xs.reshape(-1, *xs.shape[2:]).to(torch.bfloat16), ys.reshape(-1)


W2 = [2.0, 0.4]


def test_host_fed_captured_step_follows_set_loss():
    """The one-site captured step with the options on against the eager loop (losses and
    parameters at test_graph_replay_matches_eager's tolerances); then other weights WITHOUT
    recapture: the next replay equals an eager step with the new weights."""
    xs, ys, _, _ = _data(6)
    me, fe, se = _trainer(W[2], 0.1, use_graph=False)
    mg, fg, sg = _trainer(W[2], 0.1, use_graph=True)
    for i in range(4):
        le, lg = float(se(xs[i], ys[i]).detach()), float(sg(xs[i], ys[i]).detach())
        assert abs(le - lg) < 1e-4, (i, le, lg)
    torch.cuda.synchronize()
    graph = sg.graph
    assert graph is not None
    assert torch.allclose(fe.data, fg.data, rtol=1e-5, atol=1e-6)
    me.set_loss(W2, 0.0)
    mg.set_loss(W2, 0.0)
    le, lg = float(se(xs[4], ys[4]).detach()), float(sg(xs[4], ys[4]).detach())
    torch.cuda.synchronize()
    assert sg.graph is graph, "the step was captured again"
    assert abs(le - lg) < 1e-4, (le, lg)
    assert torch.allclose(fe.data, fg.data, rtol=1e-5, atol=1e-6)
    # the new weights mattered: the same step under the first objective reports another loss
    mk, fk, sk = _trainer(W[2], 0.1, use_graph=False)
    fk.data.copy_(fe.data)
    lk = float(sk(xs[4], ys[4]).detach())
    print("loss with new weights", lg, "with the first weights", lk)
    assert abs(lk - lg) > 1e-2


def test_device_fed_graph_follows_set_loss(monkeypatch):
    """K = 4 whole steps per HIP graph with weights, against the host-fed eager loop on the same
    batches (test_device_fed_multistep_graph_matches_host_fed's tolerances); then other weights
    between two replays of the SAME graph."""
    from dinunet_implementations_amd.ops import DeviceSource
    from dinunet_implementations_amd.runtime import step as step_mod
    monkeypatch.setattr(step_mod, "ADAM_PACK", True)
    _, _, X, Y = _data(8)
    B = 8
    mh, fh, sh = _trainer(W[2], 0.1, use_graph=False)
    md, fd, sd = _trainer(W[2], 0.1, use_graph=True)
    src = DeviceSource(X, Y, B)
    sd.bind(src, steps_per_graph=4)

    def host(lo, hi):
        for c in range(lo, hi):
            xb, yb = src.batch(c)
            sh(xb.float(), yb)

    def close():
        torch.cuda.synchronize()
        print("max |host - device-fed|", float((fh.data - fd.data).abs().max()),
              "losses", float(sh.last_loss), float(sd.last_loss))
        return (torch.allclose(fh.data, fd.data, rtol=1e-6, atol=1e-7)
                and abs(float(sh.last_loss) - float(sd.last_loss)) < 1e-5)

    host(0, 7)
    sd.run(3)
    sd.prepare(8)
    graph = sd._dgraphs[4][0]
    sd.run(4)
    assert close()
    mh.set_loss(W2, 0.0)
    md.set_loss(W2, 0.0)
    host(7, 11)
    sd.run(4)
    assert sd._dgraphs[4][0] is graph
    assert close()
    # the new weights mattered
    mk, fk, sk = _trainer(W[2], 0.1, use_graph=False)
    for c in range(11):
        xb, yb = src.batch(c)
        sk(xb.float(), yb)
    torch.cuda.synchronize()
    assert not torch.allclose(fk.data, fh.data, rtol=1e-6, atol=1e-7)


def test_set_loss_needs_the_options_on():
    from dinunet_implementations_amd.ops.head import HeadSpec
    spec = HeadSpec(list(_ica_head()))
    assert not spec.loss_on and spec.loss_block(DEV) is None
    with pytest.raises(RuntimeError):
        spec.set_loss([1.0, 2.0])


# ---- 8. evaluation -----------------------------------------------------------------------------
ICA = dict(task_id="ICA-Classification", num_components=16, window_size=10, window_stride=10,
           temporal_size=120, input_size=32, hidden_size=64, batch_size=32)


def test_eval_feed_and_host_loop_report_the_same_weighted_loss():
    """70 subjects at batch 32 (a tail batch): EvalFeed == NNTrainer.evaluate exactly, and both
    equal the weighted cross-entropy of the host loop's own outputs."""
    from dinunet_implementations_amd.config import build_config
    from dinunet_implementations_amd.data.loader import DeviceLoader
    from dinunet_implementations_amd.runtime.evalfeed import EvalFeed
    from dinunet_implementations_amd.tasks import get_task
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(1)
    X = torch.randn(70, 12, 16, 10, generator=g).to(dev)
    Y = torch.randint(0, 2, (70,), generator=g).to(dev)
    res = {}
    for w in (W[2], None):
        cfg = build_config(overrides=dict(ICA, class_weights=w, label_smoothing=0.1 if w else 0))
        T, _, _ = get_task(cfg["task_id"])
        tr = T(cache=cfg, state={}, device=dev)
        tr.init_nn(seed=0)
        host = tr.evaluate(DeviceLoader(X, Y, 32))
        got = EvalFeed(tr, X, Y, 32).run()
        assert got["averages"].count == host["averages"].count == 70
        assert got["averages"].average == host["averages"].average
        assert torch.equal(got["out"], host["out"])
        res[w is not None] = host
    # the probabilities do not depend on the options; the loss is F.cross_entropy's on them
    assert torch.equal(res[True]["out"], res[False]["out"])
    logp = res[True]["out"].float().log()
    want, n = 0.0, 0
    for i in range(0, 70, 32):
        lb = F.cross_entropy(logp[i:i + 32], Y[i:i + 32], weight=torch.tensor(W[2], device=dev),
                             label_smoothing=0.1)
        want += float(lb) * len(Y[i:i + 32])
        n += len(Y[i:i + 32])
    print("weighted validation loss", res[True]["averages"].average, "from the outputs", want / n)
    assert abs(res[True]["averages"].average - want / n) < 1e-4
    assert abs(res[True]["averages"].average - res[False]["averages"].average) > 1e-3


# ---- 9. rank-dAD capture -----------------------------------------------------------------------
@pytest.mark.parametrize("B", [32, 200])
def test_rank_dad_capture_sees_the_weighted_deltas(B):
    """Shape and bound of test_ica_layernorm_rank_dad_capture, with the options on."""
    from dinunet_implementations_amd.ops.capture import DADCapture
    from dinunet_implementations_amd.ops.head import HeadSpec, head_loss
    torch.manual_seed(8)
    head = _ica_head("layer").to(DEV).train()
    spec = HeadSpec(list(head), class_weights=W[2], label_smoothing=0.1)
    x = torch.randn(B, 384, device=DEV, requires_grad=True)
    y = torch.randint(0, 2, (B,), device=DEV)
    assert spec.ok and spec.supported(x)
    with DADCapture() as cap:
        _, loss, _ = head_loss(x, spec, y, log_out=False)
        loss.backward()
        recs = dict(cap.records)
    for L in spec.layers:
        (A, D), = recs[L.linear]
        assert A.shape == (B, L.linear.in_features) and D.shape == (B, L.linear.out_features)
        assert rel(D.t() @ A, L.linear.weight.grad) < 1e-5
    # and they are the weighted ones: the last layer's Delta is not the unweighted head's
    spec0 = HeadSpec(list(copy.deepcopy(head)))
    with DADCapture() as cap:
        _, loss, _ = head_loss(x.detach().clone().requires_grad_(), spec0, y, log_out=False)
        loss.backward()
        recs0 = dict(cap.records)
    (_, D0), = recs0[spec0.layers[-1].linear]
    (_, D1), = recs[spec.layers[-1].linear]
    assert rel(D1, D0) > 0.2


# ---- 10. determinism ---------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["batch", "layer"])
def test_weighted_head_is_deterministic(norm):
    torch.manual_seed(6)
    head = _ica_head(norm).to(DEV).train()
    x = torch.randn(200, 384, device=DEV)
    y = torch.randint(0, 2, (200,), device=DEV)
    a = _head_run(list(copy.deepcopy(head)), x, y, False, W[2], 0.1)
    b = _head_run(list(copy.deepcopy(head)), x, y, False, W[2], 0.1)
    for u, v in zip(_flat(a), _flat(b)):
        assert torch.equal(u, v)
