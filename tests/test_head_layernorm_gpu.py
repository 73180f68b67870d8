"""LayerNorm heads (norm_layer="layer", kernel norm mode 3) through the fused head kernels --
csrc/kernels/mlp_head.hip for batches <= 64, csrc/kernels/head_big.hip above -- against the module
chain with the kernels' rounding points (bf16 MFMA operands, fp32 everywhere else).

A hinted step of the ICA head (LayerNorm on layer 0) runs the one-launch replicated head
(head_rep.hip), compared with the three-launch path and with the unhinted launches."""
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a, b):
    a, b = a.float(), b.float()
    return (a - b).norm().item() / max(b.norm().item(), 1e-12)


def _ica_head(p=0.0, hidden=384, ncls=2):
    return nn.Sequential(nn.Dropout(p), nn.Linear(hidden, 256), nn.LayerNorm(256), nn.ReLU(),
                         nn.Linear(256, 64), nn.ReLU(), nn.Linear(64, ncls))


class _RoundFwd(torch.autograd.Function):
    """bf16 rounding of a forward value (an MFMA operand); gradient passes through."""
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).float()

    @staticmethod
    def backward(ctx, d):
        return d


class _RoundBwd(torch.autograd.Function):
    """Identity forward; rounds the incoming gradient to bf16 (the kernel's dZ operand)."""
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, d):
        return d.to(torch.bfloat16).float()


def _emulated(mods, x):
    """The module chain with the fused kernel's rounding points (bf16 MFMA operands, fp32
    bias / norm / accumulation), no dropout.  The norm module itself (BatchNorm1d or LayerNorm)
    is applied to the fp32 pre-norm values."""
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


def _run_both(mods, ref_mods, x, y, log_out):
    """Fused head on ``mods`` and the emulation on ``ref_mods``: prints and asserts loss / out /
    pred / dx; returns after both backwards (parameter gradients are in .grad)."""
    from dinunet_implementations_amd.ops import reference as ref
    from dinunet_implementations_amd.ops.head import HeadSpec, head_loss
    spec = HeadSpec(mods)
    assert spec.ok and spec.supported(x)
    xf = x.clone().requires_grad_()
    xr = x.clone().requires_grad_()
    out, loss, pred = head_loss(xf, spec, y, log_out=log_out)
    ro, rl, _ = (ref.log_softmax_nll if log_out else ref.softmax_ce)(_emulated(ref_mods, xr), y)
    print(f"B={x.shape[0]} loss {loss.item():.6f} ref {rl.item():.6f} rel(out) {rel(out, ro):.3e}")
    assert abs(loss.item() - rl.item()) < 2e-2 * max(1.0, abs(rl.item()))
    assert rel(out, ro) < 2e-2
    assert torch.equal(pred, out.argmax(1))
    loss.backward()
    rl.backward()
    print(f"  rel(dx) {rel(xf.grad, xr.grad):.3e}")
    return xf, xr


@pytest.mark.parametrize("B", [1, 7, 32, 33, 64, 65, 200])
def test_ica_layernorm_head_train_matches_emulation(B):
    torch.manual_seed(0)
    head = _ica_head().to(DEV).train()
    with torch.no_grad():  # a LayerNorm that is not at its identity initialisation
        head[2].weight.uniform_(0.5, 1.5)
        head[2].bias.uniform_(-0.3, 0.3)
    ref_head = copy.deepcopy(head)
    x = torch.randn(B, 384, device=DEV)
    y = torch.randint(0, 2, (B,), device=DEV)
    xf, xr = _run_both(list(head), list(ref_head), x, y, log_out=False)
    assert rel(xf.grad, xr.grad) < 2e-2
    for (n, p), (_, q) in zip(head.named_parameters(), ref_head.named_parameters()):
        print(f"  {n} rel {rel(p.grad, q.grad):.3e}")
        assert rel(p.grad, q.grad) < 2e-2, n
    # the bias ahead of a LayerNorm has a real gradient (ahead of a BatchNorm it is ~0)
    gb = dict(ref_head.named_parameters())["1.bias"].grad
    assert gb.abs().max() > 1e-4


@pytest.mark.parametrize("B", [5, 48, 130])
def test_fs_layernorm_ragged_widths(B):
    """66 -> 40 -> 72 -> 2: no width is a tile multiple, so padding columns sit next to the valid
    ones in every row reduction."""
    from dinunet_implementations_amd.models import MSANNet
    torch.manual_seed(3)
    net = MSANNet(66, [40, 72], 2, norm_layer="layer").to(DEV).train()
    with torch.no_grad():
        for blk in net.layers:
            blk[1].weight.uniform_(0.5, 1.5)
            blk[1].bias.uniform_(-0.3, 0.3)
    ref_net = copy.deepcopy(net)
    mods = [m for blk in net.layers for m in blk] + [net.fc_out]
    ref_mods = [m for blk in ref_net.layers for m in blk] + [ref_net.fc_out]
    x = torch.rand(B, 66, device=DEV)
    y = torch.randint(0, 2, (B,), device=DEV)
    xf, xr = _run_both(mods, ref_mods, x, y, log_out=True)
    errs = sorted(rel(p.grad, q.grad) for p, q in zip(net.parameters(), ref_net.parameters()))
    errs.append(rel(xf.grad, xr.grad))
    errs.sort()
    print("  grad errs", [f"{e:.3e}" for e in errs])
    assert errs[len(errs) // 2] < 6e-2 and errs[-1] < 0.1, errs


def test_fs_layernorm_default_network():
    from dinunet_implementations_amd.models import MSANNet
    torch.manual_seed(4)
    net = MSANNet(66, [256, 128, 64, 32], 2, dropout_in=[], norm_layer="layer").to(DEV).train()
    ref_net = copy.deepcopy(net)
    x = torch.rand(16, 66, device=DEV)
    y = torch.randint(0, 2, (16,), device=DEV)
    assert net.head_spec().ok and net.head_spec().supported(x)
    out, loss, pred = net.forward_loss(x, y)
    from dinunet_implementations_amd.ops import reference as ref
    ro, rl, _ = ref.log_softmax_nll(_emulated([m for blk in ref_net.layers for m in blk]
                                              + [ref_net.fc_out], x), y)
    assert abs(loss.item() - rl.item()) < 2e-2 * max(1.0, abs(rl.item()))
    assert rel(out, ro) < 2e-2
    assert torch.equal(pred, out.argmax(1))
    loss.backward()
    rl.backward()
    errs = sorted(rel(p.grad, q.grad) for p, q in zip(net.parameters(), ref_net.parameters()))
    print("  grad errs", [f"{e:.3e}" for e in errs])
    assert errs[len(errs) // 2] < 6e-2 and errs[-1] < 0.1, errs


def test_ica_layernorm_eval_equals_training_math():
    from dinunet_implementations_amd.ops.head import HeadSpec, head_loss
    torch.manual_seed(5)
    head = _ica_head().to(DEV)
    x = torch.randn(7, 384, device=DEV)
    y = torch.randint(0, 2, (7,), device=DEV)
    res = []
    for train in (True, False):
        head.train(train)
        spec = HeadSpec(list(head))
        assert spec.ok and spec.supported(x)
        with torch.no_grad():
            res.append(head_loss(x, spec, y, log_out=False))
    for a, b in zip(res[0], res[1]):  # the same launches run: bitwise
        assert torch.equal(a, b)
    head.eval()
    from dinunet_implementations_amd.ops import reference as ref
    with torch.no_grad():
        ro, rl, _ = ref.softmax_ce(_emulated(list(head), x), y)
    assert rel(res[1][0], ro) < 2e-2
    assert abs(res[1][1].item() - rl.item()) < 2e-2 * max(1.0, abs(rl.item()))


def _steps(B, p, variants):
    """Two accumulating training steps of the ICA head per variant ``(hinted, one_launch)`` from
    identical state and the same dropout seed; returns per variant (out, loss, pred, dx, grads)."""
    from dinunet_implementations_amd.ops import head as H
    torch.manual_seed(11)
    base = list(_ica_head(p=p).to(DEV).train())
    with torch.no_grad():
        base[2].weight.uniform_(0.5, 1.5)
        base[2].bias.uniform_(-0.3, 0.3)
    x = torch.randn(B, 384, device=DEV)
    y = torch.randint(0, 2, (B,), device=DEV)
    one = torch.ones((), device=DEV)
    res, seed0 = [], None
    for hinted, one_launch in variants:
        ms = [copy.deepcopy(m) for m in base]
        old = H._HEAD_STEP
        H._HEAD_STEP = one_launch
        try:
            spec = H.HeadSpec(ms)
            assert spec.ok and spec.supported(x)
            r = spec.rng(x.device)
            if seed0 is None:
                seed0 = r.clone()
            else:
                r.copy_(seed0)
            for _ in range(2):  # twice: the gradients accumulate
                xi = x.clone().requires_grad_()
                with H.loss_grad_hint(one if hinted else None):
                    out, loss, pred = H.head_loss(xi, spec, y, log_out=False)
                torch.autograd.backward(loss, one)
            torch.cuda.synchronize()
        finally:
            H._HEAD_STEP = old
        res.append((out.clone(), loss.clone(), pred.clone(), xi.grad.clone(),
                    [q.grad.clone() for m in ms for q in m.parameters()]))
    return res


def _flat(r):
    return list(r[:4]) + list(r[4])


@pytest.mark.parametrize("B,p", [(4, 0.0), (32, 0.0), (4, 0.25), (32, 0.25)])
def test_ica_layernorm_one_launch_matches_three_launch(B, p):
    """The hinted step runs head_rep.hip (one launch) and equals the three-launch path: both reduce
    rows and columns in the same order with the same roundings (head_common.h)."""
    from dinunet_implementations_amd.ops import head as H
    n0 = H.REP_LAUNCHES
    a, b = _steps(B, p, [(True, True), (True, False)])
    assert H.REP_LAUNCHES == n0 + 2, "the replicated head did not run"
    worst = 0.0
    for u, v in zip(_flat(a), _flat(b)):
        worst = max(worst, (u.double() - v.double()).abs().max().item())
        assert torch.allclose(u.double(), v.double(), rtol=1e-6, atol=0)
    print(f"  one-launch vs three-launch: max abs difference {worst:.3e}")
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in a[4])
    assert torch.equal(a[2], a[0].argmax(1))


@pytest.mark.parametrize("B,p", [(4, 0.0), (32, 0.25)])
def test_ica_layernorm_hinted_three_launch_bitwise(B, p):
    """With the one-launch step off, the hinted forward (output-gradient chain in the forward
    launch, vector gradients through the workspace stash) equals the unhinted launches bitwise."""
    a, b = _steps(B, p, [(True, False), (False, False)])
    for u, v in zip(_flat(a), _flat(b)):
        assert torch.equal(u, v)


def test_ica_layernorm_hinted_graph_replay():
    """The hinted LayerNorm step captured in a HIP graph; each replay with fresh inputs in the
    static buffers equals the eager step on that input."""
    from dinunet_implementations_amd.ops import head as H
    torch.manual_seed(14)
    mods = list(_ica_head().to(DEV).train())
    spec = H.HeadSpec(mods)
    params = [q for m in mods for q in m.parameters()]
    xs = torch.randn(32, 384, device=DEV, requires_grad=True)
    ys = torch.randint(0, 2, (32,), device=DEV)
    assert spec.ok and spec.supported(xs)
    one = torch.ones((), device=DEV)

    def run(x, y):
        with H.loss_grad_hint(one):
            out, loss, _ = H.head_loss(x, spec, y, log_out=False)
        torch.autograd.backward(loss, one)
        return out, loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    n0 = H.REP_LAUNCHES
    with torch.cuda.stream(s):
        for _ in range(2):
            run(xs, ys)
    torch.cuda.current_stream().wait_stream(s)
    assert H.REP_LAUNCHES == n0 + 2, "the replicated head did not run"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        so, sl = run(xs, ys)
    for i in range(2):
        xn = torch.randn(32, 384, device=DEV)
        yn = torch.randint(0, 2, (32,), device=DEV)
        with torch.no_grad():
            xs.copy_(xn)
            ys.copy_(yn)
        for q in params:
            q.grad.zero_()
        xs.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = (so.clone(), sl.clone(), xs.grad.clone(), [q.grad.clone() for q in params])
        for q in params:
            q.grad.zero_()
        xe = xn.clone().requires_grad_()
        eo, el = run(xe, yn)
        torch.cuda.synchronize()
        assert torch.equal(got[0], eo) and torch.equal(got[1], el), i
        assert torch.equal(got[2], xe.grad), i
        for u, q in zip(got[3], params):
            assert torch.equal(u, q.grad), i


@pytest.mark.parametrize("B", [32, 200])
def test_ica_layernorm_head_deterministic(B):
    from dinunet_implementations_amd.ops.head import HeadSpec, head_loss
    torch.manual_seed(6)
    head = _ica_head().to(DEV).train()
    x = torch.randn(B, 384, device=DEV)
    y = torch.randint(0, 2, (B,), device=DEV)
    runs = []
    for _ in range(2):
        m = copy.deepcopy(head)
        spec = HeadSpec(list(m))
        assert spec.ok and spec.supported(x)
        xi = x.clone().requires_grad_()
        _, loss, _ = head_loss(xi, spec, y, log_out=False)
        loss.backward()
        runs.append([xi.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    for u, v in zip(*runs):
        assert torch.equal(u, v)


def test_ica_layernorm_batch_independence():
    """The replica property: LayerNorm does not couple rows, so the gradient of a 32-row batch is
    the mean of the gradients of its two 16-row halves (each with its own mean loss)."""
    from dinunet_implementations_amd.ops.head import HeadSpec, head_loss
    torch.manual_seed(7)
    head = _ica_head().to(DEV).train()
    x = torch.randn(32, 384, device=DEV)
    y = torch.randint(0, 2, (32,), device=DEV)

    def grads(xb, yb):
        m = copy.deepcopy(head)
        spec = HeadSpec(list(m))
        assert spec.ok and spec.supported(xb)
        xi = xb.clone().requires_grad_()
        _, loss, _ = head_loss(xi, spec, yb, log_out=False)
        loss.backward()
        return xi.grad, [p.grad for p in m.parameters()]

    dx, full = grads(x, y)
    dxa, ga = grads(x[:16], y[:16])
    dxb, gb = grads(x[16:], y[16:])
    worst = rel(torch.cat([dxa, dxb]) / 2, dx)
    assert worst < 1e-2
    for (n, _), f, a, b in zip(head.named_parameters(), full, ga, gb):
        e = rel((a + b) / 2, f)
        worst = max(worst, e)
        assert e < 1e-2, n
    print(f"  halves vs full batch: worst rel {worst:.3e}")


@pytest.mark.parametrize("B", [32, 200])
def test_ica_layernorm_rank_dad_capture(B):
    """rank-dAD's (A, Delta) pairs come from the workspace images of the fused LayerNorm head:
    Delta^T A of every Linear is that layer's weight gradient (both are the same bf16 operands
    accumulated in fp32; only the summation order differs)."""
    from dinunet_implementations_amd.ops.capture import DADCapture
    from dinunet_implementations_amd.ops.head import HeadSpec, head_loss
    torch.manual_seed(8)
    head = _ica_head().to(DEV).train()
    spec = HeadSpec(list(head))
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


def test_ica_model_with_layernorm_runs_the_fused_head():
    from dinunet_implementations_amd.models import ICALstm
    torch.manual_seed(0)
    m = ICALstm(input_size=64, hidden_size=384, num_comps=20, window_size=10,
                norm_layer="layer").to(DEV).train()
    x = torch.randn(32, 12, 20, 10, device=DEV)
    y = torch.randint(0, 2, (32,), device=DEV)
    feat = torch.zeros(32, m.classifier[1].in_features, device=DEV)
    assert m.head_spec().ok and m.head_spec().supported(feat)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        _, loss, _ = m.forward_loss(x, y)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0], losses
