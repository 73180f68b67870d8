"""Does a NaN or an infinity that appears anywhere in a step reach the loss and the gradient norm?

The fused Adam skips an update whose global gradient norm is not finite, secure aggregation turns a
poisoned site's mean into NaN and top-k ships a NaN first: all of it presumes that no kernel on the
way swallows the value.  ``fmaxf(v, 0)`` does (it returns 0 for NaN), and so does a row maximum or
an argmax written with ``>`` alone.  Every assertion here is a set (which elements are non-finite)
or a bit pattern; none needs a tolerance.  The rules are torch's in the forward (``relu(NaN)`` is
NaN, a batch-statistics BatchNorm spreads a NaN over its column, LayerNorm and the softmax over its
row, ``argmax`` returns the first NaN) and the kernels' declared keep mask ``a > 0`` in the backward
(``tests/head_ref.py``).

(1) The fused heads (``mlp_head.hip`` at 17 rows, ``head_big.hip`` at 129 rows with a last row
block of one row, ``head_rep.hip`` at 17 rows) with one poisoned element of ``x``, a weight, a
bias or a norm ``gamma`` against the fp64 reference; rows a poisoned ``x`` cannot reach are the
clean run's bits.  (2) ``dn_softmax_xent(_lw)``, ``layernorm.hip`` and the ReLU-backward mask
kernels of ``elementwise.hip`` called directly (``dn_relu_bwd_colsum`` has no other test: the
encoder of every model has ``N * O % 8 == 0``).  (3) A whole training step of the ICA model with
one poisoned element: the loss and the gradient norm are non-finite and the update is skipped,
bit for bit, eager and captured, wherever the same model on the CPU in fp32 has a non-finite loss.

Run on one MI355X against the kernels as they were before this file: every head case failed (102
three-launch, 18 one-launch).  With ``fmaxf`` as the ReLU a poisoned ``x``, layer-0 weight, hidden
bias or ``gamma`` left ``out`` and the loss finite (ragged, 17 rows, ``x[1, 3] = nan``: no
non-finite element in ``out``, the loss or the images, against 5, 1, 50 and 19 in the reference),
and a poisoned last-layer weight left ``pred`` at the finite maximum on the rows with a NaN logit.
``head_big.hip``'s backward kept the gradient where ``gamma xhat + beta <= 0`` is false, so at a
NaN activation too, against the declared ``a > 0`` (``gb``, ``gbeta``, ``gW`` of the layers below
came out NaN where the rule says finite).  ``dn_softmax_xent`` wrote ``pred = 2147483647`` for an
all-NaN row and the finite maximum for a row with one NaN.  The whole step at every NaN site
reported a finite loss (0.72, about ``log 2``; 0.15 and 0.11 for the head weight and ``gamma``);
its gradient norm was NaN all the same, through the weight gradient of the poisoned layer, so the
update was skipped.  LayerNorm, the ReLU-backward kernels and the ``+inf`` / ``-inf`` softmax rows
passed unchanged.  ``+inf`` in an encoder weight is absorbed by the model itself (the LSTM gates
saturate, CPU loss 0.367): the loss is finite, the gradient norm is not, the step is skipped.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import head_ref as ref
import test_head_layers_gpu as hl

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NAN, INF = math.nan, math.inf


@pytest.fixture(autouse=True)
def _native():
    from dinunet_implementations_amd.ops import _lib
    if not _lib.native_available():
        pytest.fail("gfx950 kernel library not built")


def _nf(t):
    return ref.nonfinite(t)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_sets(pairs, what):
    """Every ``(name, kernel, reference)``: the same non-finite elements; all names reported."""
    bad = []
    for name, got, want in pairs:
        assert got is not None, f"{what} {name}: missing"
        a, b = _nf(got), _nf(want)
        assert a.shape == b.shape, (what, name, tuple(a.shape), tuple(b.shape))
        if not torch.equal(a, b):
            bad.append(f"{name}: kernel {int(a.sum())} non-finite, reference {int(b.sum())}")
    assert not bad, f"{what}: non-finite sets differ: {bad}"


# ---------------------------------------------------------------------------------------------
# (1) the fused heads

HEAD_B = (17, 129)      # mlp_head.hip; head_big.hip with a last row block of one row
ROW = 1                 # the row of the poisoned x


def _row_local(name, train):
    """No batch statistics on the way: a poisoned ``x[ROW]`` stays in its row."""
    return (not train) or not ref.has_train_bn(ref.make_head(name)[0])


def _check_forward(k, fw, case, what):
    layers, B = case["layers"], case["B"]
    C = layers[-1].out
    pairs = [("out", k["out"], fw["out"]), ("loss", k["loss"], fw["loss"])]
    if "A" in k:
        pairs += [(f"A{l}", k["A"][l][:B, :L.inp], fw["A"][l]) for l, L in enumerate(layers)]
    for l in range(len(layers)):
        if fw["rmean"][l] is not None:     # what nn.BatchNorm1d leaves: NaN in a poisoned column
            pairs += [(f"rmean{l}", k["rmean"][l], fw["rmean"][l]),
                      (f"rvar{l}", k["rvar"][l], fw["rvar"][l])]
    pred = k["pred"]
    in_range = bool(((pred >= 0) & (pred < C)).all())
    nan_rows = torch.isnan(fw["logits"]).any(1)
    print(f"{what}: loss {float(k['loss'])} ref {float(fw['loss'])}; {int(nan_rows.sum())} rows "
          f"with a NaN logit; pred in range {in_range}")
    _same_sets(pairs, what)
    assert in_range, f"{what}: pred outside [0, {C}): {pred.tolist()}"
    assert torch.equal(pred[nan_rows], fw["pred"][nan_rows]), f"{what}: pred on NaN rows"


def _check_backward(grads, fw, case, what):
    g = ref.backward(fw)
    want = ref.grad_tensors(case, g)
    got = dict(ref.grad_tensors(case, grads))
    _same_sets([(n, got.get(n), t) for n, t in want], what)
    if bool(_nf(fw["loss"])):       # the consequence that matters: the gradient norm sees it
        assert any(bool(_nf(t).any()) for n, t in got.items() if n != "dx"), \
            f"{what}: non-finite loss, every parameter gradient finite"


def _check_local(k, k0, case, train, what):
    """Every row but ``ROW`` is the clean run's, bit for bit."""
    B, layers = case["B"], case["layers"]
    keep = torch.arange(B) != ROW
    names = ["out", "pred"] + (["dx"] if train else [])
    for n in names:
        assert torch.equal(_bits(k[n])[keep], _bits(k0[n])[keep]), f"{what}: {n} off the row"
    if train:
        for l, L in enumerate(layers):
            a, a0 = k["A"][l][:B, :L.inp], k0["A"][l][:B, :L.inp]
            assert torch.equal(_bits(a)[keep], _bits(a0)[keep]), f"{what}: A{l} off the row"


@pytest.mark.parametrize("B", HEAD_B)
@pytest.mark.parametrize("name,train,label", ref.nonfinite_matrix())
def test_head_three_launch(name, train, label, B):
    clean, case, p = ref.poisoned(name, B, label)
    what = f"{hl._kernel_of(B)} {name} B={B} {'train' if train else 'eval'} {label}"
    k = hl._launch(case, train=train)
    fw = ref.forward(case, F64, ref.NONE, train=train)
    _check_forward(k, fw, case, what)
    if train:
        _check_backward(k["grads"], fw, case, what)
    if p[1] == "x" and _row_local(name, train):
        bad = _nf(fw["out"]).any(1)
        assert bad.tolist() == [r == ROW for r in range(B)]
        _check_local(k, hl._launch(clean, train=train), case, train, what)


@pytest.mark.parametrize("name,label", [(n, lab) for n, t, lab in ref.nonfinite_matrix()
                                        if t and n in ("ica", "ica_ln")])
def test_head_one_launch(name, label):
    """``dn_head_rep``, reached as ``test_one_launch_and_hinted_paths_bitwise`` reaches it."""
    B = 17
    clean, case, p = ref.poisoned(name, B, label)
    what = f"head_rep {name} B={B} {label}"
    ex, st, ran, spec = hl._via_head_loss(case, "rep")
    assert ran == 1, "the one-launch head did not run"
    layers = case["layers"]
    k = dict(out=ex[0], loss=ex[1], pred=ex[2], dx=ex[3])
    grads, it = dict(dx=ex[3], gW=[], gb=[], ggamma=[], gbeta=[]), iter(ex[4:])
    for L in layers:        # module order: Linear (weight, bias), norm (weight, bias)
        grads["gW"].append(next(it))
        grads["gb"].append(next(it) if L.bias else None)
        grads["ggamma"].append(next(it) if L.norm else None)
        grads["gbeta"].append(next(it) if L.norm else None)
    k["rmean"], k["rvar"] = [None] * len(layers), [None] * len(layers)
    sit = iter(st)
    for l, L in enumerate(layers):
        if L.norm == "bn_run":
            k["rmean"][l], k["rvar"][l], _ = next(sit), next(sit), next(sit)
    fw = ref.forward(case, F64, ref.NONE)
    _check_forward(k, fw, case, what)
    _check_backward(grads, fw, case, what)
    if p[1] == "x" and _row_local(name, True):
        ex0, _, ran0, _ = hl._via_head_loss(clean, "rep")
        assert ran0 == 1
        keep = torch.arange(B) != ROW
        for n, a, b in (("out", ex[0], ex0[0]), ("pred", ex[2], ex0[2]), ("dx", ex[3], ex0[3])):
            assert torch.equal(_bits(a)[keep], _bits(b)[keep]), f"{what}: {n} off the row"


# ---------------------------------------------------------------------------------------------
# (2a) dn_softmax_xent, dn_softmax_xent_lw

SOFTMAX_SHAPES = ((5, 2), (9, 3), (6, 70))      # 70: more than one class per lane
SOFTMAX_POISONS = ("one_nan", "all_nan", "one_inf", "two_inf", "all_ninf")


def _poison_row(z, kind):
    C = z.shape[1]
    c = 65 if C > 64 else C - 1     # 65: the second class of lane 1
    if kind == "one_nan":
        z[ROW, c] = NAN
    elif kind == "all_nan":
        z[ROW] = NAN
    elif kind == "one_inf":
        z[ROW, c] = INF
    elif kind == "two_inf":
        z[ROW, c] = INF
        z[ROW, min(3, C - 2)] = INF
    elif kind == "all_ninf":
        z[ROW] = -INF
    else:
        raise ValueError(kind)
    return z


def _softmax(z, y, log_out, block):
    from dinunet_implementations_amd.ops import _lib, heads  # noqa: F401 (registers the launchers)
    B, C = z.shape
    zd, yd = z.to(DEV), y.to(DEV)
    out = torch.full((B, C), 7.0, device=DEV)
    dz = torch.full((B, C), 7.0, device=DEV)
    loss = torch.full((), 7.0, device=DEV)
    pred = torch.full((B,), -5, dtype=torch.long, device=DEV)
    if block is None:
        _lib.call("dn_softmax_xent", zd.data_ptr(), yd.data_ptr(), B, C, int(log_out),
                  out.data_ptr(), dz.data_ptr(), loss.data_ptr(), pred.data_ptr(), _lib.stream())
    else:
        _lib.call("dn_softmax_xent_lw", zd.data_ptr(), yd.data_ptr(), B, C, int(log_out),
                  out.data_ptr(), dz.data_ptr(), loss.data_ptr(), pred.data_ptr(),
                  block.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return out.cpu(), dz.cpu(), loss.cpu(), pred.cpu()


@pytest.mark.parametrize("kind", SOFTMAX_POISONS)
@pytest.mark.parametrize("B,C", SOFTMAX_SHAPES)
def test_softmax_xent_kernels(B, C, kind):
    from dinunet_implementations_amd.ops import heads
    g = torch.Generator().manual_seed(100 * B + C)
    z0 = torch.randn(B, C, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    w = 0.5 + torch.rand(C, generator=g)
    z = _poison_row(z0.clone(), kind)
    keep = torch.arange(B) != ROW
    for lw in (False, True):
        block = heads.loss_block_values(w, 0.1, C).to(DEV) if lw else None
        z64 = z.double().requires_grad_()
        kw = dict(weight=w.double(), label_smoothing=0.1) if lw else {}
        loss64 = F.cross_entropy(z64, y, **kw)
        loss64.backward()
        pred64 = z64.detach().argmax(1)
        for log_out in (0, 1):
            what = f"softmax_xent{'_lw' if lw else ''} {B}x{C} {kind} log_out={log_out}"
            out64 = (F.log_softmax if log_out else F.softmax)(z64.detach(), 1)
            out, dz, loss, pred = _softmax(z, y, log_out, block)
            print(f"{what}: loss {float(loss)} ref {float(loss64)} pred[{ROW}] {int(pred[ROW])} "
                  f"ref {int(pred64[ROW])}")
            _same_sets([("out", out, out64), ("dz", dz, z64.grad), ("loss", loss, loss64)], what)
            assert bool(_nf(loss)) and bool(_nf(out[ROW]).all())
            assert torch.equal(pred, pred64), f"{what}: pred {pred.tolist()}"
            c_out, c_dz, _, c_pred = _softmax(z0, y, log_out, block)
            assert torch.equal(_bits(out)[keep], _bits(c_out)[keep]), what
            assert torch.equal(_bits(dz)[keep], _bits(c_dz)[keep]), what
            assert torch.equal(pred[keep], c_pred[keep]), what


# ---------------------------------------------------------------------------------------------
# (2b) layernorm.hip

# D -> 16-byte vectors per lane K = 1, 2 (a ragged last group of one vector) and 8; 4100 rows: a
# workgroup takes a second row in the grid-stride loop (1024 workgroups of 4 rows)
LN_SHAPES = ((5, 12, 2), (9, 260, 2), (6, 2048, 2), (4100, 64, 4097))


def _layer_norm(x, w, b, gdy):
    """Forward and backward through the kernels with ``dy = y * gdy`` (a non-finite row of ``y``
    hands a non-finite ``dy`` row back, as a loss that reads ``y`` would)."""
    from dinunet_implementations_amd.ops.layernorm import fused_ok, layer_norm
    xd = x.to(DEV).requires_grad_()
    wd, bd = w.to(DEV).requires_grad_(), b.to(DEV).requires_grad_()
    assert fused_ok(xd, x.shape[1])
    y = layer_norm(xd, wd, bd)
    mean, rstd = (t.detach().cpu() for t in y.grad_fn.saved_tensors[2:4])
    y.backward(y.detach() * gdy.to(DEV))
    torch.cuda.synchronize()
    return [t.detach().cpu() for t in (y, xd.grad, wd.grad, bd.grad)] + [mean, rstd]


@pytest.mark.parametrize("kind", ["nan", "inf", "nan_and_inf"])
@pytest.mark.parametrize("R,D,row", LN_SHAPES)
def test_layernorm_kernels(R, D, row, kind):
    g = torch.Generator().manual_seed(R + D)
    x0 = torch.randn(R, D, generator=g)
    w, b = 0.5 + torch.rand(D, generator=g), torch.randn(D, generator=g)
    gdy = torch.randn(R, D, generator=g)
    x = x0.clone()
    if "nan" in kind:
        x[row, 1] = NAN
    if "inf" in kind:
        x[row, D - 1] = INF
    y, dx, dg, db, mean, rstd = _layer_norm(x, w, b, gdy)
    y0, dx0, dg0, db0, mean0, rstd0 = _layer_norm(x0, w, b, gdy)
    for t in (y0, dx0, dg0, db0, mean0, rstd0):
        assert bool(torch.isfinite(t).all())
    # torch's own answer, in fp64: the whole row, and through it every column's parameter gradient
    x64 = x.double().requires_grad_()
    w64, b64 = w.double().requires_grad_(), b.double().requires_grad_()
    y64 = F.layer_norm(x64, (D,), w64, b64, 1e-5)
    y64.backward(y64.detach() * gdy.double())
    what = f"layernorm {R}x{D} {kind}"
    _same_sets([("y", y, y64), ("dx", dx, x64.grad), ("dgamma", dg, w64.grad),
                ("dbeta", db, b64.grad)], what)
    only = [r == row for r in range(R)]
    assert _nf(y).all(1).tolist() == only and _nf(dx).all(1).tolist() == only
    assert _nf(mean).tolist() == only and _nf(rstd).tolist() == only
    assert bool(_nf(dg).all()) and bool(_nf(db).all())
    keep = torch.arange(R) != row
    assert torch.equal(_bits(y)[keep], _bits(y0)[keep])
    assert torch.equal(_bits(dx)[keep], _bits(dx0)[keep])
    assert torch.equal(_bits(mean)[keep], _bits(mean0)[keep])
    assert torch.equal(_bits(rstd)[keep], _bits(rstd0)[keep])


# ---------------------------------------------------------------------------------------------
# (2c) dn_relu_bwd, dn_relu_bwd_colsum

# (65, 257): two column strips and the slab edge (64 slabs of 2 rows, the last ones empty);
# (8, 256), (200, 264): the 16-byte vector branch, which ops.linear never routes here
RELU_SHAPES = ((5, 3), (64, 7), (65, 257), (8, 256), (200, 264), (700, 12))


def _relu_case(N, O):
    """bf16 ``dy`` of small integers and ``y = relu(randn)``: ``dym`` and the fp32 column sums
    (at most 700 * 4) are exact, so the comparison with fp64 is bitwise."""
    g = torch.Generator().manual_seed(1000 * N + O)
    dy = torch.randint(-4, 5, (N, O), generator=g).to(BF16)
    y = torch.relu(torch.randn(N, O, generator=g)).to(BF16)
    db0 = torch.randint(-9, 10, (O,), generator=g).float()
    return dy, y, db0


def _relu_ref(dy, y, db0, accumulate):
    dym = torch.where(y.double() > 0, dy.double(), torch.zeros((), dtype=F64))
    db = dym.sum(0) + (db0.double() if accumulate else 0.0)
    return dym.to(BF16), db.float()


def _relu_bwd_colsum(dy, y, db0, accumulate):
    from dinunet_implementations_amd.ops import _lib, linear  # noqa: F401 (registers the launchers)
    N, O = dy.shape
    dyd, yd = dy.to(DEV).contiguous(), y.to(DEV).contiguous()
    dym = torch.full((N, O), 7.0, dtype=BF16, device=DEV)
    db = db0.to(DEV).clone()
    n_ws = _lib.lib().dn_relu_bwd_colsum_workspace
    n_ws.restype = _lib.c_long
    n_ws.argtypes = [_lib.c_int, _lib.c_int]
    ws = torch.full((int(n_ws(N, O)),), NAN, device=DEV)
    _lib.call("dn_relu_bwd_colsum", dyd.data_ptr(), yd.data_ptr(), dym.data_ptr(), db.data_ptr(),
              ws.data_ptr(), N, O, int(accumulate), _lib.stream())
    torch.cuda.synchronize()
    return dym.cpu(), db.cpu()


def _relu_bwd(dy, y):
    from dinunet_implementations_amd.ops import _lib, linear  # noqa: F401
    dyd, yd = dy.to(DEV).contiguous(), y.to(DEV).contiguous()
    dym = torch.full(dy.shape, 7.0, dtype=BF16, device=DEV)
    _lib.call("dn_relu_bwd", dyd.data_ptr(), yd.data_ptr(), dym.data_ptr(), dy.numel(),
              _lib.stream())
    torch.cuda.synchronize()
    return dym.cpu()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("N,O", RELU_SHAPES)
def test_relu_backward_kernels_are_exact(N, O, accumulate):
    dy, y, db0 = _relu_case(N, O)
    want_m, want_b = _relu_ref(dy, y, db0, accumulate)
    assert 0 < int((y > 0).sum()) < y.numel()
    dym, db = _relu_bwd_colsum(dy, y, db0, accumulate)
    assert torch.equal(_bits(dym), _bits(want_m)), "dym"
    assert torch.equal(_bits(db), _bits(want_b)), "db"
    if (N * O) % 8 == 0:
        assert torch.equal(_bits(_relu_bwd(dy, y)), _bits(want_m)), "dn_relu_bwd"


@pytest.mark.parametrize("N,O", [(5, 3), (8, 256), (65, 257)])
def test_relu_backward_mask_rule(N, O):
    """The keep mask is ``y > 0``: a NaN in ``y`` keeps no gradient (not even a NaN one); a NaN in
    ``dy`` at a kept position stays NaN in ``dym`` and in its column's ``db``, and only there."""
    dy, y, db0 = _relu_case(N, O)
    kept = torch.nonzero(y > 0)
    (r1, c1), (r2, c2) = kept[0].tolist(), kept[-1].tolist()
    assert c1 != c2
    y[r1, c1] = NAN             # was kept: now it is not
    dy[r1, c1] = NAN
    dy[r2, c2] = NAN            # kept, and NaN
    want_m, want_b = _relu_ref(dy, y, db0, 1)
    assert float(want_m[r1, c1]) == 0.0 and math.isnan(float(want_m[r2, c2]))
    assert _nf(want_b).tolist() == [c == c2 for c in range(O)]
    dym, db = _relu_bwd_colsum(dy, y, db0, 1)
    fin = torch.isfinite(want_m)
    assert torch.equal(_nf(dym), ~fin) and torch.equal(_bits(dym)[fin], _bits(want_m)[fin])
    finb = torch.isfinite(want_b)
    assert torch.equal(_nf(db), ~finb) and torch.equal(_bits(db)[finb], _bits(want_b)[finb])
    if (N * O) % 8 == 0:
        d2 = _relu_bwd(dy, y)
        assert torch.equal(_nf(d2), ~fin) and torch.equal(_bits(d2)[fin], _bits(want_m)[fin])


def test_linear_bias_relu_takes_the_colsum_kernel():
    """``N * O % 8 != 0`` (9 x 7 from a 9 x 5 input) routes ``ops.linear`` to
    ``dn_relu_bwd_colsum``: both gradients against the bf16-rounded torch reference, within
    ``test_linear_bias_relu_grad``'s tolerance."""
    from dinunet_implementations_amd.ops import linear_bias_relu
    from test_kernels_gpu import bf, rel
    g = torch.Generator().manual_seed(3)
    x = torch.randn(9, 5, generator=g).to(DEV)
    w = (torch.randn(7, 5, generator=g) * 0.5).to(DEV).requires_grad_()
    b = (torch.randn(7, generator=g) * 0.1).to(DEV).requires_grad_()
    y = linear_bias_relu(x, w, b)
    assert (y.numel() % 8) != 0
    wr, br = bf(w.detach()).requires_grad_(), b.detach().clone().requires_grad_()
    yr = torch.relu(bf(x) @ wr.t() + br)
    assert rel(y, yr) < 1e-2
    gy = torch.randn(9, 7, generator=g).to(DEV)
    (y.float() * gy).sum().backward()
    (yr * gy).sum().backward()
    torch.cuda.synchronize()
    print("rel gW", rel(w.grad, wr.grad), "rel gb", rel(b.grad, br.grad))
    assert rel(w.grad, wr.grad) < 2e-2 and rel(b.grad, br.grad) < 2e-2


# ---------------------------------------------------------------------------------------------
# (3) end to end: the step is skipped

SITES = ("input", "encoder_weight", "W_hh", "W_ih", "head_weight", "norm_gamma")


def _model():
    from dinunet_implementations_amd.models import ICALstm
    m = ICALstm(input_size=64, hidden_size=128, num_comps=20, window_size=10)
    m.classifier[0].p = 0.0
    return m


def _trainer(use_graph):
    """The ICA trainer of ``test_topk_gpu._trainer`` on the plain dSGD engine at one site, with
    clipping on at a threshold that never bites."""
    from dinunet_implementations_amd.ops import FlatParams, FusedAdam
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    from dinunet_implementations_amd.runtime.step import TrainStep
    torch.manual_seed(0)
    m = _model().cuda().train()
    flat = FlatParams(m.parameters())
    opt = FusedAdam(flat, lr=1e-3, max_grad_norm=1e30)
    eng = make_engine("dSGD", m, flat, SiteGroup(device=torch.device("cuda")),
                      {"precision_bits": "32"})
    step = TrainStep(m, flat, opt, eng, task="ica", use_graph=use_graph)
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn(8, 12, 20, 10, device="cuda", generator=g).bfloat16().float()
    y = torch.randint(0, 2, (8,), device="cuda", generator=g)
    for _ in range(5 if use_graph else 1):      # clean steps first (the fourth call captures)
        step(x, y)
    torch.cuda.synchronize()
    if use_graph:
        assert step.graph is not None and step.graph_opt
    return dict(m=m, flat=flat, opt=opt, step=step, x=x, y=y)


@pytest.fixture(scope="module")
def eager_trainer():
    return _trainer(False)


@pytest.fixture(scope="module")
def graph_trainer():
    return _trainer(True)


def _site(m, site):
    """``(parameter, index)`` of a poison site (``None`` for the input batch)."""
    return {"input": (None, (2, 3, 4, 5)),
            "encoder_weight": (m.encoder[0].weight, (5, 7)),
            "W_hh": (m.lstm.lstms[0].h2h.weight, (3, 2)),
            "W_ih": (m.lstm.lstms[1].i2h.weight, (4, 6)),
            "head_weight": (m.classifier[4].weight, (1, 2)),
            "norm_gamma": (m.classifier[2].weight, (9,))}[site]


def _cpu_loss(T, site, value):
    """The loss of the same model on the CPU in fp32 (reference math) with the same poison."""
    m = _model().train()
    m.load_state_dict({k: v.detach().cpu() for k, v in T["m"].state_dict().items()})
    m.use_fused = False
    m.lstm.use_fused = False
    x = T["x"].cpu().clone()
    p, idx = _site(m, site)
    with torch.no_grad():
        if p is None:
            x[idx] = value
        else:
            p[idx] = value
        return float(m.forward_loss(x, T["y"].cpu())[1])


def _poisoned_step(T, site, value):
    m, flat, opt, step = T["m"], T["flat"], T["opt"], T["step"]
    want = _cpu_loss(T, site, value)
    torch.cuda.synchronize()
    bn = m.classifier[2]
    stats = [t.clone() for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
    before = [t.clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)]
    skipped, count = int(opt.skipped_steps), opt.step_count
    p, idx = _site(m, site)
    x = T["x"]
    orig = None if p is None else p.data[idx].clone()
    try:
        if p is None:
            x = x.clone()
            x[idx] = value
        else:
            p.data[idx] = value         # a view of flat.data: poisoned in place
            assert int(_nf(flat.data).sum()) == 1
        loss = float(step(x, T["y"]))
        torch.cuda.synchronize()
        G = float(opt.grad_norm)
        now_skipped = int(opt.skipped_steps)
    finally:
        if p is not None:
            p.data[idx] = orig
        with torch.no_grad():
            for t, s in zip((bn.running_mean, bn.running_var, bn.num_batches_tracked), stats):
                t.copy_(s)
    after = [t.clone() for t in (flat.data, opt.exp_avg, opt.exp_avg_sq)]
    print(f"{site}={value}: CPU loss {want}, loss {loss}, G {G}, "
          f"skipped {now_skipped - skipped}")
    # one clean step: the parameters move and stay finite (whatever the poisoned one did)
    step(T["x"], T["y"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flat.data).all())
    assert not torch.equal(flat.data, after[0])
    assert opt.step_count == count + 2
    return want, loss, G, now_skipped - skipped, before, after


def _assert_skipped(res, what):
    want, loss, G, skipped, before, after = res
    assert not math.isfinite(want), f"{what}: the CPU model's loss is finite"
    assert not math.isfinite(loss), f"{what}: loss {loss}"
    assert not math.isfinite(G), f"{what}: gradient norm {G}"
    assert skipped == 1, f"{what}: skipped {skipped}"
    for n, a, b in zip(("flat.data", "exp_avg", "exp_avg_sq"), after, before):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: {n} changed"


@pytest.mark.parametrize("site", SITES)
def test_nan_step_is_skipped_eager(eager_trainer, site):
    _assert_skipped(_poisoned_step(eager_trainer, site, NAN), f"eager {site}=nan")


@pytest.mark.parametrize("site", ["input", "W_hh"])
def test_nan_step_is_skipped_captured(graph_trainer, site):
    graph = graph_trainer["step"].graph
    _assert_skipped(_poisoned_step(graph_trainer, site, NAN), f"captured {site}=nan")
    assert graph_trainer["step"].graph is graph       # a replay, not a new capture


@pytest.mark.parametrize("site", SITES)
def test_inf_step_is_skipped_where_the_model_says_so(eager_trainer, site):
    """``+inf`` at the same sites: asserted wherever the CPU model's loss is non-finite (a
    saturating gate can absorb an infinity: ``sigmoid(inf) = 1``)."""
    res = _poisoned_step(eager_trainer, site, INF)
    if math.isfinite(res[0]):
        print(f"eager {site}=inf: absorbed by the model (CPU loss {res[0]})")
        return
    _assert_skipped(res, f"eager {site}=inf")
