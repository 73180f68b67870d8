"""The reference of ``tests/head_ref.py`` held to account, on the CPU: against autograd through the
real modules in fp64, its masks path, its rounding switches, a second accumulation order, the
deliberately wrong references (each must break the rule of the GPU tests; the biased
``running_var`` and, at the layer seam, a batch row missing from ``gW`` do so under the older
whole-tensor bound of 2e-2, while a missing output row of ``gW`` or 8 missing columns of ``dx``
are several percent of the whole tensor at any width these heads have and break both), and the
conditions on the inputs that ``tests/
test_head_layers_gpu.py`` relies on."""
import math

import pytest
import torch
import torch.nn as nn

import head_ref as ref

F64 = torch.float64
OLD_BOUND = 2e-2      # the whole-tensor bound of tests/test_head_gpu.py
CPU_B = (2, 5, 17, 33)


def _loss_fn(case):
    from dinunet_implementations_amd.ops import reference as R
    fn = R.log_softmax_nll if case["log_out"] else R.softmax_ce
    kw = {}
    if case["class_weights"] is not None:
        kw = dict(weight=torch.tensor(case["class_weights"], dtype=F64),
                  label_smoothing=case["smoothing"])
    return lambda z: fn(z, case["y"], **kw)


def _module_grads(case, mods, x):
    """``forward`` / ``backward`` shaped results of autograd through ``mods``."""
    layers = case["layers"]
    lins = [m for m in mods if isinstance(m, nn.Linear)]
    out, loss, pred = _loss_fn(case)(nn.Sequential(*mods)(x))
    loss.backward()
    g = dict(dx=x.grad, gW=[m.weight.grad for m in lins],
             gb=[m.bias.grad if m.bias is not None else None for m in lins],
             ggamma=[None] * len(layers), gbeta=[None] * len(layers))
    norms = iter(m for m in mods if isinstance(m, (nn.BatchNorm1d, nn.LayerNorm)))
    fw = dict(out=out.detach(), loss=loss.detach(), pred=pred, case=case,
              rmean=[None] * len(layers), rvar=[None] * len(layers), nbt=[None] * len(layers))
    for l, L in enumerate(layers):
        if L.norm:
            m = next(norms)
            g["ggamma"][l], g["gbeta"][l] = m.weight.grad, m.bias.grad
            if L.norm == "bn_run":
                fw["rmean"][l], fw["rvar"][l] = m.running_mean, m.running_var
                fw["nbt"][l] = int(m.num_batches_tracked)
    return fw, g


def _agree(fw_a, g_a, fw_b, g_b, dz64, tol=1e-12):
    layers = fw_b["case"]["layers"]
    for (name, kind, a), (_, _, b) in zip(ref.tensors(fw_a, g_a), ref.tensors(fw_b, g_b)):
        assert ref.slice_err(a, b, kind) <= tol, name
        assert ref.whole_err(a, b) <= tol, name
    for l in range(len(layers)):   # exact value zero: absolute, against the size of its terms
        if ref.bias_before_bn(layers, l):
            scale = float(dz64[l].abs().sum(0).max())
            assert float((g_a["gb"][l] - g_b["gb"][l]).abs().max()) <= tol * scale
    assert torch.equal(fw_a["pred"], fw_b["pred"])
    assert fw_a["nbt"] == fw_b["nbt"]


@pytest.mark.parametrize("opts", [False, True])
@pytest.mark.parametrize("name", ref.HEADS)
def test_matches_autograd_through_modules(name, opts):
    for B in CPU_B:
        case = ref.make_case(name, B, seed=1, loss_opts=opts)
        if B == 2 and ref.has_train_bn(case["layers"]):
            # two rows under batch statistics: xhat = +-(1 - 2 eps / d^2), and the BatchNorm
            # backward cancels to that fraction of dy -- 1e-12 is then beyond fp64 itself
            continue
        mods = [m for m in ref.modules(case, F64) if not isinstance(m, nn.Dropout)]
        for m in mods:
            m.train()
        x = case["x"].double().requires_grad_()
        fw_m, g_m = _module_grads(case, mods, x)
        fw = ref.forward(case, F64)
        g = ref.backward(fw)
        _agree(fw, g, fw_m, g_m, g["dZ"])


@pytest.mark.parametrize("norm_layer,name", [("batch", "fs"), ("layer", "fs_ln")])
def test_fs_matches_msannet(norm_layer, name):
    """The ``fs`` heads are ``MSANNet(66, [72, 40, 24], 2)``."""
    from dinunet_implementations_amd.models import MSANNet
    case = ref.make_case(name, 9)
    net = MSANNet(66, [72, 40, 24], 2, norm_layer=norm_layer).double().train()
    lins = [blk[0] for blk in net.layers] + [net.fc_out]
    with torch.no_grad():
        for l, (lin, p) in enumerate(zip(lins, case["params"])):
            lin.weight.copy_(p["W"])
            if p["b"] is not None:
                lin.bias.copy_(p["b"])
            if p["gamma"] is not None:
                net.layers[l][1].weight.copy_(p["gamma"])
                net.layers[l][1].bias.copy_(p["beta"])
    assert net.layers[0][1].eps == ref.EPS
    x = case["x"].double().requires_grad_()
    out, loss, pred = net.forward_loss(x, case["y"])
    loss.backward()
    fw = ref.forward(case, F64)
    g = ref.backward(fw)
    assert ref.slice_err(fw["out"], out.detach(), "rows") <= 1e-12
    assert ref.slice_err(g["dx"], x.grad, "rows") <= 1e-12
    for l, lin in enumerate(lins):
        assert ref.slice_err(g["gW"][l], lin.weight.grad, "gW") <= 1e-12
    for l in range(3):
        assert ref.slice_err(g["ggamma"][l], net.layers[l][1].weight.grad, "feat") <= 1e-12


def test_eval_uses_running_statistics():
    case = ref.make_case("ica", 20)
    mods = ref.modules(case, F64)
    for m in mods:
        m.eval()
    with torch.no_grad():
        out, loss, pred = _loss_fn(case)(nn.Sequential(*mods)(case["x"].double()))
    fw = ref.forward(case, F64, train=False)
    assert ref.slice_err(fw["out"], out, "rows") <= 1e-12
    assert ref.slice_err(fw["loss"], loss, "scalar") <= 1e-12
    assert fw["rmean"][0] is None and fw["nbt"][0] is None


# ---------------------------------------------------------------------------------------------
# masks

def _random_masks(case, fw, seed=5):
    """The reference's own ReLU masks times a seeded dropout keep, scaled by ``1/(1-p)``."""
    g = torch.Generator().manual_seed(seed)
    masks = []
    for L, own in zip(case["layers"], fw["own_masks"]):
        m = own
        if L.drop:
            keep = (torch.rand(case["B"], L.inp, generator=g) >= L.drop).double() / (1 - L.drop)
            m = keep if m is None else m * keep
        masks.append(m)
    return masks


@pytest.mark.parametrize("name", ref.HEADS)
def test_own_masks_change_nothing(name):
    case = ref.make_case(name, 17)
    for dtype, rnd in ((F64, ref.NONE), (torch.float32, ref.KERNEL)):
        fw = ref.forward(case, dtype, rnd)
        fm = ref.forward(case, dtype, rnd, masks=fw["own_masks"])
        g, gm = ref.backward(fw), ref.backward(fm)
        for (n, _, a), (_, _, b) in zip(ref.tensors(fw, g), ref.tensors(fm, gm)):
            assert torch.equal(a, b), n


@pytest.mark.parametrize("name", ["ica_drop", "ica_ln", "fs_drop"])
def test_dropout_masks_match_autograd(name):
    """With given masks (ReLU of the mask-free run times a dropout keep) the hand-written
    backward is autograd through ``value * mask`` at every layer input."""
    case = ref.make_case(name, 17)
    masks = _random_masks(case, ref.forward(case, F64))
    fw = ref.forward(case, F64, masks=masks)
    g = ref.backward(fw)
    x = case["x"].double().requires_grad_()
    mods = [m for m in ref.modules(case, F64) if not isinstance(m, (nn.Dropout, nn.ReLU))]
    for m in mods:
        m.train()
    v, l = x, -1
    for m in mods:
        if isinstance(m, nn.Linear):
            l += 1
            if masks[l] is not None:
                v = v * masks[l]
        v = m(v)
    out, loss, _ = _loss_fn(case)(v)
    loss.backward()
    lins = [m for m in mods if isinstance(m, nn.Linear)]
    assert ref.slice_err(fw["out"], out.detach(), "rows") <= 1e-12
    assert ref.slice_err(g["dx"], x.grad, "rows") <= 1e-12
    for l, lin in enumerate(lins):
        assert ref.slice_err(g["gW"][l], lin.weight.grad, "gW") <= 1e-12
    norms = [m for m in mods if isinstance(m, (nn.BatchNorm1d, nn.LayerNorm))]
    gg = [t for t in g["ggamma"] if t is not None]
    for a, m in zip(gg, norms):
        assert ref.slice_err(a, m.weight.grad, "feat") <= 1e-12


# ---------------------------------------------------------------------------------------------
# non-finite values

def _poisoned_chain(case, train):
    """The poisoned case through the plain modules in fp64 with autograd (training) on."""
    mods = [m for m in ref.modules(case, F64) if not isinstance(m, nn.Dropout)]
    for m in mods:
        m.train(train)
    x = case["x"].double().requires_grad_(train)
    with torch.set_grad_enabled(train):
        logits = nn.Sequential(*mods)(x)
        out, loss, _ = _loss_fn(case)(logits)
    g = None
    if train:
        loss.backward()
        lins = [m for m in mods if isinstance(m, nn.Linear)]
        n = len(lins)
        g = dict(dx=x.grad, gW=[m.weight.grad for m in lins],
                 gb=[m.bias.grad if m.bias is not None else None for m in lins],
                 ggamma=[None] * n, gbeta=[None] * n)
        norms = iter(m for m in mods if isinstance(m, (nn.BatchNorm1d, nn.LayerNorm)))
        for l, L in enumerate(case["layers"]):
            if L.norm:
                nm = next(norms)
                g["ggamma"][l], g["gbeta"][l] = nm.weight.grad, nm.bias.grad
    state = [(m.running_mean, m.running_var) for m in mods
             if isinstance(m, nn.BatchNorm1d) and m.track_running_stats]
    return logits.detach(), out.detach(), loss.detach(), g, state


def test_poison_leaves_the_case_alone():
    case = ref.poison_case("ica", 5)
    before = [case["x"].clone()] + [p["W"].clone() for p in case["params"]]
    for _, where, v, l, i, k in ref.poisons("ica"):
        c = ref.poison(case, where, v, l, i, k)
        t = c["x"] if where == "x" else c["params"][l][where]
        assert int(ref.nonfinite(t).sum()) == 1
        got = t[i, k] if t.dim() == 2 else t[i]
        assert math.isnan(v) and math.isnan(float(got)) or float(got) == v
    for a, b in zip(before, [case["x"]] + [p["W"] for p in case["params"]]):
        assert torch.equal(a, b)
    assert all(bool(torch.isfinite(p[k]).all()) for p in case["params"] for k in p
               if p[k] is not None)
    with pytest.raises(ValueError):
        ref.poison(ref.poison_case("ragged", 5), "gamma", math.nan)


@pytest.mark.parametrize("name,train,label", ref.nonfinite_matrix())
def test_poisoned_forward_matches_the_modules(name, train, label):
    """Where a NaN or an infinity goes in the reference's forward is where torch's modules take
    it: the same non-finite elements of ``out``, ``loss`` and the new running statistics;
    ``pred`` is the argmax of the logits the chain ends in (NaN the largest, the first one wins),
    which on every row whose ``out`` is finite is the argmax of ``out`` as well (a row of ``out``
    with a NaN logit is all NaN: its argmax, 0, says nothing)."""
    for B in (5, 17):
        clean, case, _ = ref.poisoned(name, B, label)
        logits, out, loss, _, state = _poisoned_chain(case, train)
        fw = ref.forward(case, F64, ref.NONE, train=train)
        assert torch.equal(ref.nonfinite(fw["logits"]), ref.nonfinite(logits))
        assert torch.equal(ref.nonfinite(fw["out"]), ref.nonfinite(out))
        assert bool(ref.nonfinite(fw["loss"])) == bool(ref.nonfinite(loss))
        assert bool(ref.nonfinite(loss)), "every poison of the matrix reaches the loss"
        assert torch.equal(fw["pred"], logits.argmax(1))
        ok = torch.isfinite(out).all(1)
        assert torch.equal(fw["pred"][ok], out.argmax(1)[ok])
        if train:
            got = [(a, b) for a, b in zip(fw["rmean"], fw["rvar"]) if a is not None]
            assert len(got) == len(state)
            for (a, b), (c, d) in zip(got, state):
                assert torch.equal(ref.nonfinite(a), ref.nonfinite(c))
                assert torch.equal(ref.nonfinite(b), ref.nonfinite(d))
        if not train and label.startswith("x"):     # finite statistics: only the poisoned row
            bad = ref.nonfinite(fw["out"]).any(1)
            assert bad.tolist() == [r == 1 for r in range(B)]
            assert torch.equal(fw["out"][~bad], ref.forward(clean, F64, train=False)["out"][~bad])


@pytest.mark.parametrize("name,train,label",
                         [c for c in ref.nonfinite_matrix() if c[1]])
def test_poisoned_backward_follows_the_declared_mask_rule(name, train, label, record_property):
    """The backward keeps ``a > 0`` by a select, so it can only have FEWER non-finite gradients
    than autograd, whose ReLU backward passes the gradient on at a NaN output: the reference's
    non-finite set of every tensor is inside autograd's, the tensors where it is smaller are
    recorded (not enforced), and a non-finite loss still leaves a non-finite parameter gradient."""
    B = 17
    _, case, _ = ref.poisoned(name, B, label)
    _, _, loss, g_auto, _ = _poisoned_chain(case, True)
    fw = ref.forward(case, F64, ref.NONE)
    g = ref.backward(fw)
    differ = []
    for (n, a), (_, b) in zip(ref.grad_tensors(case, g), ref.grad_tensors(case, g_auto)):
        na, nb = ref.nonfinite(a), ref.nonfinite(b)
        assert bool((nb | ~na).all()), n
        if not torch.equal(na, nb):
            differ.append(n)
    print(f"{name} {label}: declared rule and autograd differ in {differ}")
    record_property("differ", ",".join(differ))
    assert bool(ref.nonfinite(loss))
    assert any(bool(ref.nonfinite(t).any()) for n, t in ref.grad_tensors(case, g) if n != "dx")


def test_relu_and_argmax_of_the_reference_keep_a_nan():
    """The two places a plain formula loses one: ``v * (v > 0)`` is NaN for ``-inf`` and
    ``max`` / ``argmax`` written with comparisons skip a NaN."""
    case = ref.poison_case("ragged", 5)
    c = ref.poison(case, "x", -math.inf, i=1, k=3)
    fw = ref.forward(c, F64)
    z0 = fw["Z"][0][1]
    assert bool((z0 == -math.inf).any()) and bool((z0 == math.inf).any())
    a1 = fw["A"][1][1]
    assert torch.equal(a1 == 0, z0 == -math.inf) and not bool(torch.isnan(a1).any())
    c = ref.poison(case, "b", math.nan, l=2, i=3)
    fw = ref.forward(c, F64)
    assert fw["pred"].tolist() == [3] * 5 and bool(torch.isnan(fw["loss"]))


# ---------------------------------------------------------------------------------------------
# roundings and accumulation order

@pytest.mark.parametrize("switch", ref.Rounding._fields)
def test_every_rounding_switch_changes_the_baseline(switch):
    case = ref.make_case("ica", 17, off_grid=switch == "w")
    res = []
    for rnd in (ref.KERNEL, ref.KERNEL._replace(**{switch: False})):
        fw = ref.forward(case, torch.float32, rnd)
        res.append((fw, ref.backward(fw)))
    (fa, ga), (fb, gb) = res
    assert not torch.equal(ga["dx"], gb["dx"])
    assert not torch.equal(ga["gW"][0], gb["gW"][0])
    if switch != "dz":
        assert not torch.equal(fa["out"], fb["out"])


@pytest.mark.parametrize("name", ref.HEADS)
def test_other_accumulation_order_stays_within_rule(name):
    for B in (17, 129):
        case, f64, g64, fb, gb = ref.solved(name, B)
        masks = f64["own_masks"]
        fb = ref.forward(case, torch.float32, ref.KERNEL, masks=masks)
        gb = ref.backward(fb)
        f2 = ref.forward(case, torch.float32, ref.KERNEL, masks=masks, mm=ref.mm_fp64)
        g2 = ref.backward(f2)
        for (n, kind, r), (_, _, a), (_, _, b) in zip(ref.tensors(f64, g64), ref.tensors(fb, gb),
                                                      ref.tensors(f2, g2)):
            ref.assert_close(b, r, a, kind, f"{name} B={B} {n}")


# ---------------------------------------------------------------------------------------------
# mutations: what the rule sees and the whole-tensor bound does not

# mutation -> (head, B, loss options, the tensor it must break, whether the whole-tensor error of
# that tensor stays under the old bound)
MUTANTS = {
    "biased_running_var": ("ica", 64, False, "rvar0", True),
    "bn_no_xhat_term": ("fs", 33, False, "gW0", False),
    "drop_no_scale": ("ica_drop", 33, False, "dx", False),
    "gW_last_batch_row": ("ica", 33, False, "gW0", False),
    "gW_last_out_row": ("ica", 33, False, "gW0", False),
    "dx_last8": ("wide", 33, False, "dx", False),
    "loss_div_B": ("ica", 33, True, "loss", False),
    "ln_rup32": ("ica_ln", 33, False, "out", False),
}
# mutations whose whole-tensor error stays under the old bound
UNSEEN = {"biased_running_var": ("ica", 64)}


def _mutant(name, B, opts, mut):
    case = ref.make_case(name, B, loss_opts=opts)
    f64 = ref.forward(case, F64)
    masks = _random_masks(case, f64)
    f64 = ref.forward(case, F64, masks=masks)
    fb = ref.forward(case, torch.float32, ref.KERNEL, masks=masks)
    fm = ref.forward(case, torch.float32, ref.KERNEL, masks=masks, mutate=mut)
    return (ref.tensors(f64, ref.backward(f64)), ref.tensors(fb, ref.backward(fb)),
            ref.tensors(fm, ref.backward(fm, mutate=mut)))


@pytest.mark.parametrize("mut", ref.MUTATIONS)
def test_mutation_breaks_the_rule(mut):
    name, B, opts, target, _ = MUTANTS[mut]
    broken = {}
    for (n, kind, r), (_, _, b), (_, _, m) in zip(*_mutant(name, B, opts, mut)):
        e_m, e_b = ref.slice_err(m, r, kind), ref.slice_err(b, r, kind)
        if not ref.within_rule(e_m, e_b):
            broken[n] = ref.whole_err(m, r)
    assert target in broken, (mut, sorted(broken))


@pytest.mark.parametrize("mut", sorted(UNSEEN))
def test_single_slice_mutation_is_invisible_to_the_whole_tensor_bound(mut):
    name, B = UNSEEN[mut]
    target = MUTANTS[mut][3]
    for (n, kind, r), (_, _, b), (_, _, m) in zip(*_mutant(name, B, False, mut)):
        if n == target:
            assert not ref.within_rule(ref.slice_err(m, r, kind), ref.slice_err(b, r, kind))
            assert ref.whole_err(m, r) < OLD_BOUND, ref.whole_err(m, r)
            return
    raise AssertionError(target)


def test_missing_batch_row_of_gW_is_seen_at_the_seam_only():
    """One batch row of 4100 missing from ``gW``: 1.5 % of every output row, under the old
    whole-tensor bound.  End to end that is within reach of the baseline's own bf16 error; at the
    seam ``gW = dZ^T A`` on saved images the baseline is fp32 accumulation and the rule sees it."""
    case = ref.make_case("ica", 4100)
    f64 = ref.forward(case, F64)
    g64 = ref.backward(f64)
    fb = ref.forward(case, torch.float32, ref.KERNEL, masks=f64["own_masks"])
    gm = ref.backward(fb, mutate="gW_last_batch_row")["gW"][0]
    assert ref.whole_err(gm, g64["gW"][0]) < OLD_BOUND
    dz, a = ref.bf(g64["dZ"][0]), ref.bf(f64["A"][0])     # "saved images"
    seam64 = dz.t() @ a
    base = dz.float().t() @ a.float()
    mut = dz.float()[:-1].t() @ a.float()[:-1]
    assert ref.whole_err(mut, seam64) < OLD_BOUND
    e_m, e_b = ref.slice_err(mut, seam64, "gW"), ref.slice_err(base, seam64, "gW")
    assert e_b < 1e-5 and not ref.within_rule(e_m, e_b)


# ---------------------------------------------------------------------------------------------
# conditions on the inputs of the GPU tests

@pytest.mark.parametrize("name", ref.HEADS)
def test_input_conditions(name):
    """No non-finite pre-activation; every hidden unit of ``ica``, ``fs`` and ``wide`` alive for
    at least one row (from 17 rows on: two rows leave a quarter of the units of a layer without
    a norm dead, and their exactly-zero ``gW`` rows are then part of the test); at most 10 % of
    rows (one row at the least) under the ``pred`` margin of the GPU tests."""
    for n, B in ref.matrix():
        if n != name:
            continue
        for opts in (False, True):
            case, f64, g64, fb, gb = ref.solved(name, B, None, opts)
            for z in f64["Z"]:
                assert bool(torch.isfinite(z).all())
            assert bool((case["x"].abs() >= 0.0625).all())
            if name in ("ica", "fs", "wide") and B >= 17:
                for l, m in enumerate(f64["own_masks"]):
                    if m is not None:
                        assert bool((m.sum(0) > 0).all()), (B, l)
            ok = ref.pred_margin(f64["out"], fb["out"])
            assert int((~ok).sum()) <= max(1, B // 10), (B, opts)    # the cap of the GPU test
            assert torch.equal(fb["pred"][ok], f64["pred"][ok])


def test_slice_err_zero_slices_and_shapes():
    r = torch.zeros(3, 4, dtype=F64)
    r[0] = 1.0
    g = r.clone()
    assert ref.slice_err(g, r, "gW") == 0.0 and ref.zero_slices(r, "gW") == [1, 2]
    g[2, 1] = 1e-30
    assert ref.slice_err(g, r, "gW") == math.inf
    g[2, 1] = math.nan
    assert math.isnan(ref.slice_err(g, r, "gW"))
    assert ref._slices(torch.arange(19.0), "feat").shape == (2, 16)
    with pytest.raises(ValueError):
        ref.slice_err(torch.zeros(2, 4), r, "gW")
    assert ref.within_rule(8 * ref.U23, 0.0) and not ref.within_rule(9 * ref.U23, 0.0)
