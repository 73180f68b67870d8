"""The fused classifier heads (``csrc/kernels/mlp_head.hip`` for B <= 64, ``head_big.hip`` above,
``head_rep.hip`` for the one-launch step) against the fp64 reference of ``tests/head_ref.py``, per
slice.

(a) End to end through ``dn_head_fwd_lw`` + ``dn_head_bwd_lw`` (what ``ops.head.head_loss``
calls), every case head of ``head_ref.matrix()``: ``out``, ``loss``, ``dx``, every parameter
gradient (accumulated into a seeded non-zero ``.grad`` pattern) and the running statistics are held
to ``E_kernel <= 8 max(E_base, 2^-23)``: ``E`` the largest relative 2-norm error against fp64 over
the slices of the tensor (one batch row, one output row of ``gW``, one block of 16 features),
``E_base`` that of the same formulas in fp32 on the CPU with the kernels' declared bf16 roundings.
Reference and baseline run with the kernel's own masks, read from its saved activation images;
(c) checks the masks themselves.  A slice that is exactly zero in the reference must be exactly
zero.  The gradient of a bias ahead of a batch-statistics BatchNorm (exactly zero) is bounded in
absolute terms (``head_ref.zero_bias_bound``).
(b) ``pred`` is the argmax of the kernel's ``out`` and the fp64 argmax wherever the fp64 margin
allows.  (d) Every layer seam on the kernel's own saved images, where the baseline is fp32
accumulation (about 1e-7): a wrong tile edge shows here.  The seam of ``gb`` against the column
sums of the ``dZ`` image is not taken: the kernels sum the fp32 values ahead of the bf16 cast
(``head_ref``'s docstring), which the image no longer holds; (a) holds ``gb`` per 16 features.
(e) The one-launch and hinted paths are bitwise the three-launch result.  (f) Two runs are
bitwise equal, on a zeroed workspace and on one filled with NaN patterns.  Both errors of every
tensor go to ``$DINUNET_ERR_LOG`` (jsonl) when set; ``profiles/head_kernel_errors.md`` is one
such run.

Measured on one MI355X (``profiles/head_kernel_errors.md``): 2326 compared tensors, the largest
ratio ``E_kernel / max(E_base, 2^-23)`` 1.87 (``gb`` of the one-layer head at 65 rows, both
errors below 1e-6), most 1.00 to two digits; no kernel changed.  Run once against the
deliberately wrong references of ``tests/head_ref.py`` (``MUTATIONS``), every end-to-end and seam
test a mutation reaches failed, bar the one-class head (all gradients zero) and one- and two-row
batches under batch statistics, where the baseline itself keeps few digits (the profile has the
counts).
"""
import functools
import json
import math
import os

import pytest
import torch

import head_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
SEED0 = 0x5EED0123


@pytest.fixture(autouse=True)
def _native():
    from dinunet_implementations_amd.ops import _lib
    if not _lib.native_available():
        pytest.fail("gfx950 kernel library not built")


def _record(kind, case, e_k, e_b):
    path = os.environ.get("DINUNET_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"kind": kind, "case": case, "e_kernel": float(f"{e_k:.4g}"),
                                "e_base": float(f"{e_b:.4g}")}) + "\n")


def _kernel_of(B):
    return "mlp_head" if B <= 64 else "head_big"


# ---------------------------------------------------------------------------------------------
# running the kernels

def _patterns(case, mods):
    """A seeded non-zero ``.grad`` for every parameter: bf16-valued, of the size of the gradient
    itself (the mask-free fp64 one), so that accumulating into it costs the comparison nothing."""
    _, _, g64, _, _ = ref.solved(case["name"], case["B"], None, case["class_weights"] is not None) \
        if case["name"] in ref.HEADS else (None, None, None, None, None)
    gen = torch.Generator().manual_seed(4242 + case["B"])
    pats = []
    lins = [m for m in mods if isinstance(m, torch.nn.Linear)]
    norms = iter(m for m in mods if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.LayerNorm)))
    for l, (L, lin) in enumerate(zip(case["layers"], lins)):
        ps = [("gW", lin.weight)] + ([("gb", lin.bias)] if L.bias else [])
        if L.norm:
            nm = next(norms)
            ps += [("ggamma", nm.weight), ("gbeta", nm.bias)]
        for k, p in ps:
            rms = float(g64[k][l].pow(2).mean().sqrt()) if g64 is not None else 0.0
            pat = ref.bf(torch.randn(p.shape, generator=gen) * (rms if rms > 1e-12 else 1e-3))
            pat[pat == 0] = 1e-3 if rms <= 1e-12 else ref.bf(torch.tensor(rms))
            p.grad = pat.to(DEV)
            pats.append((k, l, p, pat))
    return pats


def _img(ws, off, rows, S):
    return ws[off: off + 2 * rows * S].view(BF16).view(rows, S).float().cpu()


def _launch(case, train=True, strided=False, ws_fill=0, seed=SEED0, dloss=1.0):
    """One forward (+ backward when training) through the three-launch entry points.  Returns
    CPU copies of everything: outputs, ``dx``, gradients minus their patterns, state, the
    workspace images (full padded extent) and the raw bits for bitwise comparisons."""
    from dinunet_implementations_amd.ops import _lib
    from dinunet_implementations_amd.ops.head import HeadSpec
    B, layers = case["B"], case["layers"]
    mods = ref.modules(case, F32, DEV)
    for m in mods:
        m.train(train)
    spec = HeadSpec(mods, case["class_weights"], case["smoothing"])
    if strided:
        buf = torch.full((B, layers[0].inp + 8), 1e30, device=DEV)
        buf[:, :layers[0].inp] = case["x"].to(DEV)
        x = buf[:, :layers[0].inp]
    else:
        x = case["x"].to(DEV)
    assert spec.ok and spec.supported(x)
    y = case["y"].to(DEV)
    lay = spec.layout(B)
    ws = torch.full((lay[0],), ws_fill, dtype=torch.uint8, device=DEV)
    C = layers[-1].out
    out = torch.empty(B, C, device=DEV)
    loss = torch.empty((), device=DEV)
    pred = torch.empty(B, dtype=torch.long, device=DEV)
    rng = spec.rng(DEV)
    rng.fill_(seed)
    lossp = _lib.ptr(spec.loss_block(DEV))
    pats = _patterns(case, mods) if train else []
    _lib.call("dn_head_fwd_lw", spec.nl, spec._dims, spec._flags, spec._drops, spec._bnp,
              spec.ptrs(False), x.data_ptr(), x.stride(0), B, y.data_ptr(), out.data_ptr(),
              loss.data_ptr(), pred.data_ptr(), rng.data_ptr(), ws.data_ptr(), int(train),
              int(case["log_out"]), lossp, _lib.stream())
    res = dict(case=case, train=train)
    if train:
        dl = torch.full((), dloss, device=DEV)
        dx = torch.full((B, layers[0].inp), 7.0, device=DEV)
        _lib.call("dn_head_bwd_lw", spec.nl, spec._dims, spec._flags, spec._drops, spec._bnp,
                  spec.ptrs(True), B, ws.data_ptr(), dl.data_ptr(), dx.data_ptr(),
                  layers[0].inp, int(spec.loss_on), _lib.stream())
        torch.cuda.synchronize()
        res["dx"] = dx.cpu()
        g = dict(gW=[None] * len(layers), gb=[None] * len(layers), ggamma=[None] * len(layers),
                 gbeta=[None] * len(layers))
        res["pat"] = {k: [None] * len(layers) for k in g}
        res["raw"] = []
        for k, l, p, pat in pats:
            g[k][l] = p.grad.cpu().double() - pat.double()
            res["pat"][k][l] = pat
            res["raw"].append(p.grad.cpu())
        res["grads"] = dict(g, dx=res["dx"])
        res["seed_after"] = int(rng.item())
    torch.cuda.synchronize()
    res.update(out=out.cpu(), loss=loss.cpu(), pred=pred.cpu())
    nl = len(layers)
    res["rmean"], res["rvar"], res["nbt"] = [None] * nl, [None] * nl, [None] * nl
    norms = iter(m for m in mods if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.LayerNorm)))
    for l, L in enumerate(layers):
        if L.norm:
            nm = next(norms)
            if L.norm == "bn_run":
                res["rmean"][l], res["rvar"][l] = nm.running_mean.cpu(), nm.running_var.cpu()
                res["nbt"][l] = int(nm.num_batches_tracked)
    if train:
        Mp = 32 if B <= 32 else (64 if B <= 64 else B)   # image rows (head_big: exactly B)
        res["Mp"] = Mp
        res["A"], res["dZ"] = [], []
        for l in range(nl):
            a_off, S_a, dz_off, S_z = lay[1 + 4 * l: 5 + 4 * l]
            assert S_a >= layers[l].inp and S_z >= layers[l].out
            res["A"].append(_img(ws, a_off, Mp, S_a))
            res["dZ"].append(_img(ws, dz_off, Mp, S_z))
    return res


def _masks(k):
    """The kernel's combined keep masks, one per layer input, from its saved activation images:
    ``image > 0`` (ReLU below, dropped elements are zero) times ``1/(1-p)``; layer 0: ``image !=
    0`` (``x`` is drawn away from zero) when it has dropout."""
    case, B = k["case"], k["case"]["B"]
    masks = []
    for l, L in enumerate(case["layers"]):
        a = k["A"][l][:B, :L.inp]
        inv = 1.0 / (1.0 - L.drop) if L.drop else 1.0
        if l == 0:
            masks.append((a != 0).double() * inv if L.drop else None)
        else:
            assert case["layers"][l - 1].relu
            masks.append((a > 0).double() * inv)
    return masks


@functools.lru_cache(maxsize=None)
def _solved(name, B, opts=False, strided=False, dloss=1.0):
    """The kernel's step of a case and the reference (fp64) and baseline (fp32 + roundings) under
    the kernel's masks: computed once per process, shared by (a) to (d), never modified."""
    case = ref.make_case(name, B, None, opts)
    k = _launch(case, strided=strided, dloss=dloss)
    masks = _masks(k)
    f64 = ref.forward(case, F64, ref.NONE, masks=masks)
    fb = ref.forward(case, F32, ref.KERNEL, masks=masks)
    g64, gb = ref.backward(f64, dloss), ref.backward(fb, dloss)
    for key in ("gW", "gb", "ggamma", "gbeta"):     # the baseline accumulates into the pattern too
        for l, pat in enumerate(k["pat"][key]):
            if pat is not None:
                gb[key][l] = (pat + gb[key][l]).double() - pat.double()
    return case, k, masks, f64, g64, fb, gb


def _check(kind, label, triples):
    """``(name, slice kind, kernel, fp64, baseline)`` under the rule; every figure is printed and
    logged before the first assertion."""
    bad = []
    for name, sk, got, want, base in triples:
        assert got is not None, f"{name}: missing"
        assert tuple(got.shape) == tuple(want.shape), name
        e_k, e_b = ref.slice_err(got, want, sk), ref.slice_err(base, want, sk)
        _record(kind, f"{label} {name}", e_k, e_b)
        print(f"{kind} {label} {name}: E_kernel {e_k:.3e} E_base {e_b:.3e}")
        if not ref.within_rule(e_k, e_b):
            bad.append((name, e_k, e_b))
    assert not bad, f"{kind} {label}: E_kernel > 8 max(E_base, 2^-23): {bad}"


def _end_to_end(name, B, opts=False, strided=False, dloss=1.0):
    case, k, masks, f64, g64, fb, gb = _solved(name, B, opts, strided, dloss)
    layers = case["layers"]
    label = f"{name} B={B}" + (" opts" if opts else "") + (" strided" if strided else "") + \
        (f" dloss={dloss}" if dloss != 1.0 else "")
    kind = f"a:{_kernel_of(B)}"
    tr = [(n, sk, got, want, base) for (n, sk, got), (_, _, want), (_, _, base) in
          zip(ref.tensors(k, k["grads"]), ref.tensors(f64, g64), ref.tensors(fb, gb))]
    zero_bias = []
    for l in range(len(layers)):
        if ref.bias_before_bn(layers, l):
            bound = ref.zero_bias_bound(gb["gb"][l], g64["dZ"][l])
            got = float(k["grads"]["gb"][l].abs().max())
            print(f"{kind} {label} gb{l} (exactly zero): max|gb| {got:.3e} bound {bound:.3e}")
            _record(kind + ":zero_bias", f"{label} gb{l}", got, bound / 8)
            zero_bias.append((l, got, bound))
    _check(kind, label, tr)
    for l, got, bound in zero_bias:
        assert math.isfinite(got) and got <= bound, (l, got, bound)
    assert k["nbt"] == f64["nbt"]
    if not any(L.drop for L in layers):     # the forward against the reference's own masks too
        c, o64, _, ob, _ = ref.solved(name, B, None, opts)
        _check(kind + ":own_masks", label, [("out", "rows", k["out"], o64["out"], ob["out"]),
                                            ("loss", "scalar", k["loss"], o64["loss"], ob["loss"])])


# ---------------------------------------------------------------------------------------------
# (a) end to end

@pytest.mark.parametrize("name,B", ref.matrix(), ids=lambda v: str(v))
def test_end_to_end(name, B):
    _end_to_end(name, B)


@pytest.mark.parametrize("name,B", [("ica", 17), ("ica", 129), ("fs", 33), ("fs", 128)])
def test_end_to_end_loss_options(name, B):
    """Class weights + label smoothing 0.1, one batch per kernel."""
    _end_to_end(name, B, opts=True)


@pytest.mark.parametrize("B", [17, 129])
def test_end_to_end_strided_input(B):
    """``x`` a view of a buffer 8 columns wider (``ldx``), the rest of it poisoned."""
    _end_to_end("ica", B, strided=True)


@pytest.mark.parametrize("name,B", [("ica", 17), ("ica", 129), ("fs_drop", 33), ("fs_drop", 128)])
def test_end_to_end_scaled_dloss(name, B):
    """``d loss = -2.5``: the scale enters ahead of the bf16 cast of the logits' ``dZ``."""
    _end_to_end(name, B, dloss=-2.5)


@pytest.mark.parametrize("B", [1, 20, 129])
def test_evaluation_mode(B):
    """Running statistics, no state update, no dropout."""
    case = ref.make_case("ica_drop", B)
    k = _launch(case, train=False)
    f64 = ref.forward(case, F64, train=False)
    fb = ref.forward(case, F32, ref.KERNEL, train=False)
    _check(f"a:{_kernel_of(B)}:eval", f"ica_drop B={B}",
           [("out", "rows", k["out"], f64["out"], fb["out"]),
            ("loss", "scalar", k["loss"], f64["loss"], fb["loss"])])
    p = case["params"][0]
    assert torch.equal(k["rmean"][0], p["rmean"]) and torch.equal(k["rvar"][0], p["rvar"])
    assert k["nbt"][0] == 0
    assert torch.equal(k["pred"], k["out"].argmax(1))


def test_exactly_zero_tensors():
    """One class: every gradient is exactly zero (``.grad`` keeps its pattern bit for bit)."""
    for B in (17, 129):
        case, k, masks, f64, g64, fb, gb = _solved("one_class", B)
        assert float(f64["loss"]) == 0.0 and float(k["loss"]) == 0.0
        assert not bool(k["dx"].any())
        for l in range(2):
            assert not bool(k["grads"]["gW"][l].any()) and not bool(k["grads"]["gb"][l].any())


# ---------------------------------------------------------------------------------------------
# (b) pred

@pytest.mark.parametrize("name,B", ref.matrix(), ids=lambda v: str(v))
def test_pred(name, B):
    """``pred`` is the argmax of the kernel's own ``out``, and the fp64 argmax on every row whose
    fp64 top-two gap exceeds twice the row's allowed absolute error (``head_ref.pred_margin``:
    the rule applied to the row's own baseline error; with the tensor-wide ``E_base``, the
    largest over all rows, 10 to 25 % of the rows of these heads would fall under the gap at any
    seed).  At most a tenth of the rows, one at the least, may fall under it."""
    case, k, masks, f64, g64, fb, gb = _solved(name, B)
    assert torch.equal(k["pred"], k["out"].argmax(1))
    ok = ref.pred_margin(f64["out"], fb["out"])
    under = int((~ok).sum())
    print(f"b {name} B={B}: {under} of {B} rows under the margin")
    _record("b:pred_excluded", f"{name} B={B}", under, B)
    assert under <= max(1, B // 10)
    assert torch.equal(k["pred"][ok], f64["pred"][ok])


# ---------------------------------------------------------------------------------------------
# (c) masks

@pytest.mark.parametrize("name,B", ref.matrix(), ids=lambda v: str(v))
def test_relu_masks(name, B):
    """Where the kernel's ReLU mask differs from the fp64 reference's own, the reference's value
    is within the allowed forward error of that element (the rule applied to its row)."""
    case, k, masks, f64, g64, fb, gb = _solved(name, B)
    for l in range(1, len(case["layers"])):
        v64, vb = f64["V"][l], fb["V"][l].double()
        e_b = ref.slice_err(vb, v64, "rows")
        allowed = 8 * max(e_b, ref.U23) * v64.norm(dim=1, keepdim=True)
        on = masks[l] > 0
        if case["layers"][l].drop:      # a dropped element says nothing about the ReLU
            differs = on & (v64 <= 0)
        else:
            differs = on != (v64 > 0)
        print(f"c {name} B={B} layer {l}: {int(differs.sum())} of {differs.numel()} differ")
        assert bool((v64.abs() <= allowed)[differs].all()), l


@pytest.mark.parametrize("name,B", [("ica_drop", 33), ("ica_drop", 129), ("fs_drop", 33),
                                    ("fs_drop", 129), ("fs_drop2", 64), ("fs_drop2", 1030)])
def test_dropout_masks(name, B):
    """The dropped share is p within 5 binomial standard deviations; two calls, and two layers of
    one call, draw different masks."""
    case = ref.make_case(name, B)
    k1 = _launch(case)
    k2 = _launch(case, seed=k1["seed_after"])
    assert k1["seed_after"] == SEED0 + 1
    m1, m2 = _masks(k1), _masks(k2)
    f64 = ref.forward(case, F64, masks=m1)
    keeps = []
    for l, L in enumerate(case["layers"]):
        if not L.drop:
            continue
        pos = torch.ones_like(m1[l], dtype=torch.bool) if l == 0 else f64["V"][l] > 0
        # (away from the ReLU's edge: a share of the sign flips of (c) would count as drops)
        if l > 0:
            pos &= f64["V"][l] > 1e-2 * f64["V"][l].norm(dim=1, keepdim=True)
        n = int(pos.sum())
        share = float(((m1[l] == 0) & pos).sum()) / n
        sd = math.sqrt(L.drop * (1 - L.drop) / n)
        print(f"c {name} B={B} layer {l}: dropped {share:.4f} of {n}, p {L.drop} sd {sd:.4f}")
        assert abs(share - L.drop) <= 5 * sd
        pos2 = pos if l == 0 else pos & (ref.forward(case, F64, masks=m2)["V"][l] > 0)
        assert not torch.equal((m1[l] == 0) & pos2, (m2[l] == 0) & pos2)
        keeps.append((m1[l] == 0, pos))
    if len(keeps) == 2:
        (d1, p1), (d2, p2) = keeps
        w = min(d1.shape[1], d2.shape[1])
        both = p1[:, :w] & p2[:, :w]
        assert int(both.sum()) > 100
        assert not torch.equal(d1[:, :w] & both, d2[:, :w] & both)


# ---------------------------------------------------------------------------------------------
# (d) per-layer seams on the kernel's own saved state

@pytest.mark.parametrize("name,B", ref.matrix(), ids=lambda v: str(v))
def test_layer_seams(name, B):
    case, k, masks, f64, g64, fb, gb = _solved(name, B)
    layers = case["layers"]
    nl = len(layers)
    A = [k["A"][l][:B, :layers[l].inp] for l in range(nl)]          # bf16 values
    dZ = [k["dZ"][l][:B, :layers[l].out] for l in range(nl)]
    Wq = [ref.bf(p["W"]) for p in case["params"]]
    tr = []
    for l in range(nl):
        pat = k["pat"]["gW"][l]
        want = dZ[l].double().t() @ A[l].double()
        base = (pat + dZ[l].t() @ A[l]).double() - pat.double()
        tr.append((f"gW{l}", "gW", k["grads"]["gW"][l], want, base))
    want = dZ[0].double() @ Wq[0].double()
    base = dZ[0] @ Wq[0]
    if masks[0] is not None:
        want, base = want * masks[0], base * masks[0].float()
    tr.append(("dx", "rows", k["dx"], want, base))
    for l in range(nl - 1):
        m = masks[l + 1]
        want = ref.layer_forward(case, l, A[l], F64) * m
        base = ref.bf(ref.layer_forward(case, l, A[l], F32) * m.float())
        tr.append((f"A{l + 1}", "rows", A[l + 1], want, base))
    for l in range(nl - 1, 0, -1):
        want = ref.layer_backward(case, l, A[l - 1], dZ[l], masks[l], F64)
        base = ref.bf(ref.layer_backward(case, l, A[l - 1], dZ[l], masks[l], F32))
        tr.append((f"dZ{l - 1}", "rows", dZ[l - 1], want, base))
    _check(f"d:{_kernel_of(B)}", f"{name} B={B}", tr)
    for l in range(nl):     # padding of the images: finite (zero or never read: see (f))
        assert bool(torch.isfinite(k["A"][l]).all()) and bool(torch.isfinite(k["dZ"][l]).all())
        if B <= 64:         # what the kernels write of the pad is zero
            assert not bool(k["A"][l][B:, :layers[l].inp].any())
            assert not bool(k["dZ"][l][B:, :layers[l].out].any())


# ---------------------------------------------------------------------------------------------
# (e) one-launch and hinted paths

def _via_head_loss(case, path, seed=SEED0):
    """A training step through ``ops.head.head_loss``: ``path`` ``"classic"`` (no hint),
    ``"hinted"`` (``dn_head_fwd_train`` + ``dn_head_bwd0``) or ``"rep"`` (``dn_head_rep`` on the
    spec's own images).  Returns the raw results and whether the replicated head ran."""
    from dinunet_implementations_amd.ops import head as H
    mods = ref.modules(case, F32, DEV)
    for m in mods:
        m.train()
    spec = H.HeadSpec(mods, case["class_weights"], case["smoothing"])
    spec.rng(DEV).fill_(seed)
    _patterns(case, mods)
    x = case["x"].to(DEV).requires_grad_()
    y = case["y"].to(DEV)
    one = torch.ones((), device=DEV)
    old, n0 = H._HEAD_STEP, H.REP_LAUNCHES
    H._HEAD_STEP = path == "rep"
    try:
        with H.loss_grad_hint(None if path == "classic" else one):
            out, loss, pred = H.head_loss(x, spec, y, log_out=case["log_out"])
        torch.autograd.backward(loss, one)
        torch.cuda.synchronize()
    finally:
        H._HEAD_STEP = old
    ran = H.REP_LAUNCHES - n0
    exact = [out, loss, pred, x.grad] + [p.grad for m in mods for p in m.parameters()]
    state = [b for m in mods for b in m.buffers()]
    return [t.detach().cpu() for t in exact], [t.detach().cpu() for t in state], ran, spec


@pytest.mark.parametrize("B", [2, 17, 32])
@pytest.mark.parametrize("name", ref.HEADS)
def test_one_launch_and_hinted_paths_bitwise(name, B):
    """Inside their envelopes ``dn_head_rep`` and the hinted pair are bitwise the three-launch
    result (running statistics to an ulp: FMA contraction, as the existing rep tests allow);
    outside, the hinted call falls back and still matches."""
    from dinunet_implementations_amd.ops import _lib
    case = ref.make_case(name, B)
    ex0, st0, ran0, spec = _via_head_loss(case, "classic")
    assert ran0 == 0
    inside = int(_lib.lib().dn_head_rep_supported(spec.nl, spec._dims, spec._flags, B)) == 1
    if name in ("ragged", "deep", "fs", "wide", "one_layer", "one_class"):
        assert not inside       # in % 8, LayerNorm on a later layer, > 256 outputs, one layer
    if name in ("ica", "ica_drop", "ica_ln"):
        assert inside
    for path in ("hinted", "rep"):
        ex, st, ran, _ = _via_head_loss(case, path)
        assert ran == (1 if path == "rep" and inside else 0), (path, ran)
        for i, (u, v) in enumerate(zip(ex, ex0)):
            assert torch.equal(u, v), (path, i)
        for u, v in zip(st, st0):
            assert torch.allclose(u.double(), v.double(), rtol=1e-6, atol=0), path
    # and the low-level launches of (a) are what head_loss issues
    k = _launch(case)
    assert torch.equal(k["out"], ex0[0]) and torch.equal(k["dx"], ex0[3])
    for u, v in zip(k["raw"], ex0[4:]):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------
# (f) determinism

@pytest.mark.parametrize("name,B", [(n, b) for n, b in ref.matrix() if b in (1, 33, 64, 129, 1030)],
                         ids=lambda v: str(v))
def test_two_runs_bitwise_equal(name, B):
    """The same step twice, once on a zeroed workspace and once on one filled with 0xFF bytes (NaN
    as bf16 and as fp32): outputs, gradients, state and the compared extent of every image are
    bitwise equal, so nothing compared depends on padding or on what a launch did not write
    (``ops.head`` hands the kernels an uninitialised workspace)."""
    case = ref.make_case(name, B)
    k1 = _launch(case)
    k2 = _launch(case, ws_fill=255)
    for key in ("out", "loss", "pred", "dx"):
        assert torch.equal(k1[key], k2[key]), key
    for u, v in zip(k1["raw"], k2["raw"]):
        assert torch.equal(u, v)
    for l, L in enumerate(case["layers"]):
        assert torch.equal(k1["A"][l][:B, :L.inp], k2["A"][l][:B, :L.inp]), l
        assert torch.equal(k1["dZ"][l][:B, :L.out], k2["dZ"][l][:B, :L.out]), l
        if k1["rmean"][l] is not None:
            assert torch.equal(k1["rmean"][l], k2["rmean"][l])
            assert torch.equal(k1["rvar"][l], k2["rvar"][l])


# ---------------------------------------------------------------------------------------------
# (g) the error log

def test_error_log_format(tmp_path, monkeypatch):
    p = tmp_path / "err.jsonl"
    monkeypatch.setenv("DINUNET_ERR_LOG", str(p))
    _record("k", "c", 1.23456e-3, 2e-3)
    row = json.loads(p.read_text())
    assert row == {"kind": "k", "case": "c", "e_kernel": 1.235e-3, "e_base": 2e-3}
    assert math.isclose(row["e_kernel"] / row["e_base"], 0.6175)
