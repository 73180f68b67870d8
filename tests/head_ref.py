"""Plain torch reference of the fused classifier heads (``csrc/kernels/mlp_head.hip``,
``head_big.hip``, ``head_rep.hip`` behind ``ops.head.head_loss``): CPU only, no project kernel.

One pair of functions, ``forward`` and ``backward``, serves as the fp64 reference (``dtype =
torch.float64``, ``NONE``: no internal rounding) and as the baseline (fp32 with the roundings the
kernels declare, ``KERNEL``), whose own error against fp64 sets the tolerance of the GPU tests
(``assert_close``: ``E_kernel <= 8 max(E_base, 2^-23)``, ``E`` the largest relative 2-norm error
over the slices of a tensor, ``slice_err``).

A head is a list of ``Layer``: ``[dropout on the input] -> Linear(+-bias) -> [BatchNorm with batch
statistics ("bn") | BatchNorm with running statistics ("bn_run": batch statistics and a state
update in training, the running ones in evaluation) | LayerNorm ("ln") | none] -> [ReLU]``; the
last layer's logits feed softmax cross-entropy (probabilities out) or log-softmax + NLL
(log-probabilities out), with optional class weights and label smoothing normalised as
``F.cross_entropy`` does.  The backward is written by hand (``dZ`` is rounded between layers,
where autograd offers no seam); ``tests/test_head_ref.py`` holds it to autograd in fp64.

``masks``: one combined keep mask per layer input (the previous layer's ReLU mask times this
layer's dropout keep, scaled by ``1/(1-p)``; ``None`` for "all ones").  Without ``masks`` the
reference applies its own ReLU and no dropout; with them it multiplies by the given ones, forward
and backward.  A pre-activation within rounding distance of zero flips its ReLU mask, which
changes a whole row of ``dZ`` by percents without any arithmetic being wrong, so the GPU tests
hand the kernel's own masks in and check the masks themselves separately.

Declared roundings (each a switch of ``Rounding``; read off the kernel headers):

* ``a``: the input activation image of every Linear (after norm, ReLU and dropout with its
  scale) is bf16: the MFMA operand, also saved for ``dW``.
* ``w``: the weights are rounded to bf16 while loading (forward, ``dA`` and ``dx``).
* ``dz``: ``dZ_l`` is bf16 before it feeds ``dA = dZ W``, ``dW = dZ^T A`` and ``dx``.

Everything else is fp32: bias, statistics, ``xhat``, normalisation, loss, ``dx``, all parameter
gradients.  The column sums that make ``gb`` (and ``ggamma``, ``gbeta``) are taken of the fp32
values BEFORE ``dZ`` is rounded (``bwd1_body``: ``sb += d`` ahead of the cast; ``head_big``:
"bf16 image + fp32 column partials for the bias gradient"; the logits' bias: ``gs * sum dzl``), so
``dz`` does not touch them.

``make_case`` rounds ``x`` and the weights to bf16 values once, for reference and baseline alike;
biases, norm parameters and running statistics stay fp32.

Non-finite values (``poison`` puts one into a case) follow torch in the forward: ``relu(NaN)`` is
NaN, ``relu(-inf)`` is 0, a batch-statistics BatchNorm spreads a NaN over its column, LayerNorm and
the softmax over its row, and ``argmax`` takes NaN for the largest value and returns the first one.
The backward follows the mask rule the kernels declare, which is also that of the GEMM mask
epilogue: the keep mask of a ReLU is ``a > 0``, a select and not a product, so a NaN activation is
NOT kept and a gradient that meets a mask of zero is zero whatever it was.  torch autograd differs
there (its ReLU backward is ``grad * (out > 0)``, a product, so a NaN gradient stays NaN where the
mask is zero); ``tests/test_head_ref.py`` records where that shows and does not enforce it.
"""
import collections
import functools
import math

import torch

U23 = 2.0 ** -23    # fp32 resolution: the floor of every baseline error

Rounding = collections.namedtuple("Rounding", "a w dz", defaults=(False,) * 3)
NONE = Rounding()
KERNEL = Rounding(a=True, w=True, dz=True)

# norm: None, "bn" (batch statistics always), "bn_run" (running statistics kept), "ln"
Layer = collections.namedtuple("Layer", "inp out bias norm relu drop")

EPS = 1e-5
MOMENTUM = 0.1

# deliberately wrong references (tests/test_head_ref.py: each must break the rule)
MUTATIONS = ("biased_running_var", "bn_no_xhat_term", "drop_no_scale", "gW_last_batch_row",
             "gW_last_out_row", "dx_last8", "loss_div_B", "ln_rup32")


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _r(t, on):
    return bf(t) if on else t


def _t(x, dtype):
    return x.detach().to("cpu", dtype)


def mm_fp64(a, b):
    """``a @ b`` accumulated in fp64, then rounded to the operands' type: the same product in
    another accumulation order (the second baseline of ``tests/test_head_ref.py``)."""
    return (a.double() @ b.double()).to(a.dtype)


def rup32(v):
    return (v + 31) & ~31


# ---------------------------------------------------------------------------------------------
# heads

def _chain(dims, bias=True, norms=None, drops=None):
    """Layers of ``dims`` with ReLU on every hidden one."""
    n = len(dims) - 1
    norms = norms or {}
    drops = drops or {}
    return [Layer(dims[l], dims[l + 1], bias, norms.get(l), l < n - 1, drops.get(l, 0.0))
            for l in range(n)]


def make_head(name):
    """``(layers, log_out)`` of a case head.  The smallest shapes that still cross every tiling
    edge: 16-column wave tiles, 32-deep MFMA K steps, rup32 / rup8 strides, head_big's 64 x 64
    tiles with a 64-deep K chunk, head_rep's ``in % 8`` and <= 256 envelope."""
    if name in ("ica", "ica_drop", "ica_ln"):
        norm = "ln" if name == "ica_ln" else "bn_run"
        p = 0.0 if name == "ica" else 0.25
        return _chain([40, 48, 24, 3], True, {0: norm}, {0: p}), False
    if name in ("fs", "fs_drop", "fs_drop2", "fs_ln"):      # MSANNet(66, [72, 40, 24], 2)
        norm = "ln" if name == "fs_ln" else "bn"
        drops = {"fs_drop": {2: 0.5}, "fs_drop2": {1: 0.5, 2: 0.5}}   # dropout_in=[1], [0, 1]
        L = _chain([66, 72, 40, 24, 2], False, {0: norm, 1: norm, 2: norm}, drops.get(name))
        L[-1] = L[-1]._replace(bias=True)
        return L, True
    if name == "ragged":                        # in % 8 != 0: the scalar staging path
        return _chain([37, 50, 19, 5]), False
    if name == "wide":                          # K = 4*64 + 8 and 8*32 + 8; 16 classes
        return _chain([264, 272, 16], True, {0: "bn"}), False
    if name == "one_layer":
        return _chain([33, 4]), False
    if name == "deep":                          # the six-layer maximum
        return _chain([24, 32, 32, 16, 16, 8, 2], True, {0: "bn", 3: "bn", 2: "ln"}), False
    if name == "one_class":
        return _chain([12, 8, 1]), False
    raise ValueError(name)


HEADS = ("ica", "ica_drop", "ica_ln", "fs", "fs_drop", "fs_ln", "ragged", "wide", "one_layer",
         "deep", "one_class")
SMALL_B = (2, 17, 32, 33, 64)        # mlp_head.hip
BIG_B = (65, 128, 129, 1030)         # head_big.hip: 17 row blocks over <= 16 splits; 65 and 129
#                                      leave a last block of one row
EXTRA = ("fs_drop2",)                # two dropout layers: only for the masks test
ONE_ROW = ("ica_ln", "ragged", "one_layer", "one_class")   # no training BatchNorm: B = 1 is legal
LOSS_OPTS = dict(smoothing=0.1)      # + class weights (make_case)


def has_train_bn(layers):
    return any(L.norm in ("bn", "bn_run") for L in layers)


def matrix():
    """Every ``(head, B)`` of the end-to-end GPU tests."""
    m = []
    for h in HEADS:
        bs = ((1,) if h in ONE_ROW else ()) + SMALL_B + BIG_B
        m += [(h, b) for b in bs]
    return m


# data seeds other than 0: chosen so that the conditions on the inputs (tests/test_head_ref.py:
# at most 10 % of rows under the pred margin) hold under the kernels' dropout draws as well
SEEDS = {("ica_ln", 33): 3}


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def make_case(name, B, seed=None, loss_opts=False, off_grid=False):
    """Inputs of a case: ``x`` (bf16 values in fp32, drawn away from zero so that a zero in the
    kernel's input image is a dropped element), labels, per layer ``W`` (bf16 values in fp32;
    ``off_grid``: left unrounded), ``b``, ``gamma``, ``beta``, ``rmean``, ``rvar`` (fp32), and
    with ``loss_opts`` class weights and label smoothing 0.1."""
    layers, log_out = make_head(name)
    seed = SEEDS.get((name, B), 0) if seed is None else seed
    g = _gen(7919 * seed + 104729 * (HEADS + EXTRA).index(name) + B)
    C = layers[-1].out
    x = torch.randn(B, layers[0].inp, generator=g)
    x = bf(torch.sign(x) * (x.abs() + 0.1))
    if name.startswith("fs"):
        x = x.abs()
    y = torch.randint(0, C, (B,), generator=g)
    params = []
    for L in layers:
        W = torch.randn(L.out, L.inp, generator=g) * (1.5 / math.sqrt(L.inp))
        p = dict(W=W if off_grid else bf(W), b=None, gamma=None, beta=None, rmean=None, rvar=None)
        if L.bias:
            p["b"] = torch.randn(L.out, generator=g) * 0.3
            if L.relu and not L.norm:       # keeps the units of a layer without a norm alive
                p["b"] = 0.5 + p["b"].abs()
        if L.norm:                          # (|beta| < gamma: no unit dead by its parameters)
            p["gamma"] = 0.7 + 0.6 * torch.rand(L.out, generator=g)
            p["beta"] = 0.6 * torch.rand(L.out, generator=g) - 0.3
        if L.norm == "bn_run":
            p["rmean"] = torch.rand(L.out, generator=g) - 0.5
            p["rvar"] = 0.5 + 1.5 * torch.rand(L.out, generator=g)
        params.append(p)
    w = eps = None
    if loss_opts:
        w = [round(0.5 + 1.5 * float(v), 3) for v in torch.rand(C, generator=g)]
        eps = LOSS_OPTS["smoothing"]
    return dict(name=name, B=B, layers=layers, log_out=log_out, x=x, y=y, params=params,
                class_weights=w, smoothing=eps or 0.0)


POISON_WHERE = ("x", "W", "b", "gamma")


def poison(case, where, value, l=0, i=0, k=0):
    """A copy of ``case`` with one element replaced by ``value`` (``nan``, ``+inf``, ``-inf``):
    ``x[i, k]``, or of layer ``l`` ``W[i, k]``, ``b[i]`` or ``gamma[i]``.  The case handed in is
    left as it was."""
    if where not in POISON_WHERE:
        raise ValueError(where)
    value = float(value)
    c = dict(case, params=[dict(p) for p in case["params"]])
    if where == "x":
        t = case["x"].clone()
        t[i, k] = value
        c["x"] = t
        return c
    t = case["params"][l][where]
    if t is None:
        raise ValueError(f"layer {l} has no {where}")
    t = t.clone()
    if where == "W":
        t[i, k] = value
    else:
        t[i] = value
    c["params"][l][where] = t
    return c


NONFINITE_HEADS = ("ragged", "ica_ln", "ica", "fs")     # no norm, LayerNorm, running and batch BatchNorm
EVAL_HEADS = ("ica", "ragged")                           # evaluation mode: running statistics, no norm


def poison_case(name, B):
    """The case the non-finite tests poison: ``make_case`` with dropout off.  (``ica_ln`` drops a
    quarter of ``x``.  The kernels' dropout is a select, so a dropped NaN is gone, where torch's,
    a product, keeps it; which element a seed drops is not what these tests are about.)"""
    c = make_case(name, B)
    return dict(c, layers=[L._replace(drop=0.0) for L in c["layers"]])


def poisons(name, train=True):
    """``(label, where, value, l, i, k)`` of every poison of a head: ``x[1, 3]`` and one weight of
    the last layer with ``nan``, ``+inf`` and ``-inf``; one weight of layer 0, one hidden bias and
    one norm ``gamma`` (where the head has them) with ``nan``."""
    layers, _ = make_head(name)
    last = len(layers) - 1
    inf = math.inf
    ps = [(f"x[1,3]={v}", "x", v, 0, 1, 3) for v in (math.nan, inf, -inf)]
    ps.append(("W0[2,5]=nan", "W", math.nan, 0, 2, 5))
    ps += [(f"W{last}[1,4]={v}", "W", v, last, 1, 4) for v in (math.nan, inf, -inf)]
    hb = [l for l in range(last) if layers[l].bias]
    if hb:
        ps.append((f"b{hb[0]}[3]=nan", "b", math.nan, hb[0], 3, 0))
    hn = [l for l in range(last) if layers[l].norm]
    if hn:
        ps.append((f"gamma{hn[0]}[2]=nan", "gamma", math.nan, hn[0], 2, 0))
    return ps


def nonfinite_matrix():
    """``(head, train, poison label)`` of the non-finite tests."""
    m = []
    for h in NONFINITE_HEADS:
        for train in (True, False) if h in EVAL_HEADS else (True,):
            m += [(h, train, p[0]) for p in poisons(h)]
    return m


def poisoned(name, B, label):
    """``(clean case, poisoned case, the poison)`` of one entry of ``nonfinite_matrix``."""
    p = {q[0]: q for q in poisons(name)}[label]
    c = poison_case(name, B)
    return c, poison(c, p[1], p[2], p[3], p[4], p[5]), p


def grad_tensors(case, g):
    """``[(name, tensor)]`` of ``dx`` and every parameter gradient of ``backward``'s result."""
    out = [("dx", g["dx"])]
    for l in range(len(case["layers"])):
        for k in ("gW", "gb", "ggamma", "gbeta"):
            if g[k][l] is not None:
                out.append((f"{k}{l}", g[k][l]))
    return out


def nonfinite(t):
    """The set of non-finite elements of ``t`` as a boolean CPU tensor."""
    return ~torch.isfinite(t.detach().to("cpu"))


def modules(case, dtype=torch.float32, device="cpu"):
    """The plain ``torch.nn`` module list of a case (what ``ops.head.HeadSpec`` parses), with the
    case's parameters and running state loaded."""
    import torch.nn as nn
    mods = []
    for L, p in zip(case["layers"], case["params"]):
        if L.drop:
            mods.append(nn.Dropout(L.drop))
        lin = nn.Linear(L.inp, L.out, bias=L.bias)
        with torch.no_grad():
            lin.weight.copy_(p["W"])
            if L.bias:
                lin.bias.copy_(p["b"])
        mods.append(lin)
        if L.norm:
            if L.norm == "ln":
                nm = nn.LayerNorm(L.out, eps=EPS)
            else:
                nm = nn.BatchNorm1d(L.out, eps=EPS, momentum=MOMENTUM,
                                    track_running_stats=L.norm == "bn_run")
            with torch.no_grad():
                nm.weight.copy_(p["gamma"])
                nm.bias.copy_(p["beta"])
                if L.norm == "bn_run":
                    nm.running_mean.copy_(p["rmean"])
                    nm.running_var.copy_(p["rvar"])
            mods.append(nm)
        if L.relu:
            mods.append(nn.ReLU())
    return [m.to(device=device, dtype=dtype) for m in mods]


# ---------------------------------------------------------------------------------------------
# operations

def forward(case, dtype=torch.float64, rnd=NONE, masks=None, train=True, mm=torch.matmul,
            mutate=None, x=None):
    """The head's forward.  Returns a dict with ``out``, ``loss``, ``pred``, ``logits``, per layer
    the input activation image ``A``, the value ``V`` it is the masked and rounded form of (the
    layer below's output ahead of its ReLU) and the pre-norm ``z``, the reference's own masks
    (``own_masks``: ReLU only), after a training step ``rmean``, ``rvar``, ``nbt`` per layer
    (``None`` where the layer keeps no state) and what ``backward`` needs."""
    layers = case["layers"]
    v = _t(case["x"] if x is None else x, dtype)     # the value feeding the next layer's mask
    B = v.shape[0]
    A, Z, V, own, st, rmean, rvar, nbt, Wq = [], [], [], [], [], [], [], [], []
    for l, (L, p) in enumerate(zip(layers, case["params"])):
        relu_below = l > 0 and layers[l - 1].relu
        m_own = (v > 0).to(dtype) if relu_below else None
        own.append(m_own)
        V.append(v)
        m = masks[l] if masks is not None else m_own
        if masks is None and relu_below:
            a = _r(torch.relu(v), rnd.a)     # (not v * m_own: NaN stays NaN, -inf becomes 0)
        else:
            a = _r(v if m is None else v * _t(m, dtype), rnd.a)
        W = _r(_t(p["W"], dtype), rnd.w)
        z = mm(a, W.t())
        if L.bias:
            z = z + _t(p["b"], dtype)
        A.append(a)
        Z.append(z)
        Wq.append(W)
        s = dict(mask=m)
        rm = rv = nb = None
        if L.norm in ("bn", "bn_run"):
            if train or L.norm == "bn":
                mean = z.mean(0)
                var = ((z - mean) ** 2).mean(0)
                if L.norm == "bn_run":
                    unb = 1.0 if mutate == "biased_running_var" else B / max(B - 1, 1)
                    rm = (1 - MOMENTUM) * _t(p["rmean"], dtype) + MOMENTUM * mean
                    rv = (1 - MOMENTUM) * _t(p["rvar"], dtype) + MOMENTUM * var * unb
                    nb = 1
            else:
                mean, var = _t(p["rmean"], dtype), _t(p["rvar"], dtype)
            rstd = (var + EPS) ** -0.5
            xhat = (z - mean) * rstd
            v = _t(p["gamma"], dtype) * xhat + _t(p["beta"], dtype)
            s.update(xhat=xhat, rstd=rstd)
        elif L.norm == "ln":
            n = rup32(L.out) if mutate == "ln_rup32" else L.out     # (the pad columns hold zeros)
            mean = z.sum(1, keepdim=True) / n
            var = (((z - mean) ** 2).sum(1, keepdim=True) + (n - L.out) * mean ** 2) / n
            rstd = (var + EPS) ** -0.5
            xhat = (z - mean) * rstd
            v = _t(p["gamma"], dtype) * xhat + _t(p["beta"], dtype)
            s.update(xhat=xhat, rstd=rstd)
        else:
            v = z
        st.append(s)
        rmean.append(rm)
        rvar.append(rv)
        nbt.append(nb)
    logits = v
    C = logits.shape[1]
    y = case["y"].clamp(0, C - 1)
    w = torch.ones(C, dtype=dtype) if case["class_weights"] is None else \
        torch.tensor(case["class_weights"], dtype=dtype)
    eps = case["smoothing"]
    mx = logits.max(1, keepdim=True).values      # (one class: lse == z exactly, as in the kernels)
    lse = mx + (logits - mx).exp().sum(1, keepdim=True).log()
    lp = logits - lse
    prob = lp.exp()
    hit = torch.nn.functional.one_hot(y, C).to(dtype)
    wy = w[y].unsqueeze(1)
    D = float(B) if mutate == "loss_div_B" else wy.sum()
    rows = ((1 - eps) * wy * -(lp * hit).sum(1, keepdim=True)
            + (eps / C) * -(lp * w).sum(1, keepdim=True))
    loss = rows.sum() / D
    # (grouped so that one class, p = 1, gives exactly zero)
    dlogits = ((1 - eps) * wy * (prob - hit) + (eps / C) * (prob * w.sum() - w)) / D
    return dict(out=lp if case["log_out"] else prob, loss=loss, pred=logits.argmax(1),
                logits=logits, A=A, Z=Z, V=V, own_masks=own, rmean=rmean, rvar=rvar, nbt=nbt,
                st=st, W=Wq, dlogits=dlogits, case=case, dtype=dtype, rnd=rnd, mm=mm, train=train)


def backward(fw, dloss=1.0, mutate=None):
    """Gradients of ``dloss * loss`` through ``forward``'s result (with the masks it ran with):
    ``dx`` and per layer ``gW``, ``gb``, ``ggamma``, ``gbeta`` (``None`` where the layer has no
    such parameter) and the output-gradient image ``dZ``."""
    case, dtype, rnd, mm = fw["case"], fw["dtype"], fw["rnd"], fw["mm"]
    layers = case["layers"]
    n = len(layers)
    res = dict(gW=[None] * n, gb=[None] * n, ggamma=[None] * n, gbeta=[None] * n, dZ=[None] * n)
    dzf = fw["dlogits"] * dloss                       # fp32 dZ of the layer at hand, unrounded
    for l in range(n - 1, -1, -1):
        L, s = layers[l], fw["st"][l]
        dZ = _r(dzf, rnd.dz)
        res["dZ"][l] = dZ
        a = fw["A"][l]
        if mutate == "gW_last_batch_row" and l == 0:
            gW = mm(dZ[:-1].t(), a[:-1])
        else:
            gW = mm(dZ.t(), a)
        if mutate == "gW_last_out_row" and l == 0:
            gW = gW.clone()
            gW[-1] = 0
        res["gW"][l] = gW
        if L.bias:
            res["gb"][l] = dzf.sum(0)
        dA = mm(dZ, fw["W"][l])
        m = s["mask"]
        if m is not None:
            m = _t(m, dtype)
            if mutate == "drop_no_scale" and L.drop:
                m = (m != 0).to(dtype)
            dA = torch.where(m != 0, dA * m, torch.zeros_like(dA))    # a select: see the docstring
        if l == 0:
            if mutate == "dx_last8":
                dA = dA.clone()
                dA[:, -8:] = 0
            res["dx"] = dA
            break
        P, ps, pp = layers[l - 1], fw["st"][l - 1], case["params"][l - 1]
        dy = dA
        if P.norm in ("bn", "bn_run"):
            if not (fw["train"] or P.norm == "bn"):
                raise ValueError("backward through running statistics")
            xhat, rstd, gamma = ps["xhat"], ps["rstd"], _t(pp["gamma"], dtype)
            res["ggamma"][l - 1] = (dy * xhat).sum(0)
            res["gbeta"][l - 1] = dy.sum(0)
            t = 0 if mutate == "bn_no_xhat_term" else xhat * (dy * xhat).mean(0)
            dzf = gamma * rstd * (dy - dy.mean(0) - t)
        elif P.norm == "ln":
            xhat, rstd, gamma = ps["xhat"], ps["rstd"], _t(pp["gamma"], dtype)
            res["ggamma"][l - 1] = (dy * xhat).sum(0)
            res["gbeta"][l - 1] = dy.sum(0)
            g = dy * gamma
            dzf = rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
        else:
            dzf = dy
    return res


def layer_forward(case, l, a, dtype, train=True):
    """Layer ``l`` applied to its input image ``a`` (fp32 statistics and all): the value ahead of
    the next layer's mask.  The seam of ``A_{l+1}`` against ``A_l``."""
    c = dict(case, layers=case["layers"][l:l + 1], params=case["params"][l:l + 1],
             x=a, y=torch.zeros(a.shape[0], dtype=torch.long), class_weights=None, smoothing=0.0)
    return forward(c, dtype, Rounding(w=True), train=train)["logits"]


def layer_backward(case, l, a_prev, dz, mask, dtype):
    """``dZ_{l-1}`` (unrounded) from ``dZ_l``: ``dA = dZ_l W_l`` (bf16 weights), the combined mask
    of layer ``l``'s input, the norm backward of layer ``l-1`` on its forward state recomputed
    from that layer's own input image ``a_prev``."""
    layers = case["layers"]
    c = dict(case, layers=layers[l - 1:l], params=case["params"][l - 1:l], x=a_prev,
             y=torch.zeros(a_prev.shape[0], dtype=torch.long), class_weights=None, smoothing=0.0)
    s = forward(c, dtype, Rounding(w=True))["st"][0]
    dy = _t(dz, dtype) @ bf(_t(case["params"][l]["W"], dtype))
    if mask is not None:
        dy = dy * _t(mask, dtype)
    P = layers[l - 1]
    if not P.norm:
        return dy
    gamma, xhat, rstd = _t(case["params"][l - 1]["gamma"], dtype), s["xhat"], s["rstd"]
    if P.norm == "ln":
        g = dy * gamma
        return rstd * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    return gamma * rstd * (dy - dy.mean(0) - xhat * (dy * xhat).mean(0))


# ---------------------------------------------------------------------------------------------
# errors

def _slices(t, kind):
    """``t`` as ``[slices, values]`` for ``kind``: ``rows`` (``out``, ``dx``, activation and
    ``dZ`` images) one batch row; ``gW`` one output row; ``feat`` (``gb``, ``ggamma``, ``gbeta``,
    running statistics) one block of 16 consecutive features, the last one ragged (16 columns is
    what one wave owns); ``scalar`` the value."""
    t = _t(t, torch.float64)
    if kind in ("rows", "gW"):
        return t.reshape(t.shape[0], -1)
    if kind == "feat":
        t = t.reshape(-1)
        pad = -t.numel() % 16
        return torch.cat([t, t.new_zeros(pad)]).reshape(-1, 16)
    if kind == "scalar":
        return t.reshape(1, 1)
    raise ValueError(kind)


def zero_slices(ref64, kind):
    """Indices of the slices of the reference that are exactly zero."""
    r = _slices(ref64, kind)
    return torch.nonzero((r == 0).all(1)).flatten().tolist()


def slice_err(got, ref64, kind):
    """The largest relative 2-norm error over the slices of ``got`` against ``ref64`` (see
    ``_slices``).  A slice whose reference is exactly zero is left out of the ratio and must be
    exactly zero in ``got``: the result is ``inf`` if it is not (``nan`` for a non-finite
    ``got``)."""
    g, r = _slices(got, kind), _slices(ref64, kind)
    if g.shape != r.shape:
        raise ValueError(f"{kind}: shape {tuple(g.shape)} against {tuple(r.shape)}")
    if not bool(torch.isfinite(g).all()):
        return math.nan
    den = r.norm(dim=1)
    num = (g - r).norm(dim=1)
    zero = den == 0
    if bool((num[zero] != 0).any()):
        return math.inf
    if bool(zero.all()):
        return 0.0
    return float((num[~zero] / den[~zero]).max())


def whole_err(got, ref64):
    """Relative Frobenius error over the whole tensor: the metric of the older head tests, kept to
    show what it cannot see (``tests/test_head_ref.py``)."""
    got, ref64 = _t(got, torch.float64), _t(ref64, torch.float64)
    return float((got - ref64).norm()) / max(float(ref64.norm()), 1e-300)


def within_rule(e_k, e_b):
    return math.isfinite(e_k) and e_k <= 8 * max(e_b, U23)


def assert_close(got, ref64, base, kind, what=""):
    """The tolerance rule: ``E_kernel <= 8 max(E_base, 2^-23)`` with ``E`` the slice maximum of
    ``slice_err``; returns both errors."""
    e_k, e_b = slice_err(got, ref64, kind), slice_err(base, ref64, kind)
    assert not math.isnan(e_k), f"{what}: non-finite kernel output"
    assert e_k != math.inf, f"{what}: a slice that is exactly zero in the reference is not zero"
    assert within_rule(e_k, e_b), \
        f"{what}: E_kernel {e_k:.3e} > 8 max(E_base {e_b:.3e}, 2^-23)"
    return e_k, e_b


def bias_before_bn(layers, l):
    """Layer ``l`` has a bias ahead of a batch-statistics BatchNorm (training): its gradient is
    zero in exact arithmetic."""
    return layers[l].bias and layers[l].norm in ("bn", "bn_run")


def zero_bias_bound(gb_base, dz64):
    """The absolute bound on the gradient of a bias ahead of a batch-statistics BatchNorm, whose
    exact value is zero (the kernel's is a sum of fp32 ``dZ``): ``8 max(max|gb_base|, 2^-23
    max_col sum_rows |dZ|)`` -- the factor and floor of the relative rule."""
    floor = U23 * float(_t(dz64, torch.float64).abs().sum(0).max())
    return 8 * max(float(_t(gb_base, torch.float64).abs().max()), floor)


def tensors(fw, grads=None):
    """``[(name, kind, tensor)]`` of everything the end-to-end tests compare: ``out``, ``loss``,
    the new running statistics and, when ``grads`` is given, ``dx`` and every parameter gradient
    (a bias ahead of a batch-statistics BatchNorm excepted: ``zero_bias_bound``)."""
    layers = fw["case"]["layers"]
    out = [("out", "rows", fw["out"]), ("loss", "scalar", fw["loss"])]
    for l in range(len(layers)):
        if fw["rmean"][l] is not None:
            out += [(f"rmean{l}", "feat", fw["rmean"][l]), (f"rvar{l}", "feat", fw["rvar"][l])]
    if grads is not None:
        out.append(("dx", "rows", grads["dx"]))
        for l in range(len(layers)):
            out.append((f"gW{l}", "gW", grads["gW"][l]))
            for k in ("gb", "ggamma", "gbeta"):
                if grads[k][l] is not None and not (k == "gb" and bias_before_bn(layers, l)):
                    out.append((f"{k}{l}", "feat", grads[k][l]))
    return out


@functools.lru_cache(maxsize=None)
def solved(name, B, seed=None, loss_opts=False):
    """``(case, fp64 forward, fp64 gradients, baseline forward, baseline gradients)`` with the
    reference's own masks (ReLU, no dropout): computed once per process, never modified."""
    c = make_case(name, B, seed, loss_opts)
    f64 = forward(c, torch.float64, NONE)
    fb = forward(c, torch.float32, KERNEL)
    return c, f64, backward(f64), fb, backward(fb)


def pred_margin(out64, out_base):
    """Rows whose fp64 top-two gap of ``out`` exceeds twice the row's allowed absolute error, ``8
    max(|base_row - ref_row|, 2^-23 |ref_row|)`` (2-norms; the rule of ``assert_close`` applied
    to the row): on these ``pred`` must be the fp64 argmax."""
    o, b = _t(out64, torch.float64), _t(out_base, torch.float64)
    if o.shape[1] < 2:
        return torch.ones(o.shape[0], dtype=torch.bool)
    top = o.topk(2, dim=1).values
    allowed = 8 * torch.maximum((b - o).norm(dim=1), U23 * o.norm(dim=1))
    return (top[:, 0] - top[:, 1]) > 2 * allowed
