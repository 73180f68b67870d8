"""Plain torch reference of the persistent LSTM recurrences (``csrc/kernels/lstm.hip`` and the
GEMMs ``ops/lstm.py`` puts around them): CPU only, no project kernel.

One pair of functions, ``forward`` and ``backward``, serves as the fp64 reference (``dtype =
torch.float64``, ``NONE``: no internal rounding) and as the baseline (fp32 with the roundings the
kernels declare, ``KERNEL``), whose own error against fp64 sets the tolerance of the GPU tests
(``assert_close``: ``E_kernel <= 8 max(E_base, 2^-23)``, ``E`` the largest relative 2-norm error
over the slices of a tensor, ``slice_err``).

The math is ``ops.reference.lstm_cell_seq`` / ``bilstm``: i, f, o = sigmoid(sigmoid(pre)), g =
tanh(pre), gate rows ``[i|f|o|g]``, the reverse direction on the flipped sequence with its
outputs in processing order.  The backward is written by hand (the gate gradients are rounded in
the middle of the reverse-time recurrence, where autograd offers no seam); ``tests/
test_lstm_ref.py`` holds it to autograd through ``ops.reference.bilstm`` in fp64.

Declared roundings (each a switch of ``Rounding``):

* ``xp``: the input projection ``x W_ih^T`` is stored in bf16 (the bias is added in fp32 later).
* ``h``: ``h_{t-1}`` enters the recurrent product, and is saved for ``dW_hh``, in bf16.
* ``dpre``: the gate gradients are stored in bf16 before they feed the reverse-time product,
  both weight gradients, the bias sums and ``dx``.
* ``dx``: the input gradient is stored in bf16.
* ``pre``: the stored gate pre-activations are bf16 when the backward recomputes its gates from
  them (``DINUNET_LSTM_PRE_BF16``); the forward's own gates never see this rounding.

``x``, ``W_ih`` and ``W_hh`` are rounded to bf16 once, for reference and baseline alike
(``make_case``); the biases stay fp32, as the kernels consume them.
"""
import collections
import functools
import math

import torch

U23 = 2.0 ** -23    # fp32 resolution: the floor of every baseline error
I = 24              # input features of every case

Rounding = collections.namedtuple("Rounding", "xp h dpre dx pre", defaults=(False,) * 5)
NONE = Rounding()
FORWARD = Rounding(xp=True, h=True)
KERNEL = Rounding(xp=True, h=True, dpre=True, dx=True)
KERNEL_PRE_BF16 = KERNEL._replace(pre=True)

# deliberately wrong references (tests/test_lstm_ref.py: each must break the rule)
MUTATIONS = ("single_sigmoid", "no_flip", "mean_scale", "no_dcT", "dhT_first", "hT_neighbour",
             "dW_hh_gate", "dW_hh_gate_1.1")


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _r(t, on):
    return bf(t) if on else t


def _t(x, dtype):
    return x.detach().to("cpu", dtype)


def mm_fp64(a, b):
    """``a @ b`` accumulated in fp64, then rounded to the operands' type: the same product in
    another accumulation order (the second baseline of ``tests/test_lstm_ref.py``)."""
    return (a.double() @ b.double()).to(a.dtype)


# ---------------------------------------------------------------------------------------------
# operations

def _gates(pre, Hd, single_sigmoid=False):
    """``(s_i, s_f, s_o, i, f, o, g)`` of the pre-activations ``[B, 4Hd]`` (rows ``[i|f|o|g]``)."""
    s = torch.sigmoid(pre[:, :3 * Hd])
    a = s if single_sigmoid else torch.sigmoid(s)
    g = torch.tanh(pre[:, 3 * Hd:])
    return (s[:, :Hd], s[:, Hd:2 * Hd], s[:, 2 * Hd:], a[:, :Hd], a[:, Hd:2 * Hd], a[:, 2 * Hd:], g)


def forward(x, params, mode, dtype=torch.float64, rnd=NONE, mm=torch.matmul, mutate=None,
            mm_rec=None):
    """The bi-LSTM forward.  ``x`` ``[B, S, I]``, ``params`` one ``(w_ih, b_ih, w_hh, b_hh)`` per
    direction, ``mode`` ``"mean"`` or ``"seq"``.  Returns a dict with ``out`` (``hmean [B,
    ndir*Hd]`` or ``hseq [B, S, ndir*Hd]``), ``hT``, ``cT`` and what ``backward`` needs.  ``mm``
    forms every product, ``mm_rec`` (default: ``mm``) the recurrent one ``h_{t-1} W_hh^T``."""
    x = _t(x, dtype)
    mm_rec = mm if mm_rec is None else mm_rec
    B, S, _ = x.shape
    ndir = len(params)
    Hd = params[0][2].shape[1]
    scale = 1.0 / (S + 1) if mutate == "mean_scale" else 1.0 / S
    single = mutate == "single_sigmoid"
    dirs, outs, hTs, cTs = [], [], [], []
    for d, p in enumerate(params):
        w_ih, b_ih, w_hh, b_hh = (_t(t, dtype) for t in p)
        flip = d == 1 and mutate != "no_flip"
        xd = torch.flip(x, (1,)) if flip else x                    # processing order
        xp = _r(mm(xd.reshape(B * S, -1), w_ih.t()), rnd.xp).view(B, S, 4 * Hd)
        bias = b_ih + b_hh
        h = torch.zeros(B, Hd, dtype=dtype)
        c = torch.zeros(B, Hd, dtype=dtype)
        pres, cs, hqs, hs = [], [], [], []
        for t in range(S):
            hq = _r(h, rnd.h)
            pre = mm_rec(hq, w_hh.t()) + xp[:, t] + bias
            _, _, _, gi, gf, go, gg = _gates(pre, Hd, single)
            c = gf * c + gi * gg
            h = go * torch.tanh(c)
            pres.append(pre)
            cs.append(c)
            hqs.append(hq)
            hs.append(h)
        hseq = torch.stack(hs, 1)
        outs.append(hseq.sum(1) * scale if mode == "mean" else hseq)
        hTs.append(h)
        cTs.append(c)
        dirs.append(dict(xd=xd, flip=flip, w_ih=w_ih, w_hh=w_hh, pre=pres, c=cs, hq=hqs))
    hT = torch.cat(hTs, 1)
    if mutate == "hT_neighbour" and B > 1:   # one batch row's hT taken from its neighbour
        hT = hT.clone()
        hT[B // 2] = hT[B // 2 - 1]
    return dict(out=torch.cat(outs, -1), hT=hT, cT=torch.cat(cTs, 1), mode=mode, x=x, dirs=dirs,
                dims=(B, S, Hd, ndir), dtype=dtype, rnd=rnd, mm=mm, scale=scale, single=single)


def backward(fw, g_out=None, g_h=None, g_c=None, relu_input=False, mutate=None):
    """Gradients of ``sum(out*g_out) + sum(hT*g_h) + sum(cT*g_c)`` (each term optional) through
    ``forward``'s result: ``dx [B, S, I]``, per direction ``dW_ih``, ``db_ih``, ``dW_hh``,
    ``db_hh`` (lists), and the gate gradients ``dpre [B, S, ndir, 4Hd]`` at the original time
    index.  ``relu_input``: ``dx`` is zeroed where ``x <= 0``."""
    B, S, Hd, ndir = fw["dims"]
    dtype, rnd, mm = fw["dtype"], fw["rnd"], fw["mm"]
    mean = fw["mode"] == "mean"
    zero = torch.zeros(B, ndir * Hd, dtype=dtype)
    g_out = None if g_out is None else _t(g_out, dtype)
    g_h = zero if g_h is None else _t(g_h, dtype)
    g_c = zero if g_c is None or mutate == "no_dcT" else _t(g_c, dtype)
    res = dict(dW_ih=[], db_ih=[], dW_hh=[], db_hh=[])
    dx = torch.zeros_like(fw["x"])
    dpre_all = torch.zeros(B, S, ndir, 4 * Hd, dtype=dtype)
    t_hT = 0 if mutate == "dhT_first" else S - 1
    for d, st in enumerate(fw["dirs"]):
        sl = slice(d * Hd, (d + 1) * Hd)
        dcc = g_c[:, sl]
        dhrec = torch.zeros(B, Hd, dtype=dtype)
        es = [None] * S
        for t in range(S - 1, -1, -1):
            si, sf, so, gi, gf, go, gg = _gates(_r(st["pre"][t], rnd.pre), Hd, fw["single"])
            tc = torch.tanh(st["c"][t])
            cp = st["c"][t - 1] if t > 0 else torch.zeros(B, Hd, dtype=dtype)
            dh = dhrec
            if g_out is not None:
                dh = dh + (g_out[:, sl] * fw["scale"] if mean else g_out[:, t, sl])
            if t == t_hT:
                dh = dh + g_h[:, sl]
            dc = dcc + dh * go * (1 - tc * tc)
            dcc = dc * gf
            if fw["single"]:
                di, df, do = (dc * gg * gi * (1 - gi), dc * cp * gf * (1 - gf),
                              dh * tc * go * (1 - go))
            else:
                di = dc * gg * gi * (1 - gi) * si * (1 - si)
                df = dc * cp * gf * (1 - gf) * sf * (1 - sf)
                do = dh * tc * go * (1 - go) * so * (1 - so)
            e = _r(torch.cat([di, df, do, dc * gi * (1 - gg * gg)], 1), rnd.dpre)
            dhrec = mm(e, st["w_hh"])
            es[t] = e
        E = torch.stack(es, 1)                                   # [B, S, 4Hd], processing order
        E2 = E.reshape(B * S, 4 * Hd)
        dW_hh = mm(E2.t(), torch.stack(st["hq"], 1).reshape(B * S, Hd))
        if mutate in ("dW_hh_gate", "dW_hh_gate_1.1"):   # the o-gate block of dW_hh scaled
            dW_hh = dW_hh.clone()
            dW_hh[2 * Hd:3 * Hd] *= 1.01 if mutate == "dW_hh_gate" else 1.1
        db = E2.sum(0)
        res["dW_ih"].append(mm(E2.t(), st["xd"].reshape(B * S, -1)))
        res["dW_hh"].append(dW_hh)
        res["db_ih"].append(db)
        res["db_hh"].append(db.clone())
        dxd = mm(E2, st["w_ih"]).view(B, S, -1)
        dx = dx + (torch.flip(dxd, (1,)) if st["flip"] else dxd)
        dpre_all[:, :, d] = torch.flip(E, (1,)) if st["flip"] else E
    dx = _r(dx, rnd.dx)
    if relu_input:
        dx = dx * (fw["x"] > 0)
    res["dx"] = dx
    res["dpre"] = dpre_all
    return res


# ---------------------------------------------------------------------------------------------
# inputs (all seeded)

def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def make_case(B, S, Hd, ndir, mode, seed=0, scale=0.2, x_scale=1.0, relu=False):
    """``x`` (bf16 values in fp32), the parameters (weights bf16 values in fp32, biases fp32) and
    the loss weights ``g_out``, ``g_h``, ``g_c`` of a case."""
    g = _gen(1000 + seed)
    params = []
    for _ in range(ndir):
        w_ih, b_ih, w_hh, b_hh = (torch.randn(*s, generator=g) * scale
                                  for s in ((4 * Hd, I), (4 * Hd,), (4 * Hd, Hd), (4 * Hd,)))
        params.append((bf(w_ih), b_ih, bf(w_hh), b_hh))
    x = torch.randn(B, S, I, generator=g) * x_scale
    x = bf(torch.relu(x) if relu else x)
    g_out = torch.randn(*((B, ndir * Hd) if mode == "mean" else (B, S, ndir * Hd)), generator=g)
    g_h = torch.randn(B, ndir * Hd, generator=g)
    g_c = torch.randn(B, ndir * Hd, generator=g)
    return dict(x=x, params=params, g_out=g_out, g_h=g_h, g_c=g_c, mode=mode,
                dims=(B, S, Hd, ndir))


LOSSES = ("out", "all", "cT")   # out only; out + hT + cT; cT only (the backward's dout=None path)


def loss_weights(case, loss):
    """``dict(g_out=, g_h=, g_c=)`` of one of ``LOSSES`` (absent terms ``None``)."""
    return dict(g_out=case["g_out"] if loss in ("out", "all") else None,
                g_h=case["g_h"] if loss == "all" else None,
                g_c=case["g_c"] if loss in ("all", "cT") else None)


# (B, S, Hd per direction, ndir, mode) of the GPU tests (tests/test_lstm_gpu.py)
RESIDENT = [(5, 9, 32, 2, "mean"), (1, 1, 64, 1, "seq"), (7, 2, 64, 2, "mean"),
            (6, 5, 100, 2, "mean"), (9, 4, 128, 1, "seq"), (13, 7, 174, 2, "seq"),
            (32, 6, 192, 2, "mean")]
STREAMED = [(3, 5, 200, 2, "seq"), (6, 1, 256, 2, "mean"), (5, 4, 300, 2, "mean"),
            (2, 3, 512, 2, "seq")]
# (case, rows per workgroup of the forward, of the backward)
ROW_TILING = [((1032, 3, 192, 2, "mean"), 4, 8), ((1028, 3, 192, 2, "mean"), 4, 4),
              ((4100, 2, 40, 2, "mean"), 8, 8)]
BR_CASES = [(19, 5, 32, 2, "seq"), (19, 4, 100, 2, "mean"), (19, 5, 174, 2, "seq")]
PRE_BF16_CASE = (13, 5, 192, 2, "mean")
RELU_CASES = [(6, 5, 100, 2, "mean"), (32, 6, 192, 2, "mean")]
SATURATED = (4, 6, 64, 2, "mean")
SATURATED_SCALES = dict(scale=2.0, x_scale=4.0)


def matrix():
    """Every ``(case, make_case keywords, rounding)`` the GPU numerics tests run."""
    m = [(c, {}, KERNEL) for c in RESIDENT + STREAMED + [r[0] for r in ROW_TILING] + BR_CASES]
    m.append((PRE_BF16_CASE, {}, KERNEL_PRE_BF16))
    m += [(c, dict(relu=True), KERNEL) for c in RELU_CASES]
    return m


@functools.lru_cache(maxsize=None)
def _cached(case, kw, rnd, fp64):
    c = make_case(*case, **dict(kw))
    fw = forward(c["x"], c["params"], case[4], torch.float64 if fp64 else torch.float32,
                 NONE if fp64 else rnd)
    return c, fw, {}


def solved(case, kw=None, rnd=KERNEL, loss="out", fp64=True):
    """``(inputs, forward result, gradients)`` of a case in fp64 without rounding (``fp64``) or
    as the fp32 baseline with ``rnd``: computed once per process and shared, never modified."""
    kw = kw or {}
    c, fw, grads = _cached(tuple(case), tuple(sorted(kw.items())), rnd, bool(fp64))
    if loss not in grads:
        grads[loss] = backward(fw, relu_input=bool(kw.get("relu")), **loss_weights(c, loss))
    return c, fw, grads[loss]


# ---------------------------------------------------------------------------------------------
# errors

GATES = 4   # gate blocks of Hd rows in every weight and bias gradient


def _slices(t, kind, ndir=1):
    """``t`` as ``[slices, values]`` for ``kind``: ``hmean`` / ``hT`` / ``cT`` one (batch row,
    direction) block of Hd values; ``hseq`` one (batch row, time step, direction) block; ``dx``
    one (batch row, time step) row; ``dW_ih`` / ``dW_hh`` / ``db_ih`` / ``db_hh`` (one direction's
    gradient) one gate block of Hd rows."""
    t = _t(t, torch.float64)
    if kind in ("hmean", "hT", "cT"):
        return t.reshape(t.shape[0] * ndir, -1)
    if kind == "hseq":
        return t.reshape(t.shape[0] * t.shape[1] * ndir, -1)
    if kind == "dx":
        return t.reshape(t.shape[0] * t.shape[1], -1)
    if kind in ("dW_ih", "dW_hh", "db_ih", "db_hh"):
        return t.reshape(GATES, -1)
    raise ValueError(kind)


def zero_slices(ref64, kind, ndir=1):
    """Indices of the slices of the reference that are exactly zero."""
    r = _slices(ref64, kind, ndir)
    return torch.nonzero((r == 0).all(1)).flatten().tolist()


def slice_err(got, ref64, kind, ndir=1):
    """The largest relative 2-norm error over the slices of ``got`` against ``ref64`` (see
    ``_slices``).  A slice whose reference is exactly zero is left out of the ratio and must be
    exactly zero in ``got``: the result is ``inf`` if it is not (``nan`` for a non-finite
    ``got``)."""
    g, r = _slices(got, kind, ndir), _slices(ref64, kind, ndir)
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
    """Relative Frobenius error over the whole tensor: the metric of the older LSTM tests, kept to
    show what it cannot see (``tests/test_lstm_ref.py``)."""
    got, ref64 = _t(got, torch.float64), _t(ref64, torch.float64)
    return float((got - ref64).norm()) / max(float(ref64.norm()), 1e-300)


def within_rule(e_k, e_b):
    return math.isfinite(e_k) and e_k <= 8 * max(e_b, U23)


def assert_close(got, ref64, base, kind, what="", ndir=1):
    """The tolerance rule: ``E_kernel <= 8 max(E_base, 2^-23)`` with ``E`` the slice maximum of
    ``slice_err``; returns both errors."""
    e_k, e_b = slice_err(got, ref64, kind, ndir), slice_err(base, ref64, kind, ndir)
    assert not math.isnan(e_k), f"{what}: non-finite kernel output"
    assert e_k != math.inf, f"{what}: a slice that is exactly zero in the reference is not zero"
    assert within_rule(e_k, e_b), \
        f"{what}: E_kernel {e_k:.3e} > 8 max(E_base {e_b:.3e}, 2^-23)"
    return e_k, e_b


def out_kind(mode):
    return "hmean" if mode == "mean" else "hseq"


def tensors(fw, grads, ndir):
    """``[(name, kind, tensor)]`` of everything the tests compare: the three outputs and, when
    ``grads`` is given, ``dx`` and every direction's four parameter gradients."""
    out = [("out", out_kind(fw["mode"]), fw["out"]), ("hT", "hT", fw["hT"]), ("cT", "cT", fw["cT"])]
    if grads is not None:
        out.append(("dx", "dx", grads["dx"]))
        for d in range(ndir):
            for k in ("dW_ih", "db_ih", "dW_hh", "db_hh"):
                out.append((f"{k}{d}", k, grads[k][d]))
    return out


def expected_zero_gates(S, loss):
    """Gate blocks (0 i, 1 f, 2 o, 3 g) of the parameter gradients that are exactly zero, as
    ``{kind: gates}``.  At ``S = 1`` ``h_{-1} = 0`` zeroes all of ``dW_hh`` and ``c_{-1} = 0`` the
    f gate's gradient; with the ``cT``-only loss no gradient reaches ``h_T``, so the o gate's
    gradient at the last step -- at ``S = 1`` the only one -- is zero as well; at ``S = 2`` its
    only other step is the first, which meets ``h_{-1} = 0`` in ``dW_hh``."""
    if S > 1:
        z = {k: [] for k in ("dW_ih", "db_ih", "dW_hh", "db_hh")}
        if S == 2 and loss == "cT":
            z["dW_hh"] = [2]
        return z
    z = [1, 2] if loss == "cT" else [1]
    return dict(dW_ih=z, db_ih=z, db_hh=z, dW_hh=[0, 1, 2, 3])
