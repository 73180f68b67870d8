"""The persistent LSTM recurrences of ``csrc/kernels/lstm.hip`` against the fp64 reference of
``tests/lstm_ref.py``, per slice.

(a) Numerics through the public ``ops.lstm.bilstm`` and autograd.  Every output (``hmean`` or
``hseq``, ``hT``, ``cT``) and every gradient (``dx``, and per direction ``dW_ih``, ``db_ih``,
``dW_hh``, ``db_hh``) is held to ``E_kernel <= 8 max(E_base, 2^-23)``: ``E`` is the largest
relative 2-norm error against fp64 over the slices of the tensor (one batch row and direction, one
time step of one, one row of ``dx``, one gate block of a parameter gradient), ``E_base`` that of
the same formulas in fp32 on the CPU with the kernels' declared bf16 roundings.  A slice that is
exactly zero in the reference must be exactly zero.  Each case runs with three losses: the output
alone, output + ``hT`` + ``cT``, and ``cT`` alone (the backward without an output gradient).
Both errors of every tensor go to ``$DINUNET_ERR_LOG`` (jsonl) when set;
``profiles/lstm_kernel_errors.md`` is one such run.

(b) ``dn_lstm_fwd``, ``dn_lstm_fwd_infer`` and ``dn_lstm_bwd`` called directly on buffers that are
views inside sentinel-filled allocations, checked bit for bit after the launches: a store out of
range shows up without a fault.

(c) Not covered here: ``DINUNET_LSTM_UG=3`` and ``DN_LSTM_BWD8_MINB`` (read once per process:
they need a child process; ``tests/test_lstm_infer_gpu.py`` runs the former's forward), the
compile-time variants ``LSTM_FLAGS``, ``LSTM_PRIO``, ``LSTM_POLY`` and ``BWD_CHAINS``, and
batches past 2 GiB, which ``tests/test_kernels_gpu.py`` keeps.

Measured on one MI355X (``profiles/lstm_kernel_errors.md``): the largest ratio ``E_kernel /
max(E_base, 2^-23)`` of any tensor is 1.38 (``dx`` at 1028 rows), and most are 1.00 to two
digits -- the kernels' errors are their declared roundings.  Run once against the deliberately
wrong references of ``tests/lstm_ref.py`` (``MUTATIONS``), every numerics test a mutation
reaches failed and no other did: a single sigmoid failed all 66, the unflipped reverse direction
every bidirectional case with ``S > 1``, ``mean_scale`` every ``mean`` case, ``no_dcT`` and
``dhT_first`` every loss with that term, the neighbour's ``hT`` every case with ``B > 1`` and
the o-gate block of ``dW_hh`` scaled by 1.1 every case where that block is not exactly zero.
(Scaled by 1.01 it passes: see ``tests/test_lstm_ref.py`` for what the rule resolves.)
"""
import json
import math
import os

import pytest
import torch

import lstm_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = -1232.0   # sentinel around every buffer (exact in bf16)
FILL = 7.0       # initial content of output buffers
PAD = 64
I = ref.I
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(autouse=True)
def _native():
    from dinunet_implementations_amd.ops import _lib
    if not _lib.native_available():
        pytest.fail("gfx950 kernel library not built")


def _L():
    from dinunet_implementations_amd.ops import lstm
    return lstm


def _lib():
    from dinunet_implementations_amd.ops import _lib as lib
    return lib


def _record(kind, case, e_k, e_b):
    path = os.environ.get("DINUNET_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"kind": kind, "case": case, "e_kernel": float(f"{e_k:.4g}"),
                                "e_base": float(f"{e_b:.4g}")}) + "\n")


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------
# (a) numerics through bilstm

def _dev_inputs(c):
    ps = [tuple(t.to(DEV).requires_grad_() for t in p) for p in c["params"]]
    return ps, c["x"].to(DEV).requires_grad_()


def _loss(c, loss, out, hT, cT):
    w = ref.loss_weights(c, loss)
    total = None
    for t, g in ((out, w["g_out"]), (hT, w["g_h"]), (cT, w["g_c"])):
        if g is not None:
            term = (t * g.to(DEV)).sum()
            total = term if total is None else total + term
    return total


def _collect(c, ps, x, out, hT, cT):
    torch.cuda.synchronize()
    fw = dict(out=out.detach(), hT=hT.detach(), cT=cT.detach(), mode=c["mode"])
    grads = dict(dx=x.grad)
    for i, k in enumerate(("dW_ih", "db_ih", "dW_hh", "db_hh")):
        grads[k] = [p[i].grad for p in ps]
    return fw, grads


def _run(c, loss, relu=False):
    """Forward and backward of a case through ``bilstm``; returns the kernel's ``(outputs,
    gradients, gate gradients [B*S, ndir*4HD] bf16)``."""
    L = _L()
    ps, x = _dev_inputs(c)
    seen = []
    real = L._lstm_backward

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append(r[1])
        return r
    L._lstm_backward = spy
    try:
        out, (hT, cT) = L.bilstm(x, ps, reduce=c["mode"], relu_input=relu)
        _loss(c, loss, out, hT, cT).backward()
    finally:
        L._lstm_backward = real
    fw, grads = _collect(c, ps, x, out, hT, cT)
    assert len(seen) == 1
    return fw, grads, seen[0]


def _compare(kind, shape, loss, got_fw, got_g, kw=None, rnd=ref.KERNEL):
    """Every tensor against the fp64 reference under the rule; all figures are printed and logged
    before the first assertion."""
    _, fw64, g64 = ref.solved(shape, kw, rnd, loss, fp64=True)
    _, fwb, gb = ref.solved(shape, kw, rnd, loss, fp64=False)
    ndir = shape[3]
    if got_g is None:
        g64 = gb = None
    bad = []
    for (name, k, got), (_, _, want), (_, _, base) in zip(ref.tensors(got_fw, got_g, ndir),
                                                          ref.tensors(fw64, g64, ndir),
                                                          ref.tensors(fwb, gb, ndir)):
        assert got is not None, f"{name}: no gradient"
        assert tuple(got.shape) == tuple(want.shape), name
        e_k, e_b = ref.slice_err(got, want, k, ndir), ref.slice_err(base, want, k, ndir)
        case = f"{shape} {loss} {name}"
        _record(kind, case, e_k, e_b)
        print(f"{kind} {case}: E_kernel {e_k:.3e} E_base {e_b:.3e}")
        if not ref.within_rule(e_k, e_b):
            bad.append((name, e_k, e_b))
    assert not bad, f"{kind} {shape} {loss}: E_kernel > 8 max(E_base, 2^-23): {bad}"


def _numerics(kind, shape, loss):
    c, _, _ = ref.solved(shape, None, ref.KERNEL, loss)
    fw, grads, _ = _run(c, loss)
    _compare(kind, shape, loss, fw, grads)


@pytest.mark.parametrize("loss", ref.LOSSES)
@pytest.mark.parametrize("shape", ref.RESIDENT, ids=str)
def test_resident_weights(shape, loss, monkeypatch):
    """64 / 128 / 192 padded units with W_hh in registers, both output modes, S = 1 and S = 2 (the
    recurrences are unrolled by two with a tail step), B = 1, padded units and partial
    workgroups."""
    monkeypatch.delenv("DN_LSTM_BR", raising=False)
    _numerics("resident", shape, loss)


@pytest.mark.parametrize("loss", ref.LOSSES)
@pytest.mark.parametrize("shape", ref.STREAMED, ids=str)
def test_streamed_weights(shape, loss):
    """256 / 384 / 512 padded units with W_hh streamed every step (two unit groups per wave from
    384 on)."""
    _numerics("streamed", shape, loss)


@pytest.mark.parametrize("loss", ref.LOSSES)
@pytest.mark.parametrize("shape,br_fwd,br_bwd", ref.ROW_TILING, ids=str)
def test_default_row_tiling(shape, br_fwd, br_bwd, loss, monkeypatch):
    """The rows-per-workgroup choice left to the library: 4-row forward with 8-row backward, the
    same batch range with ``B % 8 != 0`` (4 rows in both), and 8 rows at 64 units with a ragged
    last workgroup."""
    for k in ("DN_LSTM_BR", "DN_LSTM_BR_BWD_SAME"):
        monkeypatch.delenv(k, raising=False)
    lib = _lib().lib()
    B, Hd = shape[0], shape[2]
    assert int(lib.dn_lstm_rows_per_wg(B, Hd)) == br_fwd
    assert int(lib.dn_lstm_rows_per_wg_bwd(B, Hd)) == br_bwd
    if br_fwd == 8:
        assert B > 4096 and B % 8 != 0     # past the 64-unit threshold, ragged last workgroup
    else:
        assert B >= 1024 and (B % 8 == 0) == (br_bwd == 8)
    _numerics("row_tiling", shape, loss)


@pytest.mark.parametrize("loss", ref.LOSSES)
@pytest.mark.parametrize("br", ["8", "16"])
@pytest.mark.parametrize("shape", ref.BR_CASES, ids=str)
def test_rows_per_workgroup(shape, br, loss, monkeypatch):
    """``DN_LSTM_BR`` = 8 / 16 at 64, 128 and 192 units and in both modes: the forward that
    prefetches late and the backward that computes its activations after the MFMAs."""
    monkeypatch.setenv("DN_LSTM_BR", br)
    lib = _lib().lib()
    assert int(lib.dn_lstm_rows_per_wg(shape[0], shape[2])) == int(br)
    assert int(lib.dn_lstm_rows_per_wg_bwd(shape[0], shape[2])) == int(br)
    _numerics(f"br{br}", shape, loss)


def test_bf16_pre_activations(monkeypatch):
    """``DINUNET_LSTM_PRE_BF16=1``: the backward recomputes its gates from bf16 pre-activations;
    the baseline rounds them the same way.  Rows per workgroup as the library chooses."""
    L = _L()
    monkeypatch.delenv("DN_LSTM_BR", raising=False)
    monkeypatch.setattr(L, "PRE_BF16", "1")
    shape = ref.PRE_BF16_CASE
    assert L.pre_dtype(shape[0], shape[2], shape[4]) == BF16
    flags = []
    real = _lib().call

    def spy(name, *a):
        if name in ("dn_lstm_fwd", "dn_lstm_bwd"):
            flags.append((name, a[-2]))
        return real(name, *a)
    monkeypatch.setattr(_lib(), "call", spy)
    c, _, _ = ref.solved(shape, None, ref.KERNEL_PRE_BF16, "all")
    fw, grads, _ = _run(c, "all")
    assert flags == [("dn_lstm_fwd", 1), ("dn_lstm_bwd", 1)]
    _compare("pre_bf16", shape, "all", fw, grads, rnd=ref.KERNEL_PRE_BF16)
    # the forward's own gates never see the rounding: its outputs are those of the fp32 store
    monkeypatch.setattr(L, "PRE_BF16", "0")
    fw0, _, _ = _run(c, "all")
    for k in ("out", "hT", "cT"):
        assert _same_bits(fw[k], fw0[k]), k


@pytest.mark.parametrize("shape", ref.RELU_CASES, ids=str)
def test_relu_input_mask(shape):
    """``relu_input=True``: the ReLU mask rides in the input-gradient GEMM's epilogue."""
    kw = dict(relu=True)
    c, _, _ = ref.solved(shape, kw, ref.KERNEL, "all")
    fw, grads, _ = _run(c, "all", relu=True)
    dead = (c["x"] <= 0).to(DEV)
    assert 0.4 < float(dead.float().mean()) < 0.6
    assert bool((grads["dx"][dead] == 0).all())
    assert float((grads["dx"][~dead] != 0).float().mean()) > 0.99
    _compare("relu_input", shape, "all", fw, grads, kw=kw)


@pytest.mark.parametrize("shape", ref.RELU_CASES, ids=str)
def test_projection_as_its_own_node(shape):
    """``project(...)`` then ``bilstm(xp=...)``: the gradient that reaches ``xp`` is bitwise the
    gate gradients of the fused path, and the one that reaches ``x`` follows the rule."""
    L = _L()
    kw = dict(relu=True)
    c, _, _ = ref.solved(shape, kw, ref.KERNEL, "all")
    fw_f, g_f, dpre_f = _run(c, "all", relu=True)
    ps, x = _dev_inputs(c)
    packed = L.pack_params([t for p in ps for t in p], I, DEV)
    xp = L.project(x, packed, relu_input=True)
    xp.retain_grad()
    out, (hT, cT) = L.bilstm(x.detach(), ps, reduce=c["mode"], packed=packed, xp=xp,
                             relu_input=True)
    _loss(c, "all", out, hT, cT).backward()
    fw, grads = _collect(c, ps, x, out, hT, cT)
    assert xp.grad is not None and xp.grad.dtype == BF16 and float(xp.grad.float().abs().sum()) > 0
    assert _same_bits(xp.grad, dpre_f)
    for k in ("out", "hT", "cT"):
        assert _same_bits(fw[k], fw_f[k]), k
    assert bool((grads["dx"][(c["x"] <= 0).to(DEV)] == 0).all())
    _compare("project", shape, "all", fw, grads, kw=kw)


def test_saturated_gates():
    """Parameter scale 2 and input scale 4: most pre-activations lie past +-8.  The forward follows
    the rule; the gradients vanish, so they are only required to be finite."""
    shape = ref.SATURATED
    kw = ref.SATURATED_SCALES
    c, _, _ = ref.solved(shape, kw, ref.KERNEL, "all")
    fw, grads, _ = _run(c, "all")
    for name, _, t in ref.tensors(fw, grads, shape[3]):
        assert bool(torch.isfinite(t).all()), name
    _compare("saturated", shape, "all", fw, None, kw=kw)


# ---------------------------------------------------------------------------------------------
# (b) guards around every buffer of the direct calls

class Buf:
    """A 16-byte aligned view of ``dtype`` with ``PAD`` sentinel elements before and at least
    ``PAD`` after."""

    def __init__(self, shape, dtype=F32, init=None):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.raw = torch.full((PAD + n + PAD + 7,), SENT, dtype=dtype, device=DEV)
        self.v = self.raw[PAD:PAD + n].view(*shape)
        assert self.v.data_ptr() % 16 == 0
        self.init = None if init is None else init.to(DEV, dtype).reshape(shape).clone()
        if self.init is None:
            self.v.fill_(FILL)
        else:
            self.v.copy_(self.init)

    def ptr(self):
        return self.v.data_ptr()

    def intact(self):
        edge = torch.cat([self.raw[:PAD], self.raw[PAD + self.n:]])
        return _same_bits(edge, torch.full_like(edge, SENT))

    def untouched(self):
        want = torch.full_like(self.v, FILL) if self.init is None else self.init
        return _same_bits(self.v, want)


def _direct(c, pre_bf16):
    """The three entries called as ``ops.lstm`` calls them, every buffer a ``Buf``.  Returns the
    buffers and the case's geometry."""
    from dinunet_implementations_amd.ops.gemm import mm_plain
    L, lib = _L(), _lib()
    B, S, Hd, ndir = c["dims"]
    mode = c["mode"]
    HD = L.padded_hidden(Hd)
    GP = 4 * HD
    BR = int(lib.lib().dn_lstm_rows_per_wg(B, Hd))
    assert int(lib.lib().dn_lstm_rows_per_wg_bwd(B, Hd)) == BR
    Bp = (B + BR - 1) // BR * BR
    ps = [tuple(t.to(DEV) for t in p) for p in c["params"]]
    x = c["x"].to(DEV).to(BF16)
    packed = L.pack_params([t for p in ps for t in p], I, DEV)
    wih_p, bias_p, whh_p, whhT_p, _ = packed
    assert bias_p.numel() == ndir * GP
    w = ref.loss_weights(c, "all")
    oshape = (B, ndir * Hd)
    b = dict(
        xp=Buf((B * S, ndir * GP), BF16,
               mm_plain(x.reshape(B * S, I), wih_p, trans_b=True, out_dtype=BF16)),
        pre=Buf((B * S, ndir * GP), BF16 if pre_bf16 else F32),
        hT=Buf(oshape), cT=Buf(oshape), hT_i=Buf(oshape), cT_i=Buf(oshape),
        c_save=Buf((ndir, Bp, S, HD)), hprev=Buf((ndir, Bp, S, HD), BF16),
        dh_ext=Buf(tuple(w["g_out"].shape), F32, w["g_out"]),
        dhT=Buf(oshape, F32, w["g_h"]), dcT=Buf(oshape, F32, w["g_c"]),
        dpre=Buf((Bp * S, ndir * GP), BF16))
    if mode == "mean":
        b["out"], b["out_i"] = Buf(oshape), Buf(oshape)
        hseq = hseq_i = None
        hmean, hmean_i = b["out"].ptr(), b["out_i"].ptr()
        sb, stt, scale = ndir * Hd, 0, 1.0 / S
    else:
        b["out"], b["out_i"] = Buf((Bp, S, ndir * HD)), Buf((Bp, S, ndir * HD))
        hmean = hmean_i = None
        hseq, hseq_i = b["out"].ptr(), b["out_i"].ptr()
        sb, stt, scale = S * ndir * Hd, ndir * Hd, 1.0
    st = lib.stream()
    lib.call("dn_lstm_fwd", b["xp"].ptr(), bias_p.data_ptr(), whh_p.data_ptr(), B, S, Hd, ndir,
             b["c_save"].ptr(), b["hprev"].ptr(), hseq, hmean, 1.0 / S, b["hT"].ptr(),
             b["cT"].ptr(), b["pre"].ptr(), 0, int(pre_bf16), st)
    lib.call("dn_lstm_fwd_infer", b["xp"].ptr(), bias_p.data_ptr(), whh_p.data_ptr(), B, S, Hd,
             ndir, hseq_i, hmean_i, 1.0 / S, b["hT_i"].ptr(), b["cT_i"].ptr(), 0, st)
    torch.cuda.synchronize()
    saved = {k: b[k].v.clone() for k in ("pre", "c_save", "hprev")}
    lib.call("dn_lstm_bwd", b["pre"].ptr(), b["c_save"].ptr(), whhT_p.data_ptr(),
             b["dh_ext"].ptr(), sb, stt, scale, b["dhT"].ptr(), b["dcT"].ptr(), B, S, Hd, ndir,
             b["dpre"].ptr(), Bp, int(pre_bf16), st)
    torch.cuda.synchronize()
    return b, saved, packed, (B, S, Hd, HD, ndir, Bp, mode, x, ps)


def _guarded(shape, pre_bf16, monkeypatch):
    L = _L()
    monkeypatch.setattr(L, "PRE_BF16", "1" if pre_bf16 else "0")
    c, _, _ = ref.solved(shape, None, ref.KERNEL, "all")
    b, saved, packed, (B, S, Hd, HD, ndir, Bp, mode, x, ps) = _direct(c, pre_bf16)
    for k, buf in b.items():
        assert buf.intact(), f"{k}: a guard was overwritten"
    for k in ("xp", "dh_ext", "dhT", "dcT"):
        assert b[k].untouched(), f"{k}: an input changed"
    for k, t in saved.items():     # the backward reads what the forward stored
        assert _same_bits(b[k].v, t), f"{k}: changed by the backward"
    assert not b["dpre"].untouched() and not b["pre"].untouched()
    dpre = b["dpre"].v.view(Bp, S, ndir, HD, 4)
    assert bool((dpre[:, :, :, Hd:] == 0).all()), "dpre of padded units"
    assert bool((dpre[B:] == 0).all()), "dpre of padded rows"
    assert bool(torch.isfinite(dpre.float()).all())
    # h_{-1} = 0 at the first step of each direction, exactly
    assert bool((b["hprev"].v[0, :B, 0] == 0).all())
    if ndir == 2:
        assert bool((b["hprev"].v[1, :B, S - 1] == 0).all())

    def public(t):
        if mode == "mean":
            return t
        return t.view(Bp, S, ndir, HD)[:B, :, :, :Hd].reshape(B, S, ndir * Hd)
    # the forward-only entry gives the storing entry's outputs
    assert _same_bits(public(b["out_i"].v), public(b["out"].v))
    assert _same_bits(b["hT_i"].v, b["hT"].v) and _same_bits(b["cT_i"].v, b["cT"].v)
    # and both are the bilstm path's, with its gate gradients
    seen = []
    real = L._lstm_backward

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append(r[1])
        return r
    monkeypatch.setattr(L, "_lstm_backward", spy)
    psg = [tuple(t.clone().requires_grad_() for t in p) for p in ps]
    out, (hT, cT) = L.bilstm(x, psg, reduce=mode, packed=packed, xp=b["xp"].v)
    _loss(c, "all", out, hT, cT).backward()
    torch.cuda.synchronize()
    assert _same_bits(out.detach(), public(b["out"].v))
    assert _same_bits(hT.detach(), b["hT"].v) and _same_bits(cT.detach(), b["cT"].v)
    assert len(seen) == 1 and _same_bits(seen[0], b["dpre"].v[:B * S])
    return c, b


GUARD_SHAPES = [(5, 3, 32, 2), (13, 4, 174, 2), (3, 2, 300, 1)]


@pytest.mark.parametrize("mode", ["mean", "seq"])
@pytest.mark.parametrize("shape", GUARD_SHAPES, ids=str)
def test_guards(shape, mode, monkeypatch):
    monkeypatch.delenv("DN_LSTM_BR", raising=False)
    _guarded(shape + (mode,), False, monkeypatch)


@pytest.mark.parametrize("mode", ["mean", "seq"])
def test_guards_16_rows(mode, monkeypatch):
    monkeypatch.setenv("DN_LSTM_BR", "16")
    assert int(_lib().lib().dn_lstm_rows_per_wg(19, 100)) == 16
    _guarded((19, 3, 100, 2, mode), False, monkeypatch)


def test_guards_bf16_pre_activations(monkeypatch):
    """bf16 ``pre`` is offered at 192 padded units with the temporal mean only."""
    monkeypatch.delenv("DN_LSTM_BR", raising=False)
    lib = _lib().lib()
    used = [int(lib.dn_lstm_pre_bf16_used(*a)) for a in ((174, 0), (174, 1), (32, 0), (300, 0))]
    assert used == [1, 0, 0, 0]
    _guarded((13, 4, 174, 2, "mean"), True, monkeypatch)


def test_error_log_format(tmp_path, monkeypatch):
    p = tmp_path / "err.jsonl"
    monkeypatch.setenv("DINUNET_ERR_LOG", str(p))
    _record("k", "c", 1.23456e-3, 2e-3)
    row = json.loads(p.read_text())
    assert row == {"kind": "k", "case": "c", "e_kernel": 1.235e-3, "e_base": 2e-3}
    assert math.isclose(row["e_kernel"] / row["e_base"], 0.6175)
