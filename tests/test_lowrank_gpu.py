"""The low-rank gradient kernels of ``csrc/kernels/lowrank.hip`` called directly, one process, each
against the fp64 reference of ``tests/lowrank_ref.py``.

Tolerance (every compared quantity): ``e_kernel <= 8 max(e_base, 2^-23)``, relative Frobenius
errors against fp64, ``e_base`` the error of the same formula in fp32 on the CPU (for the
persistent kernel: with its declared bf16 hi/lo split products).  Both errors of every case go
to ``$DINUNET_ERR_LOG`` (jsonl) when set; ``profiles/lowrank_kernel_errors.md`` is one such run.

Every device buffer the kernels see is a 16-byte aligned view inside a larger tensor with 64
floats of a fixed sentinel on both sides, checked bit for bit after the launches: a store out of
range shows up without a fault.  Bases aligned to 4 or 8 bytes only are out of scope here.

Measured on one MI355X (``profiles/lowrank_kernel_errors.md``): the largest ratio ``e_kernel /
max(e_base, 2^-23)`` of any case is 1.72.  "Exactly zero" for a dropped column means ``== 0.0``:
the kernels form it as the column times a zero factor, so its entries carry either sign.
"""
import functools
import json
import math
import os

import pytest
import torch

import lowrank_ref as ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENT = -1234.5   # sentinel around every buffer
FILL = 7.0       # initial content of output buffers (so "untouched" can be told)
PAD = 64
F64 = torch.float64
F32 = torch.float32


def _lr():
    from dinunet_implementations_amd.parallel import lowrank
    return lowrank


def _record(kind, case, e_k, e_b):
    path = os.environ.get("DINUNET_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"kind": kind, "case": case, "e_kernel": float(f"{e_k:.4g}"),
                                "e_base": float(f"{e_b:.4g}")}) + "\n")


def _close(kind, case, got, ref64, base):
    e_k, e_b = ref.relerr(got, ref64), ref.relerr(base, ref64)
    _record(kind, case, e_k, e_b)
    print(f"{kind} {case}: e_kernel {e_k:.3e} e_base {e_b:.3e}")
    ref.assert_close(got, ref64, base, f"{kind} {case}")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _all_zero(t):
    """Every entry is 0.0 (a dropped column is its value times a zero factor: either sign)."""
    return bool((t == 0).all())


class Buf:
    """A 16-byte aligned fp32 view with ``PAD`` sentinel floats before and at least ``PAD`` after."""

    def __init__(self, shape, init=None):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.raw = torch.full((PAD + n + PAD + 3,), SENT, dtype=F32, device=DEV)
        self.v = self.raw[PAD:PAD + n].view(*shape)
        assert self.v.data_ptr() % 16 == 0
        self.init = None if init is None else init.to(DEV, F32).reshape(shape).clone()
        self.reset()

    def reset(self):
        if self.init is None:
            self.v.fill_(FILL)
        else:
            self.v.copy_(self.init)

    def intact(self):
        s = torch.tensor([SENT], dtype=F32).view(torch.int32).item()
        edge = torch.cat([self.raw[:PAD], self.raw[PAD + self.n:]]).view(torch.int32)
        return bool((edge == s).all())

    def untouched(self):
        want = torch.full_like(self.v, FILL) if self.init is None else self.init
        return _same_bits(self.v, want)


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


class Layer:
    def __init__(self, shape, G=None, Q0=None, err=None, P=None, seed=0):
        out_f, in_f, r = shape
        self.shape = shape
        self.G0 = _randn((out_f, in_f), 100 + seed) if G is None else G
        self.Q0 = ref.rand_orth(in_f, r, 200 + seed) if Q0 is None else Q0
        self.G = Buf((out_f, in_f), self.G0)
        self.err = None if err is None else Buf((out_f, in_f), err)
        self.P = Buf((out_f, r), P)
        self.Ps = Buf((out_f, r))
        self.Qs = Buf((in_f, r), self.Q0)

    def entry(self):
        return (self.G.v, None if self.err is None else self.err.v, self.P.v, self.Ps.v, self.Qs.v)

    def bufs(self):
        return [b for b in (self.G, self.err, self.P, self.Ps, self.Qs) if b is not None]

    def reset(self):
        for b in self.bufs():
            b.reset()

    def intact(self):
        return all(b.intact() for b in self.bufs())

    def untouched(self):
        return all(b.untouched() for b in self.bufs())

    def snap(self):
        return [b.v.clone() for b in (self.P, self.Ps, self.Qs)]

    def product(self):
        return self.Ps.v.double().cpu() @ self.Qs.v.double().cpu().t()


def _table(layers):
    return _lr().LowRankTable([l.entry() for l in layers], DEV)


def _sync_intact(layers):
    torch.cuda.synchronize()
    for i, l in enumerate(layers):
        assert l.intact(), f"layer {i} {l.shape}: a store outside its buffers"


def _staged(t, iters, tol=0.0, after=None):
    for it in range(iters):
        t.gq(it, tol)
        t.orth_gtp(it)
        if after is not None:
            after(it)


def _prod(Pn, Q):
    return Pn.double() @ Q.double().t()


def _check_factors(kind, case, layer, want, base):
    """``Psend Qsend^T`` and ``Psend^T Psend`` against the reference ``(Pn, Q)`` pairs; the
    columns the reference dropped are exactly zero in ``Psend`` and ``Qsend``, the others live."""
    dead = (want[0] == 0).all(0)
    # a baseline that drops other columns than fp64 would only loosen the bound: it must not
    assert ref.dropped(base[0]) == dead.tolist(), f"{kind} {case}: the baseline's dropped columns"
    live = [c for c in range(layer.shape[2]) if not bool(dead[c])]
    for buf in (layer.Ps, layer.Qs):
        assert (buf.v == 0).all(0).cpu().tolist() == dead.tolist(), f"{kind} {case}: dropped columns"
    _close(kind + ".PQt", case, layer.product(), _prod(*want), _prod(*base))
    eye = torch.eye(len(live), dtype=F64)
    _close(kind + ".orth", case, ref.orthonormality(layer.Ps.v, live), eye,
           ref.orthonormality(base[0], live))


@functools.lru_cache(maxsize=None)
def _gapped_case(shape, iters=5, seed=31, split=False):
    G, Q0 = ref.gapped_case(shape, seed)
    want = ref.power_iterate(G, Q0, iters, 0.0)[:2]
    base = ref.power_iterate(G, Q0, iters, 0.0, dtype=F32, mm=ref.split3 if split else torch.matmul)[:2]
    return G, Q0, want, base


@functools.lru_cache(maxsize=None)
def _tol_refs(shape, split=False):
    G, Q0, tol, k, ch = ref.tol_case(shape)
    want = ref.power_iterate(G, Q0, ref.TOL_ITERS, tol)
    base = ref.power_iterate(G, Q0, ref.TOL_ITERS, tol, dtype=F32,
                             mm=ref.split3 if split else torch.matmul)
    assert want[2] == k + 1 == base[2]
    return G, Q0, tol, k, want[:2], base[:2]


# ---------------------------------------------------------------------------------------------
# lr_gq: P = (G + err) Q

GQ_SHAPES = [
    (7, 5, 3),        # tiny, out < 16, not VEC, not qvec
    (16, 16, 4),      # smallest aligned case
    (256, 66, 10),    # the FS first layer: not VEC
    (33, 66, 3),      # in * r = 198: not qvec
    (33, 1000, 3),    # both buffers in flight, wave 0 has exactly 2U chunks
    (20, 1024, 16),   # in * r = 16384: the QL boundary, the full LR_STV staging
    (20, 1040, 16),   # not QL, VEC, third issue
    (48, 1030, 16),   # not QL and not VEC
    (17, 2068, 4),    # second trip of the loop, both buffers re-issued
]


@pytest.mark.parametrize("with_err", [False, True], ids=["dad", "ef"])
@pytest.mark.parametrize("shape", GQ_SHAPES, ids=str)
def test_lr_gq(shape, with_err):
    out_f, in_f, r = shape
    err = 0.25 * _randn((out_f, in_f), 7) if with_err else None
    L = Layer(shape, err=err, seed=1)
    t = _table([L])
    m_dev = (L.G.v + L.err.v).clone() if with_err else L.G.v.clone()
    t.gq(0)
    _sync_intact([L])
    _, p64 = ref.gq(L.G0, L.Q0, err)
    _, p32 = ref.gq(L.G0, L.Q0, err, dtype=F32)
    _close("lr_gq", f"{shape} err={int(with_err)}", L.P.v, p64, p32)
    assert _same_bits(L.G.v, m_dev)                 # M = G + err in fp32, or G unchanged
    if with_err:
        assert L.err.untouched()
    assert L.Qs.untouched() and L.Ps.untouched()
    assert t.iterations() == [1] and t.active[:1].tolist() == [1]


# ---------------------------------------------------------------------------------------------
# lr_gtp: Pn = P R^-1, Q = G^T Pn, change norms

GTP_SHAPES = [  # round boundaries in out (256 / 512 / 768 rows), r == R and r < R, pvec on / off
    (1, 5, 1), (15, 16, 3), (17, 66, 4), (255, 16, 5),
    (256, 100, 8), (257, 66, 5), (25, 66, 10), (513, 16, 13),
    (769, 20, 16), (1024, 16, 16),   # out * r = 16384 = LR_PLDS
    (1025, 16, 8), (4096, 5, 4),
]


def _gtp_check(kind, case, L, t, P, Qprev, dropped=()):
    out_f, in_f, r = L.shape
    want = ref.gtp(L.G0, P, Qprev)
    base = ref.gtp(L.G0, P, Qprev, dtype=F32)
    live = [c for c in range(r) if c not in dropped]
    for name, buf, w, b in (("Psend", L.Ps, want[0], base[0]), ("Qsend", L.Qs, want[1], base[1])):
        got = buf.v.cpu()
        assert torch.isfinite(got).all(), f"{kind} {case}: {name} not finite"
        if dropped:
            assert _all_zero(got[:, list(dropped)]), \
                f"{kind} {case}: dropped columns of {name} are not exactly 0.0"
        if live:
            _close(f"{kind}.{name}", case, got[:, live], w[:, live], b[:, live])
    norms = t._keep[0].view(-1, 2).cpu()
    assert torch.isfinite(norms).all()
    if live:
        _close(kind + ".norms", case, norms, want[2], base[2])
        eye = torch.eye(len(live), dtype=F64)
        _close(kind + ".orth", case, ref.orthonormality(L.Ps.v, live), eye,
               ref.orthonormality(base[0], live))
    else:
        assert float(norms[:, 1].abs().max()) == 0.0
    assert L.G.untouched() and L.P.untouched()


@pytest.mark.parametrize("shape", GTP_SHAPES, ids=str)
def test_lr_gtp(shape):
    out_f, in_f, r = shape
    P = ref.rand_p(out_f, r, 41)
    Qprev = _randn((in_f, r), 42)
    L = Layer(shape, Q0=Qprev, P=P, seed=2)
    t = _table([L])
    t.orth_gtp(0)
    _sync_intact([L])
    _gtp_check("lr_gtp", str(shape), L, t, P, Qprev)


@pytest.mark.parametrize("name", ["copy", "zero_col", "all_zero"])
def test_lr_gtp_dropped_columns(name):
    P, dropped = ref.drop_p_cases()[name]
    shape = ref.DROP_SHAPE
    Qprev = _randn((shape[1], shape[2]), 43)
    L = Layer(shape, Q0=Qprev, P=P, seed=3)
    t = _table([L])
    t.orth_gtp(0)
    _sync_intact([L])
    _gtp_check("lr_gtp.drop", name, L, t, P, Qprev, dropped)


def test_rank_deficient_gradient():
    """G of exact rank 2 at r = 4: two columns drop (dependent at the first iteration, vanished
    afterwards); the live pair still reproduces G."""
    shape = (48, 66, 4)
    G = ref.exact_rank2(48, 66, 7)
    Q0 = ref.rand_orth(66, 4, 8)
    L = Layer(shape, G=G, Q0=Q0)
    t = _table([L])
    _staged(t, 3)
    _sync_intact([L])
    want = ref.power_iterate(G, Q0, 3)[:2]
    base = ref.power_iterate(G, Q0, 3, dtype=F32)[:2]
    for buf, w, b, nm in ((L.Ps, want[0], base[0], "Psend"), (L.Qs, want[1], base[1], "Qsend")):
        got = buf.v.cpu()
        assert torch.isfinite(got).all()
        assert _all_zero(got[:, 2:]), nm
        _close("rank2." + nm, str(shape), got[:, :2], w[:, :2], b[:, :2])
    _close("rank2.PQt", str(shape), L.product(), G.double(), _prod(*base))
    assert torch.isfinite(L.P.v).all() and t.iterations() == [3]


def test_zero_gradient():
    shape = (48, 66, 4)
    L = Layer(shape, G=torch.zeros(48, 66))
    t = _table([L])
    _staged(t, 3)
    _sync_intact([L])
    for buf in (L.P, L.Ps, L.Qs):
        assert _all_zero(buf.v)
    assert _all_zero(t._keep[0])
    assert t.iterations() == [3]


# ---------------------------------------------------------------------------------------------
# the staged power iteration

@pytest.mark.parametrize("shape", ref.STAGED_SHAPES, ids=str)
def test_staged_iteration(shape):
    G, Q0, want, base = _gapped_case(shape)
    L = Layer(shape, G=G, Q0=Q0)
    t = _table([L])
    _staged(t, 5)
    _sync_intact([L])
    _check_factors("staged", str(shape), L, want, base)
    assert t.iterations() == [5] and L.G.untouched()


@pytest.mark.parametrize("shape", ref.TOL_STAGED, ids=str)
def test_staged_dad_tol(shape):
    G, Q0, tol, k, want, base = _tol_refs(shape)
    L = Layer(shape, G=G, Q0=Q0)
    t = _table([L])
    snaps = []
    _staged(t, ref.TOL_ITERS, tol, after=lambda it: snaps.append(L.snap()))
    _sync_intact([L])
    assert t.iterations() == [k + 1]
    assert t.active[:1].tolist() == [0]
    for got, at_stop in zip(L.snap(), snaps[k]):   # the factors of the stopping iteration
        assert _same_bits(got, at_stop)
    assert not _same_bits(snaps[k][2], snaps[k - 1][2])
    _check_factors("staged.tol", str(shape), L, want, base)
    # a second sequence re-activates the layer; from the converged Q it stops after one iteration
    ch2 = ref.power_iterate(G, want[1], 2, 0.0)[3]
    assert ch2[0] * 3 <= tol
    t.gq(0, tol)
    assert t.active[:1].tolist() == [1] and t.iterations() == [k + 2]
    t.orth_gtp(0)
    for it in range(1, ref.TOL_ITERS):
        t.gq(it, tol)
        t.orth_gtp(it)
    _sync_intact([L])
    assert t.iterations() == [k + 2] and t.active[:1].tolist() == [0]


def test_stopped_layer_is_left_alone():
    """Two layers, one ``tol``: the first converges early, the second never does; the later
    launches leave the stopped layer's P, Psend and Qsend bit-unchanged."""
    sa, sb = (48, 66, 4), (40, 100, 8)
    G, Q0, tol, k, want, base = _tol_refs(sa)
    Gb = _randn((40, 100), 51)
    Qb = ref.rand_orth(100, 8, 52)
    wb = ref.power_iterate(Gb, Qb, ref.TOL_ITERS, 0.0)
    assert min(wb[3]) >= 3 * tol            # the flat spectrum keeps the change far above tol
    bb = ref.power_iterate(Gb, Qb, ref.TOL_ITERS, 0.0, dtype=F32)
    A, B = Layer(sa, G=G, Q0=Q0), Layer(sb, G=Gb, Q0=Qb)
    t = _table([A, B])
    snaps = []
    _staged(t, ref.TOL_ITERS, tol, after=lambda it: snaps.append(A.snap()))
    _sync_intact([A, B])
    assert t.iterations() == [k + 1, ref.TOL_ITERS]
    assert t.active[:2].tolist() == [0, 1]
    for got, at_stop in zip(A.snap(), snaps[k]):
        assert _same_bits(got, at_stop)
    _check_factors("two_layer.stopped", str(sa), A, want, base)
    _check_factors("two_layer.running", str(sb), B, wb[:2], bb[:2])


# ---------------------------------------------------------------------------------------------
# PowerSGD: gq, orth_gtp, recon_ef with error feedback

def _psgd_ref(Gs, Q0, dtype):
    """Two steps of ``gq / cholqr / G^T Pn / recon_ef``; returns per step ``(M, Pn, Q, G')``."""
    err = torch.zeros_like(Gs[0], dtype=dtype)
    Q = Q0.to(dtype)
    steps = []
    for G in Gs:
        M, P = ref.gq(G, Q, err, dtype=dtype)
        Pn, Q, _ = ref.gtp(M, P, Q, dtype=dtype)
        Gn, err = ref.recon_ef(M, Pn, Q, dtype=dtype)
        steps.append((M, Pn, Q, Gn))
    return steps


def _psgd_run(layers, t, Gs_per_layer, check):
    for step in range(2):
        for L, Gs in zip(layers, Gs_per_layer):
            L.G.v.copy_(Gs[step].to(DEV))
        pre = [(L.G.v + L.err.v).clone() for L in layers]
        t.gq(0)
        t.orth_gtp(0)
        ms = [L.G.v.clone() for L in layers]
        t.recon_ef()
        _sync_intact(layers)
        for i, L in enumerate(layers):
            assert _same_bits(ms[i], pre[i])                       # M = G + err (err of step 1)
            assert _same_bits(L.err.v, ms[i] - L.G.v)              # err' = M - G'
            check(i, step, L)


@pytest.mark.parametrize("shape", [(256, 66, 4), (33, 1000, 2), (20, 1040, 16), (7, 5, 3)], ids=str)
def test_powersgd_sequence(shape):
    out_f, in_f, r = shape
    Gs = [_randn((out_f, in_f), 61), _randn((out_f, in_f), 62)]
    L = Layer(shape, G=Gs[0], err=torch.zeros(out_f, in_f), seed=6)
    t = _table([L])
    want, base = _psgd_ref(Gs, L.Q0, F64), _psgd_ref(Gs, L.Q0, F32)

    def check(i, step, L):
        _close("powersgd.G", f"{shape} step={step}", L.G.v, want[step][3], base[step][3])
        _close("powersgd.err", f"{shape} step={step}", L.err.v, want[step][0] - want[step][3],
               base[step][0] - base[step][3])
    _psgd_run([L], t, [Gs], check)


# ---------------------------------------------------------------------------------------------
# tables of more than LR_KMAX layers, mixed ranks

MIX, NMIX = ref.MIX, ref.NMIX   # 19 layers: launches of 16 + 3, lr_gtp<16> and lr_gtp<8>


def _cls(r):
    return 4 if r <= 4 else 8 if r <= 8 else 16


def _mix_layers(err):
    """rank-dAD: gapped spectra (three iterations converge on them).  PowerSGD runs ONE iteration
    per step: from a random start on a graded spectrum cond(P) is the spectrum's whole spread and
    the error feedback carries the first step's rounding into the second, so its gradients are
    Gaussian (cond(P) of a few), as in ``test_powersgd_sequence``."""
    layers = []
    for i in range(NMIX):
        shape = MIX[i % len(MIX)]
        if err:
            layers.append(Layer(shape, err=torch.zeros(shape[0], shape[1]), seed=70 + i))
        else:
            G, Q0, _, _ = _gapped_case(shape, 3, 70 + i)
            layers.append(Layer(shape, G=G, Q0=Q0))
    return layers


def _alone(layers, i, err):
    """Layer i in a table of its own whose lr_gtp launch has the rank class of its launch in the
    large table (a filler layer of that class where its own rank is of a lower one)."""
    lo = 16 * (i // 16)
    cls = _cls(max(l.shape[2] for l in layers[lo:lo + 16]))
    src = layers[i]
    one = Layer(src.shape, G=src.G0, Q0=src.Q0,
                err=torch.zeros(src.shape[0], src.shape[1]) if err else None)
    group = [one]
    if _cls(src.shape[2]) != cls:
        group.append(Layer((16, 16, cls), err=torch.zeros(16, 16) if err else None, seed=9))
    return one, group


def test_large_mixed_table_rankdad():
    layers = _mix_layers(False)
    t = _table(layers)
    _staged(t, 3)
    _sync_intact(layers)
    assert t.iterations() == [3] * NMIX
    first = [l.snap() for l in layers]
    for i, L in enumerate(layers):
        _, _, want, base = _gapped_case(L.shape, 3, 70 + i)
        _check_factors("mixed19", f"{i} {L.shape}", L, want, base)
    for l in layers:                                   # the same inputs again: the same bits
        l.reset()
    _staged(t, 3)
    _sync_intact(layers)
    for l, s in zip(layers, first):
        assert all(_same_bits(a, b) for a, b in zip(l.snap(), s))
    for i in range(NMIX):                              # and the bits of the layer on its own
        one, group = _alone(layers, i, False)
        _staged(_table(group), 3)
        _sync_intact(group)
        assert all(_same_bits(a, b) for a, b in zip(one.snap(), first[i])), (i, one.shape)


def test_large_mixed_table_powersgd():
    layers = _mix_layers(True)
    t = _table(layers)
    Gs = [[l.G0, _randn(l.shape[:2], 300 + i)] for i, l in enumerate(layers)]
    refs = [(_psgd_ref(g, l.Q0, F64), _psgd_ref(g, l.Q0, F32)) for g, l in zip(Gs, layers)]
    got = {}

    def check(i, step, L):
        want, base = refs[i]
        _close("mixed19.powersgd.G", f"{i} {L.shape} step={step}", L.G.v, want[step][3], base[step][3])
        got[(i, step)] = (L.G.v.clone(), L.err.v.clone())
    _psgd_run(layers, t, Gs, check)
    for i in range(NMIX):
        one, group = _alone(layers, i, True)
        gs = [Gs[i]] + [[g.G0, g.G0] for g in group[1:]]

        def same(j, step, L, i=i):
            if j == 0:
                assert _same_bits(L.G.v, got[(i, step)][0]) and _same_bits(L.err.v, got[(i, step)][1])
        _psgd_run(group, _table(group), gs, same)


def test_table_limits():
    with pytest.raises(ValueError):
        _table([Layer((32, 32, 17))])
    with pytest.raises(ValueError):
        _table([Layer((1025, 16, 16))])       # out * r = 16400 > 16384


# ---------------------------------------------------------------------------------------------
# lr_persist: every iteration of every layer in one launch

PERSIST_SHAPES = [      # (= ref.PERSIST_SHAPES) members J by lp_plan's rule, and the instantiation
    (48, 64, 4),        # J = 1, <4, EX>: single member
    (40, 64, 3),        # J = 1, <4, !EX>: r < R
    (256, 1000, 10),    # J = 16, <10, EX>: the ICA model's largest layer
    (272, 1024, 16),    # J = 32, <16, EX>: serial Gram tail (q >= GV), members 17.. without rows
    (25, 132, 10),      # J = 3, <10, EX>: ragged out * r = 250, a 4-column last block, member 2
                        #        without rows
    (1024, 64, 12),     # J = 16, <12, EX>: out * r = 12288 > 8192, the series P staging
    (64, 64, 13),       # J = 1, <16, !EX>: r < R at the top bound
]


assert PERSIST_SHAPES == ref.PERSIST_SHAPES


def _persist_clean(t):
    torch.cuda.synchronize()
    assert t.persist_error() == 0
    assert int(t._persist[2].abs().sum().item()) == 0      # barrier counters back to zero


@pytest.mark.parametrize("shape", PERSIST_SHAPES, ids=str)
def test_lr_persist(shape):
    G, Q0, want, base = _gapped_case(shape, 5, 31, True)
    L = Layer(shape, G=G, Q0=Q0)
    t = _table([L])
    assert t.persist(5, 0.0) is True
    _sync_intact([L])
    _persist_clean(t)
    _check_factors("persist", str(shape), L, want, base)
    assert t.iterations() == [5] and L.G.untouched()
    first = L.snap()
    L.reset()
    assert t.persist(5, 0.0) is True                      # the same inputs again: the same bits
    _sync_intact([L])
    _persist_clean(t)
    assert all(_same_bits(a, b) for a, b in zip(L.snap(), first))
    assert t.iterations() == [10]


@pytest.mark.parametrize("shape", ref.TOL_PERSIST, ids=str)
def test_lr_persist_dad_tol(shape):
    G, Q0, tol, k, want, base = _tol_refs(shape, True)
    L = Layer(shape, G=G, Q0=Q0)
    t = _table([L])
    assert t.persist(ref.TOL_ITERS, tol) is True
    _sync_intact([L])
    _persist_clean(t)
    assert t.iterations() == [k + 1]
    _check_factors("persist.tol", str(shape), L, want, base)


def test_lr_persist_mixed_ranks():
    """8 layers of ranks 8 and 5: <8, !EX>."""
    shapes = ref.MIXED8
    cases = [_gapped_case(s, 5, 90 + i, True) for i, s in enumerate(shapes)]
    layers = [Layer(s, G=c[0], Q0=c[1]) for s, c in zip(shapes, cases)]
    t = _table(layers)
    assert t.persist(5, 0.0) is True
    _sync_intact(layers)
    _persist_clean(t)
    assert t.iterations() == [5] * 8
    for i, (L, c) in enumerate(zip(layers, cases)):
        _check_factors("persist.mixed8", f"{i} {L.shape}", L, c[2], c[3])


def _refused(layers, t):
    assert t.persist(5, 0.0) is False
    _sync_intact(layers)
    assert all(l.untouched() for l in layers)
    assert t.iterations() == [0] * len(layers)
    assert int(t._persist[2].abs().sum().item()) == 0


def test_lr_persist_refuses_nine_layers():
    layers = [Layer((16, 16, 4), seed=i) for i in range(9)]
    _refused(layers, _table(layers))


def test_lr_persist_refuses_unaligned_in():
    layers = [Layer((16, 16, 4)), Layer((32, 66, 4))]
    _refused(layers, _table(layers))


def test_lr_persist_env_switch(monkeypatch):
    monkeypatch.setenv("DINUNET_LR_PERSIST", "0")
    layers = [Layer((16, 16, 4))]
    _refused(layers, _table(layers))


# ---------------------------------------------------------------------------------------------
# dn_pi_reconstruct: G = sum_s P_s Q_s^T / W

def _recon_setup(shapes, W):
    off, slots = 0, []
    for out_f, in_f, r in shapes:
        qo = off + -(-out_f * r // 4) * 4          # every factor base 16-byte aligned
        slots.append((off, qo))
        off = qo + -(-in_f * r // 4) * 4
    S = -(-off // 8) * 8 + 8
    gathered = Buf((W * S,), 0.5 * _randn((W * S,), 81))
    Gs = [Buf((s[0], s[1])) for s in shapes]
    base = gathered.v.data_ptr()
    recs = [(g.v.data_ptr(), base + 4 * po, base + 4 * qo, s[0], s[1], s[2])
            for g, s, (po, qo) in zip(Gs, shapes, slots)]
    return S, gathered, Gs, recs, slots


@pytest.mark.parametrize("W", [1, 2, 3, 5])
@pytest.mark.parametrize("table", ["four", "sixteen"])
def test_pi_reconstruct(W, table):
    shapes = [(7, 5, 3), (256, 66, 10), (33, 1000, 16), (64, 64, 4)]
    if table == "sixteen":
        shapes = [(7, 5, 3), (33, 66, 10), (17, 100, 16), (64, 64, 4)] * 4
    S, gathered, Gs, recs, slots = _recon_setup(shapes, W)
    tab = _lr().PiReconTable(recs, DEV)
    tab.run(S, W)
    torch.cuda.synchronize()
    assert gathered.intact() and gathered.untouched()
    flat = gathered.v.cpu()
    for i, (g, s, (po, qo)) in enumerate(zip(Gs, shapes, slots)):
        assert g.intact()
        Ps = [flat[w * S + po:w * S + po + s[0] * s[2]].view(s[0], s[2]) for w in range(W)]
        Qs = [flat[w * S + qo:w * S + qo + s[1] * s[2]].view(s[1], s[2]) for w in range(W)]
        _close("pi_reconstruct", f"W={W} {table} {i} {s}", g.v, ref.pi_reconstruct(Ps, Qs),
               ref.pi_reconstruct(Ps, Qs, dtype=F32))


def test_pi_reconstruct_layer_limit():
    shapes = [(16, 16, 4)] * 17
    S, gathered, Gs, recs, _ = _recon_setup(shapes, 2)
    tab = _lr().PiReconTable(recs, DEV)
    with pytest.raises(RuntimeError):
        tab.run(S, 2)
    torch.cuda.synchronize()
    assert all(g.untouched() and g.intact() for g in Gs)


# ---------------------------------------------------------------------------------------------
# dn_mgs_batched through orthonormalize_

def test_mgs_batched():
    dims = [(768, 16),    # n * r = 12288: the last size kept in LDS
            (769, 16), (3000, 8),   # outside LDS
            (5, 5), (40, 1)]
    bufs = [Buf(d, _randn(d, 90 + i)) for i, d in enumerate(dims)]
    strided = Buf((50, 9), _randn((50, 9), 97))       # [50, 6] view with ld = r + 3
    zero = _randn((64, 4), 98)
    zero[:, 2] = 0.0
    zbuf = Buf((64, 4), zero)
    mats = [b.v for b in bufs] + [strided.v[:, :6], zbuf.v]
    srcs = [b.init.cpu() for b in bufs] + [strided.init[:, :6].cpu(), zero]
    assert mats[5].stride(0) == 9
    _lr().orthonormalize_(mats)
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs + [strided, zbuf])
    for i, (m, s) in enumerate(zip(mats, srcs)):
        assert torch.isfinite(m).all()
        _close("mgs", f"{i} {tuple(s.shape)} ld={m.stride(0)}", m, ref.mgs(s), ref.mgs(s, dtype=F32))
    assert _same_bits(strided.v[:, 6:], strided.init[:, 6:])
    assert _all_zero(zbuf.v[:, 2])


# ---------------------------------------------------------------------------------------------
# graph capture of the staged iteration with the device-side stop

def test_graph_capture_matches_eager():
    """4 iterations captured on one stream (a linear chain of 8 launches, no parallel branches),
    ``tol`` between the changes of iterations 1 and 2: the layer stops inside the graph."""
    shape = (256, 66, 10)
    G, Q0, _, _, ch = ref.tol_case(shape)
    tol = math.sqrt(ch[1] * ch[2])
    assert ch[1] / tol >= 3 and tol / ch[2] >= 3
    L = Layer(shape, G=G, Q0=Q0)
    t = _table([L])
    _staged(t, 4, tol)
    _sync_intact([L])
    eager, it_eager = L.snap(), t.iterations()
    assert it_eager == [3] and t.active[:1].tolist() == [0]
    L.reset()
    t.iters.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _staged(t, 4, tol)
    for _ in range(2):
        L.reset()
        t.iters.zero_()
        g.replay()
        _sync_intact([L])
        assert all(_same_bits(a, b) for a, b in zip(L.snap(), eager))
        assert t.iterations() == it_eager and t.active[:1].tolist() == [0]
