"""Plain torch reference of the GEMM (``csrc/kernels/gemm.hip`` behind ``ops.gemm.mm`` and
``mm_grouped``): CPU only, no project kernel.

``gemm`` follows the kernel's formula, not its schedule: operands rounded to bf16 (RNE), the
product formed in ``dtype``, ``* alpha``, ``+ bias``, ReLU (NaN stays NaN), the mask as a select
(``mask > 0`` keeps, anything else -- zero, -0.0, negative, NaN -- gives 0), ``+ beta * c0`` at the
mapped row, rows with a negative map entry dropped, columns ``< ncol`` stored, one rounding to the
output type.  What is not stored keeps ``c0``.

Exact cases.  bf16 x bf16 products are exact in fp32, and with integer operands in [-15, 15] and
``K <= 4096`` every partial sum of every order, split and MFMA shape stays below 2^24, so the
kernel must equal the reference bit for bit (``int_case``; ``tie_case`` adds operands that are
exact bf16 ties, where truncation and RNE differ; ``exact_ok`` checks the condition
arithmetically).  ``mismatch`` names the tile of the first unequal element.

Gaussian cases are judged per element against the scale ``S = |alpha| |A||B| + |bias| +
|beta c0|`` (``elem_err``) by the rule of the other kernel references, ``E_kernel <= 8
max(E_base, 2^-23)`` (``assert_close``), ``E_base`` the fp32 CPU evaluation of the same formula.

``embed`` places a tensor as a view inside a larger buffer (a leading dimension above the extent,
base and leading dimension on or off the kernels' 16-byte contract) and returns a check that the
surround is bit-unchanged.  ``route`` mirrors the dispatch of ``run_group`` / ``launch``: the case
lists below state the kernel each launch is meant to reach, and both test files hold the lists to
``route``.
"""
import collections
import math

import torch

U23 = 2.0 ** -23
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DT = {"bf16": BF, "fp32": F32}
OLD_BOUND = {F32: 2e-3, BF: 1e-2}    # rel() of tests/test_kernels_gpu.py, whole matrix
SENTINEL = -776.0                    # a bf16 value no exact case produces in an unstored place
PAD = 8
LAYOUTS = ((False, True), (False, False), (True, False), (True, True))   # (trans_a, trans_b)


def bf(t):
    """RNE to bf16, in the tensor's own type."""
    return t.to(BF).to(t.dtype)


def trunc_bf(t):
    """Truncation to bf16 (a wrong ``to_bf``), in the tensor's own type."""
    x = t.to(F32).contiguous()
    return (x.view(torch.int32) & -65536).view(F32).to(t.dtype)


def _t(x, dtype):
    return x.detach().to("cpu", dtype)


# ---------------------------------------------------------------------------------------------
# the operation

def gemm(a, b, *, trans_a=False, trans_b=False, alpha=1.0, beta=0.0, bias=None, relu=False,
         mask=None, row_map=None, ncol=None, c0=None, out_dtype=F32, dtype=F64, to_bf=bf):
    """The whole output buffer (``c0``'s shape; ``[M, N]`` or ``[max(row_map) + 1, N]`` zeros
    without one) after ``mm(a, b, ...)``.  ``out_dtype=None`` leaves the result in ``dtype``."""
    A = _t(a.t() if trans_a else a, dtype)
    B = _t(b.t() if trans_b else b, dtype)
    M, N = A.shape[0], B.shape[1]
    v = alpha * (to_bf(A) @ to_bf(B))
    if bias is not None:
        v = v + _t(bias, dtype)
    if relu:
        v = torch.relu(v)
    if mask is not None:
        v = torch.where(_t(mask, dtype) > 0, v, torch.zeros((), dtype=dtype))
    rows = torch.arange(M) if row_map is None else _t(row_map, torch.int64)
    if c0 is None:
        c0 = torch.zeros(int(rows.max()) + 1 if row_map is not None else M, N,
                         dtype=out_dtype or dtype)
    out = _t(c0, dtype).clone()
    keep = rows >= 0
    nc = N if not ncol else min(N, int(ncol))
    r = rows[keep]
    new = v[keep][:, :nc]
    if beta != 0:
        new = new + beta * out[r][:, :nc]
    out[r, :nc] = new
    return out if out_dtype is None else out.to(out_dtype)


def colsum(a, *, trans_a=False, alpha=1.0, beta=0.0, row_map=None, x0=None, dtype=F64,
           out_dtype=F32):
    """``op(a) @ 1`` as a vector: ``x[row_map[m]] = alpha * sum_k op(a)[m, k] + beta * x0[...]``
    (the ``colsum`` request of ``mm_grouped``: a bias gradient beside its weight gradient)."""
    K = a.shape[0] if trans_a else a.shape[1]
    c0 = None if x0 is None else x0.reshape(-1, 1)
    return gemm(a, torch.ones(K, 1), trans_a=trans_a, alpha=alpha, beta=beta, row_map=row_map,
                c0=c0, dtype=dtype, out_dtype=out_dtype).reshape(-1)


def grouped(problems, *, trans_a=False, trans_b=False, dtype=F64):
    """``mm_grouped`` per problem: a list of dicts ``out`` (and ``out2``, ``x1``, ``x2`` where the
    problem has them), each the whole buffer afterwards."""
    res = []
    for q in problems:
        kw = dict(trans_a=trans_a, alpha=q.get("alpha", 1.0), beta=q.get("beta", 0.0),
                  row_map=q.get("row_map"), dtype=dtype)
        r = {}
        for k in ("out", "out2"):
            if q.get(k) is not None:
                r[k] = gemm(q["a"], q["b"], trans_b=trans_b, bias=q.get("bias"),
                            ncol=q.get("ncol"), c0=q[k], out_dtype=q[k].dtype, **kw)
        for k, x in zip(("x1", "x2"), q.get("colsum") or ()):
            r[k] = colsum(q["a"], x0=x, **kw)
        res.append(r)
    return res


# ---------------------------------------------------------------------------------------------
# views inside guarded buffers

def embed(t, pad=PAD, fill=SENTINEL, offset=0, device="cpu"):
    """``(view, check)``: ``t`` (2-D, or 1-D as one row) as a view inside a buffer filled with
    ``fill``, ``pad`` rows above and below and ``pad`` elements left and right.  ``offset`` is
    ``(base, ld)`` (an int stands for both): 0 keeps the base and the leading dimension multiples
    of 8 elements (the LDS-DMA / 16-byte vector contract), 1 puts that one off by one element.
    ``check(what)`` asserts that every element outside the view still has its first bits."""
    ob, ol = (offset, offset) if isinstance(offset, int) else offset
    one_d = t.dim() == 1
    t2 = t.reshape(1, -1) if one_d else t
    rows, cols = t2.shape
    ld = (cols + 2 * pad + 7) // 8 * 8 + ol
    base = pad * ld + pad + ob
    n = (rows + 2 * pad) * ld + 8
    flat = torch.full((n,), fill, dtype=t.dtype)
    inside = torch.zeros(n, dtype=torch.bool)
    idx = base + torch.arange(rows)[:, None] * ld + torch.arange(cols)[None, :]
    inside[idx.reshape(-1)] = True
    flat[idx.reshape(-1)] = t2.reshape(-1)
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    snap = flat.view(ints)[~inside].clone()
    flat = flat.to(device)
    view = flat.as_strided((rows, cols), (ld, 1), base)

    def check(what=""):
        now = flat.detach().cpu().view(ints)[~inside]
        bad = torch.nonzero(now != snap).flatten()
        assert bad.numel() == 0, (f"{what}: {bad.numel()} elements outside the view were "
                                  f"written, first at flat index "
                                  f"{int(torch.nonzero(~inside).flatten()[bad[0]])} (view base "
                                  f"{base}, ld {ld}, {rows} x {cols})")
    return (view[0] if one_d else view), check


# ---------------------------------------------------------------------------------------------
# metrics

Mismatch = collections.namedtuple("Mismatch", "count first tile")


def mismatch(got, ref, tile=64):
    """Unequal elements of ``got`` against ``ref`` (values; the NaN pattern compared as a mask):
    their count, the first ``(row, col)`` and its ``(tile row, tile col)``."""
    g, r = _t(got, F64), _t(ref, F64)
    if g.shape != r.shape:
        raise ValueError(f"shape {tuple(g.shape)} against {tuple(r.shape)}")
    gn, rn = torch.isnan(g), torch.isnan(r)
    bad = torch.nonzero(~(((g == r) & ~gn & ~rn) | (gn & rn)))
    if bad.numel() == 0:
        return Mismatch(0, None, None)
    i, j = int(bad[0, 0]), int(bad[0, 1])
    return Mismatch(bad.shape[0], (i, j), (i // tile, j // tile))


def assert_exact(got, ref, tile=64, what=""):
    m = mismatch(got, ref, tile)
    if m.count:
        i, j = m.first
        raise AssertionError(
            f"{what}: {m.count} of {ref.numel()} elements differ, first at ({i}, {j}) = tile "
            f"{m.tile} of {tile} x {tile}: got {float(got[i, j])}, expected {float(ref[i, j])}")


def whole_err(got, ref):
    """``rel()`` of tests/test_kernels_gpu.py: what the older bound looks at."""
    g, r = _t(got, F64), _t(ref, F64)
    return float((g - r).norm()) / max(float(r.norm()), 1e-12)


def elem_err(got, ref64, S):
    """``max_ij |got - ref| / S_ij`` (``nan`` for a non-finite ``got``)."""
    g = _t(got, F64)
    if not bool(torch.isfinite(g).all()):
        return math.nan
    return float(((g - _t(ref64, F64)).abs() / S).max())


def within_rule(e_k, e_b):
    return math.isfinite(e_k) and e_k <= 8 * max(e_b, U23)


def assert_close(got, ref64, base, S, what=""):
    """``E_kernel <= 8 max(E_base, 2^-23)``; returns both errors."""
    e_k, e_b = elem_err(got, ref64, S), elem_err(base, ref64, S)
    assert not math.isnan(e_k), f"{what}: non-finite kernel output"
    assert within_rule(e_k, e_b), f"{what}: E_kernel {e_k:.3e} > 8 max(E_base {e_b:.3e}, 2^-23)"
    return e_k, e_b


# ---------------------------------------------------------------------------------------------
# cases

OPTS = ("alpha", "bias", "relu", "mask", "beta", "rmap")


def spec(name, M, N, K, lay=0, kind="int", adt="bf16", bdt="bf16", out="fp32", tile=0, splits=1,
         dma=True, aoff=0, boff=0, coff=0, moff=0, opts=(), ncol=0, path=None, fp32_op="a"):
    """One launch: shape, layout ``LAYOUTS[lay]``, operand / output types, ``tile`` and ``splits``
    as passed to ``mm``, the LDS-DMA switch, ``embed`` offsets of A, B, C and the mask, epilogue
    options (of ``OPTS``), ``ncol``, and ``path``: what ``route`` must say."""
    assert set(opts) <= set(OPTS), opts
    return dict(name=name, M=M, N=N, K=K, lay=lay, kind=kind, adt=adt, bdt=bdt, out=out,
                tile=tile, splits=splits, dma=dma, aoff=aoff, boff=boff, coff=coff, moff=moff,
                opts=tuple(opts), ncol=ncol, path=path, fp32_op=fp32_op)


def _gen(s):
    g = torch.Generator()
    g.manual_seed((s["M"] * 1000003 + s["N"] * 10007 + s["K"] * 101 + s["lay"] * 7
                   + len(s["kind"])) % (2 ** 31))
    return g


def _ties(shape, g):
    """+-odd integers in 257 .. 511: every entry an exact tie between two bf16 neighbours."""
    return ((2 * torch.randint(128, 256, shape, generator=g) + 1)
            * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float()


def make_case(s):
    """The CPU tensors of a spec: ``a`` / ``b`` as ``mm`` takes them (stored layout, operand
    type), the keyword arguments of ``gemm`` (``kw``) and the output buffer's first content
    ``c0`` (integers under ``beta``, else the sentinel)."""
    M, N, K = s["M"], s["N"], s["K"]
    ta, tb = LAYOUTS[s["lay"]]
    g = _gen(s)
    if s["kind"] == "int":
        A = torch.randint(-15, 16, (M, K), generator=g).float()
        B = torch.randint(-15, 16, (K, N), generator=g).float()
    elif s["kind"] == "tie":
        if s["fp32_op"] == "a":
            A, B = _ties((M, K), g), torch.randint(-3, 4, (K, N), generator=g).float()
        else:
            A, B = torch.randint(-3, 4, (M, K), generator=g).float(), _ties((K, N), g)
    elif s["kind"] == "gauss":
        A = torch.randn(M, K, generator=g)
        B = torch.randn(K, N, generator=g)
    else:
        raise ValueError(s["kind"])
    a = (A.t() if ta else A).contiguous().to(DT[s["adt"]])
    b = (B.t() if tb else B).contiguous().to(DT[s["bdt"]])
    o = s["opts"]
    odt = DT[s["out"]]
    kw = dict(trans_a=ta, trans_b=tb, out_dtype=odt)
    if "alpha" in o:
        kw["alpha"] = 0.5
    if "bias" in o:
        kw["bias"] = (torch.randint(-8, 9, (N,), generator=g).float() / 4 if s["kind"] != "gauss"
                      else torch.randn(N, generator=g))
    if "relu" in o:
        kw["relu"] = True
    if "mask" in o:
        m = torch.randint(-2, 3, (M, N), generator=g).float()
        m[::3, ::2] = -0.0
        kw["mask"] = m.to(BF)
    Mo = M
    if "rmap" in o:
        Mo = M + 5
        rm = torch.randperm(Mo, generator=g)[:M].to(torch.int32)
        if M > 3:
            rm[torch.tensor([1, M // 2, M - 1])] = -1
        kw["row_map"] = rm
    if s["ncol"]:
        kw["ncol"] = s["ncol"]
    if "beta" in o:
        kw["beta"] = 1.0
        c0 = (torch.randint(-15, 16, (Mo, N), generator=g).float() if s["kind"] != "gauss"
              else torch.randn(Mo, N, generator=g))
    else:
        c0 = torch.full((Mo, N), SENTINEL)
    return dict(spec=s, a=a, b=b, kw=kw, c0=c0.to(odt))


def int_case(M, N, K, **kw):
    """Integers in [-15, 15]: exact in every order of summation up to K = 4096."""
    return make_case(spec(f"int-{M}x{N}x{K}", M, N, K, kind="int", **kw))


def tie_case(M, N, K, fp32_op="a", **kw):
    """One fp32 operand of +-odd integers in 257 .. 511 (exact bf16 ties), the other in [-3, 3]:
    RNE and truncation give different products; sums stay below 2^24 for K <= 1024."""
    kw.setdefault("adt" if fp32_op == "a" else "bdt", "fp32")
    return make_case(spec(f"tie-{M}x{N}x{K}", M, N, K, kind="tie", fp32_op=fp32_op, **kw))


def gauss_case(M, N, K, **kw):
    """N(0, 1) fp32 operands, not pre-rounded."""
    kw.setdefault("adt", "fp32")
    kw.setdefault("bdt", "fp32")
    return make_case(spec(f"gauss-{M}x{N}x{K}", M, N, K, kind="gauss", **kw))


def reference(case, dtype=F64, out_dtype="spec", **over):
    kw = dict(case["kw"])
    if out_dtype != "spec":
        kw["out_dtype"] = out_dtype
    kw.update(over)
    return gemm(case["a"], case["b"], c0=case["c0"], dtype=dtype, **kw)


def scale(case):
    """``S = |alpha| |A||B| + |bias| + |beta c0|`` in fp64 at every place of the output buffer
    that is stored (1 elsewhere: those places must equal ``c0``, whose error is 0)."""
    kw = dict(case["kw"])
    a, b = bf(_t(case["a"], F64)).abs(), bf(_t(case["b"], F64)).abs()
    bias = kw.get("bias")
    stored = gemm(a, b, trans_a=kw["trans_a"], trans_b=kw["trans_b"],
                  alpha=abs(kw.get("alpha", 1.0)), bias=None if bias is None else bias.abs(),
                  beta=abs(kw.get("beta", 0.0)), row_map=kw.get("row_map"), ncol=kw.get("ncol"),
                  c0=_t(case["c0"], F64).abs() if kw.get("beta") else
                  torch.full(case["c0"].shape, -1.0, dtype=F64), out_dtype=None)
    return torch.where(stored < 0, torch.ones((), dtype=F64), stored)


def exact_ok(case):
    """The exactness condition of an ``int`` / ``tie`` case: every stored magnitude bound
    ``|alpha| |A||B| + |bias| + |beta c0|`` is below 2^24, and the fp32 evaluation of the formula
    equals the fp64 one bit for bit."""
    if case["spec"]["kind"] == "gauss":
        return False
    kw = case["kw"]
    c = dict(case, kw={k: v for k, v in kw.items() if k not in ("relu", "mask")})
    if float(scale(c).max()) >= 2.0 ** 24:
        return False
    r64 = reference(case, F64, None)
    r32 = reference(case, F32, None)
    return mismatch(r32, r64).count == 0 and mismatch(reference(case), r64).count == (
        0 if case["spec"]["out"] == "fp32" else mismatch(r64.to(BF), r64).count)


# ---------------------------------------------------------------------------------------------
# the dispatch, mirrored (csrc/kernels/gemm.hip run_group / launch, ops.gemm._layout)

def _lay(t, rows_first):
    s0, s1 = t.stride()
    al = (t.storage_offset() * t.element_size()) % 16 == 0
    if t.shape[1] == 1 or s1 == 1:
        return 0, (s0 if t.shape[0] > 1 else max(t.shape[1], 1)), al
    if t.shape[0] == 1 or s0 == 1:
        return 1, (s1 if t.shape[1] > 1 else max(t.shape[0], 1)), al
    raise ValueError("not contiguous along one axis")


def eff_splits(K, splits):
    """The split count ``dn_gemm`` ends up with: slices are whole 64-deep K tiles."""
    if splits <= 1:
        return 1
    kchunk = (-(-K // splits) + 63) // 64 * 64
    return -(-K // kchunk)


def route(s, a, b, out, mask=None, inlaunch=False):
    """``"<kernel>/<epilogue>"`` of one ``mm`` launch on tensors placed as given (views of
    16-byte aligned allocations).  Kernels: ``gen64``, ``gen128`` (``gemm_kernel``, branchy
    staging), ``vec64``, ``vec128`` (``gemm_kernel``, 16-byte staging), ``dma64r4``, ``dma64r2``,
    ``dma128`` (``gemm_dma_kernel``; ring depth), ``g256``.  Epilogues: ``scalar``
    (``epi_store``), ``vepi`` (LDS-staged 16-byte rows), ``inlaunch`` (split-K combined by the
    last workgroup), ``reduce4`` / ``reduce1`` (``gemm_splitk_reduce``, vector / scalar)."""
    ta_, tb_ = LAYOUTS[s["lay"]]
    A = a.t() if ta_ else a
    B = b.t() if tb_ else b
    M, N, K = s["M"], s["N"], s["K"]
    ta, lda, a_al = _lay(A, True)
    tb, ldb, b_al = _lay(B, False)

    def vec_ok(al, kcontig, rows, ld):
        return al and ld % 8 == 0 and (K % 8 == 0 if kcontig else rows % 8 == 0)
    vec = vec_ok(a_al, not ta, M, lda) and vec_ok(b_al, bool(tb), N, ldb)
    both = A.dtype == BF and B.dtype == BF
    obf = out.dtype == BF
    cv = 8 if obf else 4
    ldc = out.stride(0)
    c_al = (out.storage_offset() * out.element_size()) % 16 == 0
    # (a spec with ncol goes through mm_grouped, which keeps the split count it was given: the
    # slices past K are empty)
    sp = max(1, s["splits"]) if s["ncol"] else eff_splits(K, s["splits"])
    rmap = "rmap" in s["opts"]
    vepi = not (sp > 1 or rmap or s["ncol"] > 0 or N % cv or ldc % cv or not c_al)
    if mask is not None and (mask.stride(0) % 8 or (mask.storage_offset() * 2) % 16):
        vepi = False
    tile = s["tile"]
    if tile == 2 and vec and s["dma"] and both and ((sp > 1 and N % 4 == 0) or (sp == 1 and vepi)):
        kern, bm = "g256", 256
    else:
        bm = 128 if tile in (1, 2) else 64
        if both and vec and s["dma"]:
            wgs = -(-M // bm) * -(-N // bm) * sp
            kern = "dma128" if bm == 128 else ("dma64r4" if wgs < 512 else "dma64r2")
        else:
            kern = ("vec" if vec else "gen") + str(bm)
    if sp > 1:
        if inlaunch and bm == 64:
            epi = "inlaunch"
        else:
            epi = "reduce4" if (s["ncol"] <= 0 and N % 4 == 0 and ldc % 4 == 0 and c_al) else "reduce1"
    else:
        epi = "vepi" if (vepi and kern.startswith(("dma", "g256"))) else "scalar"
    return f"{kern}/{epi}"


def place(case, device="cpu", fill_ops=math.nan):
    """The tensors of a case embedded as its spec says: operands in ``fill_ops`` (NaN: nothing
    outside the logical operand may reach a stored output), the output and the mask in the
    sentinel.  ``(a, b, out, kwargs of mm, checks)``."""
    s, kw = case["spec"], case["kw"]
    a, ca = embed(case["a"], fill=fill_ops, offset=s["aoff"], device=device)
    b, cb = embed(case["b"], fill=fill_ops, offset=s["boff"], device=device)
    out, cc = embed(case["c0"], offset=s["coff"], device=device)
    checks = [("A", ca), ("B", cb), ("C", cc)]
    mk = dict(trans_a=kw["trans_a"], trans_b=kw["trans_b"], out=out, alpha=kw.get("alpha", 1.0),
              beta=kw.get("beta", 0.0), relu=kw.get("relu", False), tile=s["tile"],
              splits=s["splits"])
    if "bias" in kw:
        mk["bias"] = kw["bias"].to(device)
    if "mask" in kw:
        mk["mask"], cm = embed(kw["mask"], fill=math.nan, offset=s["moff"], device=device)
        checks.append(("mask", cm))
    if "row_map" in kw:
        mk["row_map"] = kw["row_map"].to(device)
    return a, b, out, mk, checks


# shape edges by tile T (tests/test_gemm_exact_gpu.py): M and N of {1, T-1, T, T+1, T+8, 2T+8},
# {8, T-8, T, T+8, 2T+8} where the 16-byte contract needs % 8; K of KS (1 .. 6 K tiles of 64
# against ring depths 2 and 4, a ragged last tile, a short last chunk)
KS = (1, 7, 8, 9, 56, 63, 64, 65, 72, 128, 136, 200, 264, 328)
KS8 = tuple(k for k in KS if k % 8 == 0)


def mn_any(T):
    return (1, T - 1, T, T + 1, T + 8, 2 * T + 8)


def mn8(T):
    return (8, T - 8, T, T + 8, 2 * T + 8)


def _sweep(prefix, T, ks, ms, ns, n=None, lay0=0, **kw):
    """One spec per K of ``ks`` (the first ``n``), M and N walking their sets at different
    strides and the layout rotating, so that every value and every layout occurs."""
    out = []
    for i, K in enumerate(ks[:n] if n else ks):
        M, N = ms[i % len(ms)], ns[(2 * i + 1) % len(ns)]
        lay = (i + lay0) % 4
        out.append(spec(f"{prefix}-{M}x{N}x{K}-l{lay}", M, N, K, lay=lay, **kw))
    return out


def _ragged_k(ks):
    return tuple(k for k in ks if k % 8)


DTYPES = (("fp32", "fp32"), ("bf16", "bf16"), ("fp32", "bf16"), ("bf16", "fp32"))


def _paths():
    L = []
    odd64, odd128 = (1, 63, 65, 129), (1, 127, 129, 257)
    for adt, bdt in DTYPES:
        d = f"{adt[0]}{bdt[0]}"
        # gemm_kernel<VEC=false>: off the contract by shape (odd M, N and K), by base, by ld
        L += _sweep(f"gen64-shape-{d}", 64, _ragged_k(KS) + (129, 201), odd64, odd64, adt=adt,
                    bdt=bdt, path="gen64/scalar")
        L += _sweep(f"gen64-base-{d}", 64, KS8, mn8(64), mn8(64), n=4, adt=adt, bdt=bdt,
                    aoff=(1, 0), path="gen64/scalar")
        L += _sweep(f"gen64-ld-{d}", 64, KS8, mn8(64), mn8(64), n=4, lay0=1, adt=adt, bdt=bdt,
                    boff=(0, 1), path="gen64/scalar")
        L += _sweep(f"gen128-shape-{d}", 128, (9, 65, 201, 329), odd128, odd128, adt=adt, bdt=bdt,
                    tile=1, path="gen128/scalar")
        # gemm_kernel<VEC=true>: fp32 and mixed operands; bf16 with the LDS-DMA kernel off
        dma = not (adt == "bf16" and bdt == "bf16")
        L += _sweep(f"vec64-{d}", 64, KS8, mn8(64), mn8(64), adt=adt, bdt=bdt, dma=dma,
                    path="vec64/scalar")
        L += _sweep(f"vec128-{d}", 128, KS8, mn8(128), mn8(128), n=5, adt=adt, bdt=bdt, dma=dma,
                    tile=1, path="vec128/scalar")
    # k-major on both sides (trans_a, not trans_b): K is free of the % 8 contract (K = 1 is
    # not: a one-column operand counts as k-contiguous in ops.gemm._layout)
    L += [spec(f"vec64-km-{K}", 72, 56, K, lay=2, adt="fp32", bdt="fp32", path="vec64/scalar")
          for K in _ragged_k(KS)[1:]]
    L += [spec(f"dma64-km-{K}", 136, 72, K, lay=2, path="dma64r4/vepi")
          for K in _ragged_k(KS)[1:]]
    # gemm_dma_kernel<64>: 4-stage ring (1 .. 6 K tiles: fewer than, as many as, more than stages)
    L += _sweep("dma64r4", 64, KS8 + (392,), mn8(64), mn8(64), path="dma64r4/vepi")
    L += _sweep("dma64r4-bf", 64, KS8, mn8(64), mn8(64), n=5, lay0=2, out="bf16",
                path="dma64r4/vepi")
    # ... 2-stage ring from 512 workgroups: 64 tiles x 10 slices of 64 (splits=8 gives chunks of
    # 128 and 5 slices = 320 workgroups, which is still the 4-stage ring)
    for lay in range(4):
        L.append(spec(f"dma64r2-l{lay}", 512, 512, 584, lay=lay, splits=10,
                      path="dma64r2/reduce4"))
    L.append(spec("dma64r4-split8", 512, 512, 584, splits=8, path="dma64r4/reduce4"))
    L += _sweep("dma128", 128, KS8, mn8(128), mn8(128), tile=1, path="dma128/vepi")
    # gemm256_kernel
    for i, (M, N) in enumerate(((264, 264), (8, 256), (520, 264))):
        for lay in range(4):
            K = (72, 200, 584, 328)[(i + lay) % 4]
            L.append(spec(f"g256-{M}x{N}x{K}-l{lay}", M, N, K, lay=lay, tile=2,
                          out=("fp32", "bf16")[(i + lay) % 2], path="g256/vepi"))
    # tile 2 without a vector epilogue falls back to 128 x 128
    L.append(spec("g256-fallback-n", 264, 260, 200, tile=2, out="bf16", path="dma128/scalar"))
    L.append(spec("g256-fallback-c", 264, 264, 200, tile=2, coff=(1, 0), path="dma128/scalar"))
    L.append(spec("g256-fallback-rmap", 264, 264, 72, tile=2, opts=("rmap",), path="dma128/scalar"))
    L.append(spec("g256-fallback-fp32", 264, 264, 72, tile=2, adt="fp32", path="vec128/scalar"))
    return L


ALL5 = ("alpha", "bias", "relu", "mask", "beta")


def _epilogues():
    L = []
    single = [(o,) for o in ALL5] + [ALL5]
    for out in ("fp32", "bf16"):
        o = out[0]
        for opts in single:
            tag = "+".join(opts) if len(opts) < 5 else "all"
            # LDS-staged vector epilogues of each tile size, and the scalar one beside them
            L.append(spec(f"epi-dma64-{o}-{tag}", 72, 136, 72, out=out, opts=opts,
                          path="dma64r4/vepi"))
            L.append(spec(f"epi-dma128-{o}-{tag}", 136, 264, 72, lay=1, out=out, opts=opts, tile=1,
                          path="dma128/vepi"))
            L.append(spec(f"epi-g256-{o}-{tag}", 264, 264, 72, lay=2, out=out, opts=opts, tile=2,
                          path="g256/vepi"))
            L.append(spec(f"epi-gen64-{o}-{tag}", 65, 129, 65, out=out, opts=opts,
                          path="gen64/scalar"))
        scal = [("rmap",), ALL5 + ("rmap",)]
        for opts in scal:
            tag = "rmap" if len(opts) == 1 else "all+rmap"
            L.append(spec(f"epi-dma64-{o}-{tag}", 72, 136, 72, out=out, opts=opts,
                          path="dma64r4/scalar"))
            L.append(spec(f"epi-dma128-{o}-{tag}", 136, 264, 72, lay=1, out=out, opts=opts, tile=1,
                          path="dma128/scalar"))
            L.append(spec(f"epi-gen128-{o}-{tag}", 129, 65, 65, lay=3, out=out, opts=opts, tile=1,
                          path="gen128/scalar"))
        # every condition under which run_group drops the vector epilogue, all options on
        cvn = 68 if out == "bf16" else 65       # N % 8 (bf16) / N % 4 (fp32); K-contiguous B
        for tag, kw in (("n", dict(N=cvn)), ("ldc", dict(coff=(0, 1))), ("cbase", dict(coff=(1, 0))),
                        ("ldm", dict(moff=(0, 1))), ("mbase", dict(moff=(1, 0)))):
            N = kw.pop("N", 136)
            L.append(spec(f"epi-dma64-{o}-drop-{tag}", 72, N, 72, out=out, opts=ALL5,
                          path="dma64r4/scalar", **kw))
            L.append(spec(f"epi-dma128-{o}-drop-{tag}", 136, N, 136, out=out, opts=ALL5, tile=1,
                          path="dma128/scalar", **kw))
        # ncol (mm_grouped only, so without ReLU and mask): alone and beside the others
        for nc in (1, 5):
            for tag, opts in (("", ()), ("-all", ("alpha", "bias", "beta", "rmap"))):
                L.append(spec(f"epi-dma64-{o}-ncol{nc}{tag}", 72, 136, 72, out=out, opts=opts,
                              ncol=nc, path="dma64r4/scalar"))
                L.append(spec(f"epi-gen128-{o}-ncol{nc}{tag}", 129, 65, 65, lay=1, out=out,
                              adt="fp32", opts=opts, ncol=nc, tile=1, path="gen128/scalar"))
    # the same fp32 N = 68 keeps the vector epilogue (4-column vectors)
    L.append(spec("epi-dma64-f-n68", 72, 68, 72, opts=ALL5, path="dma64r4/vepi"))
    return L


def _splitk():
    L = []
    i = 0
    for K in (200, 520, 584):
        for sp in (2, 3, 8, 11):
            lay = i % 4
            i += 1
            # tiles 0, 1, 2 on the LDS-DMA kernels; the vector reduce
            L.append(spec(f"split-dma64-{K}-{sp}", 72, 136, K, lay=lay, splits=sp,
                          path="dma64r4/reduce4"))
            L.append(spec(f"split-dma128-{K}-{sp}", 136, 72, K, lay=lay, splits=sp, tile=1,
                          path="dma128/reduce4"))
            L.append(spec(f"split-g256-{K}-{sp}", 264, 264, K, lay=lay, splits=sp, tile=2,
                          path="g256/reduce4"))
            # register-staged kernels, ragged shapes; the scalar reduce (N % 4)
            L.append(spec(f"split-gen64-{K}-{sp}", 65, 63, K + 1, lay=lay, splits=sp, adt="fp32",
                          path="gen64/reduce1"))
    full = ("alpha", "bias", "beta", "rmap")
    for tile, kern in ((0, "dma64r4"), (1, "dma128")):
        t = f"t{tile}"
        L.append(spec(f"split-{t}-opts", 136, 136, 584, lay=2, splits=3, tile=tile, opts=full,
                      path=f"{kern}/reduce4"))
        L.append(spec(f"split-{t}-opts-bf", 136, 136, 584, lay=2, splits=3, tile=tile, opts=full,
                      out="bf16", path=f"{kern}/reduce4"))
        L.append(spec(f"split-{t}-relu-mask", 136, 136, 520, splits=8, tile=tile,
                      opts=("relu", "mask", "bias"), path=f"{kern}/reduce4"))
        # the scalar reduce: ldc % 4, C off 16 bytes, ncol
        L.append(spec(f"split-{t}-ldc", 136, 136, 520, splits=3, tile=tile, opts=full,
                      coff=(0, 1), path=f"{kern}/reduce1"))
        L.append(spec(f"split-{t}-cbase", 136, 136, 200, splits=2, tile=tile, opts=full,
                      coff=(1, 0), out="bf16", path=f"{kern}/reduce1"))
        L.append(spec(f"split-{t}-ncol", 136, 136, 200, splits=3, tile=tile, opts=("beta",),
                      ncol=5, path=f"{kern}/reduce1"))
    L.append(spec("split-g256-opts", 264, 264, 584, lay=2, splits=3, tile=2, opts=full,
                  path="g256/reduce4"))
    L.append(spec("split-g256-n-mod4", 264, 262, 584, splits=3, tile=2, path="dma128/reduce1"))
    return L


def _inlaunch():
    L = []
    for sp, K in ((2, 200), (3, 520), (8, 584), (11, 584)):     # 2, 3, 5 and 10 slices
        for lay in (0, 2):
            L.append(spec(f"inl-dma64-{K}-{sp}-l{lay}", 72, 136, K, lay=lay, splits=sp,
                          path="dma64r4/inlaunch"))
        L.append(spec(f"inl-gen64-{K}-{sp}", 65, 63, K + 1, lay=1, splits=sp, adt="fp32",
                      opts=("alpha", "bias", "beta", "rmap"), path="gen64/inlaunch"))
        L.append(spec(f"inl-dma64-{K}-{sp}-ncol", 72, 136, K, splits=sp, ncol=5, opts=("beta",),
                      out="bf16", path="dma64r4/inlaunch"))
    return L


def _numerics():
    L = []
    for i, (adt, bdt) in enumerate((("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "fp32"))):
        op = "b" if adt == "bf16" else "a"
        L.append(spec(f"tie-gen64-{i}", 65, 63, 201, lay=i, kind="tie", adt=adt, bdt=bdt,
                      fp32_op=op, path="gen64/scalar"))
        L.append(spec(f"tie-vec64-{i}", 72, 136, 264, lay=i + 1, kind="tie", adt=adt, bdt=bdt,
                      fp32_op=op, path="vec64/scalar"))
        L.append(spec(f"tie-vec128-{i}", 136, 72, 1024, lay=i, kind="tie", adt=adt, bdt=bdt,
                      fp32_op=op, tile=1, splits=3, path="vec128/reduce4"))
    return L


def _gauss():
    L = []
    full = ("alpha", "bias", "beta")
    for i, (M, N, K) in enumerate(((65, 63, 201), (129, 65, 329), (1, 257, 73))):
        L.append(spec(f"gauss-gen-{i}", M, N, K, lay=i, kind="gauss", adt="fp32", bdt="fp32",
                      tile=i % 2, opts=full if i else (), path=f"gen{(64, 128)[i % 2]}/scalar"))
    for i, (M, N, K) in enumerate(((72, 136, 264), (264, 72, 520), (520, 520, 584))):
        L.append(spec(f"gauss-vec-{i}", M, N, K, lay=i + 1, kind="gauss", adt="fp32",
                      bdt=("fp32", "bf16", "fp32")[i], tile=i % 2, opts=full if i else (),
                      path=f"vec{(64, 128)[i % 2]}/scalar"))
        L.append(spec(f"gauss-dma-{i}", M, N, K, lay=i, kind="gauss", tile=i,
                      out=("fp32", "bf16", "fp32")[i], opts=full if i == 1 else (),
                      path=("dma64r4", "dma128", "g256")[i] + "/vepi"))
    L.append(spec("gauss-relu-bf", 520, 520, 584, kind="gauss", out="bf16", opts=("bias", "relu"),
                  path="dma64r4/vepi"))
    L.append(spec("gauss-k4096", 72, 136, 4096, kind="gauss", adt="fp32", bdt="fp32",
                  path="vec64/scalar"))
    L.append(spec("gauss-k4096-split", 72, 136, 4096, kind="gauss", lay=2, splits=8,
                  path="dma64r4/reduce4"))
    return L


PATHS = _paths()
EPILOGUES = _epilogues()
SPLITK = _splitk()
INLAUNCH = _inlaunch()
NUMERICS = _numerics()
GAUSS = _gauss()
EXACT_LISTS = dict(paths=PATHS, epilogues=EPILOGUES, splitk=SPLITK, inlaunch=INLAUNCH,
                   numerics=NUMERICS)


def find(name):
    for L in list(EXACT_LISTS.values()) + [GAUSS]:
        for s in L:
            if s["name"] == name:
                return s
    raise KeyError(name)


# non-finite locality (tests/test_gemm_exact_gpu.py test 3): the four ReLU sites and the plain
# stores beside them.  (name, spec, A row holding the NaN, its k): the last row of an edge tile,
# the last k of a split's slice.
def _nan_sites():
    S = []
    S.append(("scalar", spec("nan-gen64", 65, 63, 65, adt="fp32", bdt="fp32", opts=("relu", "bias"),
                             path="gen64/scalar"), 63, 64))
    S.append(("staged", spec("nan-dma64", 72, 136, 136, opts=("relu", "bias"),
                             path="dma64r4/vepi"), 63, 135))
    S.append(("staged128", spec("nan-dma128", 136, 136, 72, tile=1, out="bf16",
                                opts=("relu", "bias"), path="dma128/vepi"), 127, 71))
    S.append(("g256", spec("nan-g256", 264, 264, 72, tile=2, opts=("relu", "bias"),
                           path="g256/vepi"), 255, 0))
    S.append(("reduce4", spec("nan-reduce4", 72, 136, 200, splits=3, opts=("relu", "bias"),
                              path="dma64r4/reduce4"), 71, 127))
    S.append(("reduce1", spec("nan-reduce1", 65, 63, 201, splits=3, adt="fp32",
                              opts=("relu", "bias"), path="gen64/reduce1"), 64, 63))
    return S


NAN_SITES = _nan_sites()


# ---------------------------------------------------------------------------------------------
# deliberately wrong results (tests/test_gemm_ref.py: each must be caught)

MUTATIONS = ("one_element", "stale_vector", "drop_last_kchunk", "double_k_at_split",
             "truncation", "bias_last8", "beta_per_split", "rowmap_shift", "mask_lt0",
             "store_at_ncol", "relu_nan_to_zero")


def mutated(name, case):
    """``(wrong, right)``: the output buffer a kernel with the named fault would leave, and the
    reference, both in fp64 before the output rounding (round with ``.to``)."""
    s, kw = case["spec"], case["kw"]
    M, N, K = s["M"], s["N"], s["K"]
    ta, tb = kw["trans_a"], kw["trans_b"]
    right = reference(case, F64, None)
    rows = torch.arange(M) if "row_map" not in kw else kw["row_map"].long()
    last = int(rows[rows >= 0][-1])

    def with_ops(A, B, **over):
        c = dict(case, a=A.t() if ta else A, b=B.t() if tb else B)
        return reference(c, F64, None, **over)
    A = _t(case["a"].t() if ta else case["a"], F64)
    B = _t(case["b"].t() if tb else case["b"], F64)
    nst = N if not s["ncol"] else s["ncol"]
    if name == "one_element":
        wrong = right.clone()
        wrong[last, nst - 1] = 0.0 if float(right[last, nst - 1]) != 0 else 1.0
    elif name == "stale_vector":                 # 16 bytes of the output keep what was there
        n = 8 if s["out"] == "bf16" else 4
        wrong = right.clone()
        wrong[last, N - n:] = _t(case["c0"], F64)[last, N - n:]
    elif name == "drop_last_kchunk":             # the corner 64 x 64 tile misses its last 8 k
        r0, c0 = (M - 1) // 64 * 64, (N - 1) // 64 * 64
        part = with_ops(A[:, :K - 8], B[:K - 8])
        wrong = right.clone()
        mrow = rows[r0:]
        mrow = mrow[mrow >= 0]
        wrong[mrow, c0:nst] = part[mrow, c0:nst]
    elif name == "double_k_at_split":            # the first k of the second slice counted twice
        k = (-(-K // max(s["splits"], 2)) + 63) // 64 * 64
        k = min(k, K - 1)
        wrong = with_ops(torch.cat([A, A[:, k:k + 1]], 1), torch.cat([B, B[k:k + 1]], 0))
    elif name == "truncation":
        wrong = reference(case, F64, None, to_bf=trunc_bf)
    elif name == "bias_last8":
        b = kw["bias"].clone()
        b[-8:] = 0
        wrong = reference(case, F64, None, bias=b)
    elif name == "beta_per_split":
        wrong = reference(case, F64, None, beta=kw["beta"] * max(s["splits"], 2))
    elif name == "rowmap_shift":
        wrong = reference(case, F64, None, row_map=torch.roll(kw["row_map"], 1))
    elif name == "mask_lt0":                     # zero only where mask < 0
        m = kw["mask"].float()
        wrong = reference(case, F64, None, mask=torch.where(m == 0, torch.ones_like(m), m))
    elif name == "store_at_ncol":
        wrong = reference(case, F64, None, ncol=s["ncol"] + 1)
    elif name == "relu_nan_to_zero":             # fmaxf(NaN, 0) = 0
        An = A.clone()
        An[M - 1, K - 1] = math.nan
        right = with_ops(An, B)
        wrong = torch.nan_to_num(right, nan=0.0) if "beta" not in kw else None
        assert wrong is not None
    else:
        raise ValueError(name)
    return wrong, right
