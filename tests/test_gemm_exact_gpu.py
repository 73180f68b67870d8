"""``csrc/kernels/gemm.hip`` element by element against the reference of ``tests/gemm_ref.py``.

Exact tests (1-6 and the tie cases of 7): integer operands whose every partial sum is below 2^24
(``gemm_ref.exact_ok``, held on the same case lists by ``tests/test_gemm_ref.py``), so the kernel
must equal the fp64 reference bit for bit whatever its schedule; a failure names the tile of the
first unequal element.  Every operand is a view inside a NaN-filled buffer (no value outside the
logical operand may reach a stored output), every output and mask a view inside a sentinel-filled
one whose surround is compared bit for bit afterwards.  ``gemm_ref.route`` mirrors the dispatch;
each launch asserts it reaches the kernel and epilogue its spec names.

Gaussian tests (7) judge per element against ``S = |alpha| |A||B| + |bias| + |beta c0|`` by
``E_kernel <= 8 max(E_base, 2^-23)``; both errors go to ``$DINUNET_ERR_LOG`` (jsonl) when set.

Measured on one MI355X: every exact case equal bit for bit on every path; the Gaussian cases'
largest ``E_kernel / max(E_base, 2^-23)`` is 1.02 (520 x 520 x 584 on the 256 tile, ``E_kernel``
1.2e-7), with bf16 outputs 1.00 (the output rounding, 7e-4, is all there is).  The one finding:
the ReLU was ``fmaxf(v, 0)`` at its four sites, which turns NaN into 0; with it, each case of
``test_nan_stays_in_its_row_and_column_and_survives_relu`` had no NaN at all in the row of the
NaN operand (first at (63, 0), (127, 0), (255, 0), (71, 0), (64, 0): tile row 0 / 1, the last row
of the edge tile).  The ReLU is now a compare and select that keeps NaN.

Not covered: the 8-stage ring (``DN_GEMM_RING8_MAX``, read once at load, off by default) and
hipBLASLt (``DINUNET_PLAIN_BLAS``).
"""
import json
import math
import os

import pytest
import torch

import gemm_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NAN = math.nan


@pytest.fixture(autouse=True)
def _native():
    from dinunet_implementations_amd.ops import _lib
    assert _lib.native_available(), "kernel library must load on a GPU box"


def _record(kind, case, e_k, e_b):
    path = os.environ.get("DINUNET_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"kind": kind, "case": case, "e_kernel": float(f"{e_k:.4g}"),
                                "e_base": float(f"{e_b:.4g}")}) + "\n")


def _poison(n):
    """Allocate and free ``n`` NaN floats: the caching allocator then most likely hands the same
    block back as the next split-K slab (best effort, not guaranteed, not a condition)."""
    t = torch.full((n,), NAN, dtype=F32, device=DEV)
    del t


def _launch(case, inlaunch=False):
    """One spec on the GPU as ``gemm_ref.place`` lays it out; the output buffer on the CPU."""
    from dinunet_implementations_amd.ops import _lib
    from dinunet_implementations_amd.ops import gemm as G
    s = case["spec"]
    a, b, out, mk, checks = ref.place(case, DEV)
    got = ref.route(s, a, b, out, mk.get("mask"), inlaunch=inlaunch)
    assert got == s["path"], f"{s['name']}: routed to {got}, meant for {s['path']}"
    if s["splits"] > 1:
        _poison(s["splits"] * s["M"] * s["N"])
    if not s["dma"]:
        _lib.call("dn_gemm_set_dma", 0)
    try:
        if s["ncol"]:
            q = dict(a=a, b=b, out=out, alpha=mk["alpha"], beta=mk["beta"], ncol=s["ncol"])
            for k in ("bias", "row_map"):
                if k in mk:
                    q[k] = mk[k]
            G.mm_grouped([q], trans_a=mk["trans_a"], trans_b=mk["trans_b"], splits=s["splits"],
                         tile=s["tile"])
        else:
            assert G.mm(a, b, **mk) is out
    finally:
        if not s["dma"]:
            _lib.call("dn_gemm_set_dma", 1)
    torch.cuda.synchronize()
    for what, chk in checks:
        chk(f"{s['name']}: surround of {what}")
    return out.cpu()


def _tile_of(s):
    return {"gen64": 64, "vec64": 64, "dma64r4": 64, "dma64r2": 64, "gen128": 128, "vec128": 128,
            "dma128": 128, "g256": 256}[s["path"].split("/")[0]]


def _exact(specs, inlaunch=False):
    for s in specs:
        case = ref.make_case(s)
        got = _launch(case, inlaunch)
        ref.assert_exact(got, ref.reference(case), _tile_of(s), f"{s['name']} [{s['path']}]")


def _by_kernel(specs):
    groups = {}
    for s in specs:
        groups.setdefault(s["path"].split("/")[0], []).append(s)
    return groups


# ---------------------------------------------------------------------------------------------
# 1. every dispatch path, four layouts

@pytest.mark.parametrize("kernel", sorted(_by_kernel(ref.PATHS)))
def test_every_dispatch_path_is_exact(kernel):
    """``gemm_kernel`` with branchy staging (``gen``: fp32, bf16 and both mixed operand types, off
    the 16-byte contract by shape, by base and by leading dimension) and with vector staging
    (``vec``: fp32 and mixed, bf16 with the LDS-DMA kernel switched off), ``gemm_dma_kernel<64>`` on
    the 4-stage ring and, from 512 workgroups, the 2-stage ring, ``gemm_dma_kernel<128>``,
    ``gemm256_kernel``, and tile 2 falling back to 128 x 128 without a vector epilogue."""
    _exact(_by_kernel(ref.PATHS)[kernel])


# ---------------------------------------------------------------------------------------------
# 2. epilogues

@pytest.mark.parametrize("kernel", sorted(_by_kernel(ref.EPILOGUES)))
def test_epilogue_options_are_exact(kernel):
    """alpha 0.5, quarter-integer bias, ReLU, mask (with 0 and -0.0), beta 1 on integers, a row
    map into a taller output with dropped rows, ncol 1 and 5: each alone and all together, on the
    scalar epilogue and the LDS-staged vector one of each tile size, fp32 and bf16 out, and with
    each condition that makes ``run_group`` drop the vector epilogue.  One reference for all: the
    result does not depend on the epilogue that ran."""
    _exact(_by_kernel(ref.EPILOGUES)[kernel])


# ---------------------------------------------------------------------------------------------
# 3. non-finite values

def _with_nan(case, where, i, k):
    """The case with one NaN: ``where`` "a" -> A[i, k], "b" -> B[k, i] (layout 0: a is [M, K], b is
    [N, K])."""
    c = dict(case)
    t = case[where].clone()
    t[i, k] = NAN
    c[where] = t
    return c


@pytest.mark.parametrize("site", [n for n, _, _, _ in ref.NAN_SITES])
def test_nan_stays_in_its_row_and_column_and_survives_relu(site):
    """One NaN in A's row i (the last row of an edge tile, the last k of a split's slice) makes
    exactly output row i NaN, one in a B column exactly that column, through ``relu=True``
    (``torch.relu`` keeps NaN; the gradient norm, the fused Adam's ``skipped`` and DP's
    ``nonfinite`` count on it), at the four places the ReLU is written: ``epi_store``, the
    LDS-DMA kernel's staged epilogue, the 256-tile epilogue and ``epi_store4`` of the reduce."""
    _, s, i, k = next(x for x in ref.NAN_SITES if x[0] == site)
    assert s["lay"] == 0
    base = ref.make_case(s)
    M, N = s["M"], s["N"]
    for where, idx in (("a", i), ("b", N - 1 if site != "g256" else 255)):
        case = _with_nan(base, where, idx, k)
        got = _launch(case)
        want = ref.reference(case)
        nan = torch.isnan(got.float())
        expect = torch.zeros(M, N, dtype=torch.bool)
        if where == "a":
            expect[idx] = True
        else:
            expect[:, idx] = True
        assert torch.equal(torch.isnan(want.float()), expect)
        bad = torch.nonzero(nan != expect)
        assert bad.numel() == 0, (f"{s['name']} [{s['path']}], NaN in {where}: {bad.shape[0]} "
                                  f"elements have the wrong NaN state, first at "
                                  f"{tuple(bad[0].tolist())} (NaN there: {bool(nan[tuple(bad[0])])})")
        ref.assert_exact(got, want, _tile_of(s), f"{s['name']} NaN in {where}")


@pytest.mark.parametrize("site", [n for n, _, _, _ in ref.NAN_SITES])
def test_nan_under_a_closed_mask_is_zero(site):
    """The mask is a select: where ``mask <= 0`` a NaN (or Inf) product gives 0."""
    _, s, i, k = next(x for x in ref.NAN_SITES if x[0] == site)
    s = dict(s, opts=s["opts"] + ("mask",), name=s["name"] + "-mask")
    case = _with_nan(ref.make_case(s), "a", i, k)
    t = case["a"].clone()
    t[0, 0] = math.inf
    case["a"] = t
    got = _launch(case)
    want = ref.reference(case)
    m = case["kw"]["mask"].float()
    assert bool((m[i] <= 0).any()) and bool((m[i] > 0).any())
    assert bool((got[i].float()[m[i] <= 0] == 0).all())
    assert bool(torch.isnan(got[i].float()[m[i] > 0]).all())
    ref.assert_exact(got, want, _tile_of(s), s["name"])


# ---------------------------------------------------------------------------------------------
# 4. split-K

@pytest.mark.parametrize("kernel", sorted(_by_kernel(ref.SPLITK)))
def test_split_k_is_exact(kernel):
    """splits 2, 3, 8, 11 at K 200, 520, 584 (slices are whole 64-deep tiles, so the effective
    count differs from the request and the last slice is short), tiles 0, 1, 2, the vector and
    the scalar path of ``gemm_splitk_reduce`` (N % 4, ldc % 4, C off 16 bytes, ncol -- through
    ``mm_grouped``, which keeps the requested count, so slices past K are empty), beta, row map,
    bf16 out.  A NaN-filled block of the slab's size is freed just before each launch: most
    likely the slab, but the allocator does not guarantee it."""
    _exact(_by_kernel(ref.SPLITK)[kernel])


def test_split_k_in_launch_combine_is_exact(monkeypatch):
    """The combine by each tile's last-arriving workgroup, at up to 8 splits (all partials loaded
    at once) and beyond (the loop), and the tickets all zero afterwards."""
    from dinunet_implementations_amd.ops import gemm as G
    monkeypatch.setattr(G, "_SPLITK_INLAUNCH", True)
    assert {ref.eff_splits(s["K"], s["splits"]) > 8 for s in ref.INLAUNCH if not s["ncol"]} == \
        {True, False}
    _exact(ref.INLAUNCH, inlaunch=True)
    torch.cuda.synchronize()
    assert int(G._TICKETS[torch.device(DEV, torch.cuda.current_device())].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------
# 5. grouped launches

def _ints(g, *shape, dtype=F32, lo=-15, hi=15):
    return torch.randint(lo, hi + 1, shape, generator=g).float().to(dtype)


def _group(g, shapes, dtype=BF, opts=True, colsum=None, bdt=None):
    """Weight-gradient shaped problems ``out[M, N] (+)= a[K, M]^T b[K, N]`` on the CPU."""
    probs = []
    for i, (M, N, K) in enumerate(shapes):
        q = dict(a=_ints(g, K, M, dtype=dtype), b=_ints(g, K, N, dtype=bdt or dtype))
        rows = M
        if opts and i % 2 == 0:
            rows = M + 3
            rm = torch.randperm(rows, generator=g)[:M].to(torch.int32)
            if M > 2:
                rm[M // 2] = -1
            q["row_map"] = rm
        q["out"] = _ints(g, rows, N)
        if opts:
            q.update(alpha=(1.0, 0.5, 2.0)[i % 3], beta=(1.0, 0.0, 1.0, 2.0)[i % 4])
            if i % 3 != 1 and not (colsum and i in colsum):
                q["bias"] = _ints(g, N) / 4
        else:
            q["beta"] = 1.0
        if colsum and i in colsum:
            q["colsum"] = tuple(_ints(g, rows) for _ in range(colsum[i]))
        probs.append(q)
    return probs


def _on_gpu(probs, fill_ops=NAN):
    """The problems with every tensor embedded on the GPU, and the surround checks."""
    out, checks = [], []
    for i, q in enumerate(probs):
        d = {}
        for k, v in q.items():
            if k in ("a", "b", "out", "out2"):
                d[k], c = ref.embed(v, fill=fill_ops if k in "ab" else ref.SENTINEL, device=DEV)
                checks.append((f"problem {i} {k}", c))
            elif k == "colsum":
                pairs = [ref.embed(x, device=DEV) for x in v]
                d[k] = tuple(p[0] for p in pairs)
                checks += [(f"problem {i} colsum {j}", p[1]) for j, p in enumerate(pairs)]
            elif torch.is_tensor(v):
                d[k] = v.to(DEV)
            else:
                d[k] = v
        out.append(d)
    return out, checks


def _check_group(probs, dev, checks, want, what):
    torch.cuda.synchronize()
    for n, c in checks:
        c(f"{what}: surround of {n}")
    for i, (q, w) in enumerate(zip(dev, want)):
        for k in ("out", "out2"):
            if k in w:
                ref.assert_exact(q[k].cpu(), w[k], 64, f"{what}: problem {i} {k}")
        for k, x in zip(("x1", "x2"), q.get("colsum") or ()):
            assert torch.equal(x.cpu(), w[k]), f"{what}: problem {i} column sum {k}"


def _run_group(probs, what, **kw):
    from dinunet_implementations_amd.ops import gemm as G
    want = ref.grouped(probs, trans_a=True)
    dev, checks = _on_gpu(probs)
    sp = kw.get("splits") or 1
    if sp > 1:
        _poison(sp * sum(q["a"].shape[1] * q["b"].shape[1] for q in probs))
    G.mm_grouped(dev, trans_a=True, **kw)
    _check_group(probs, dev, checks, want, what)


MIXED_K = [(136, 72, 64), (72, 264, 200), (264, 136, 584), (8, 8, 64), (64, 520, 584)]


@pytest.mark.parametrize("tile", [0, 1, 2])
@pytest.mark.parametrize("splits", [1, 3])
def test_grouped_problems_of_different_depth_are_exact(tile, splits):
    """Different M, N and K (64, 200, 584) under one split count: the K = 64 problem's second
    and third slices are empty and must count as zero.  Row maps with dropped rows, per-problem
    alpha and beta, bias; the LDS-DMA kernels and (odd shapes, fp32 operands) the register-staged
    one."""
    g = torch.Generator().manual_seed(50 + tile)
    _run_group(_group(g, MIXED_K), f"tile {tile} splits {splits}", tile=tile, splits=splits)
    odd = [(65, 63, 64), (129, 7, 201), (1, 130, 584)]
    _run_group(_group(g, odd, dtype=F32), f"odd, tile {tile} splits {splits}", tile=tile,
               splits=splits)


@pytest.mark.parametrize("splits", [1, 3])
def test_grouped_ncol_and_twin_output_are_exact(splits):
    g = torch.Generator().manual_seed(60)
    K = 200
    a = _ints(g, K, 72, dtype=BF)
    ones = torch.ones(K, 8, dtype=BF)
    rm = torch.randperm(80, generator=g)[:72].to(torch.int32)
    rm[5] = -1
    probs = [dict(a=a, b=_ints(g, K, 136, dtype=BF), out=_ints(g, 72, 136), beta=1.0),
             dict(a=a, b=ones, out=_ints(g, 72, 1), out2=_ints(g, 72, 1), beta=1.0, ncol=1),
             dict(a=a, b=ones, out=_ints(g, 80, 1), out2=_ints(g, 80, 1), beta=0.0, alpha=0.5,
                  ncol=1, row_map=rm)]
    _run_group(probs, f"ncol splits {splits}", splits=splits)


@pytest.mark.parametrize("tile,splits,fold", [(0, 1, False), (0, 3, False), (1, 1, True),
                                              (1, 3, True), (2, 3, True), (1, 3, False)])
def test_grouped_column_sums_are_the_exact_sums(tile, splits, fold, monkeypatch):
    """``colsum`` folded into its problem (B's virtual ones column, 128 and 256 tiles on the
    LDS-DMA kernel) and as its own ``a^T @ ones`` problem: integers, so equal, not close."""
    from dinunet_implementations_amd.ops import gemm as G
    monkeypatch.setattr(G, "COLSUM_FOLD", fold)
    g = torch.Generator().manual_seed(70)
    shapes = [(136, 192, 200), (72, 64, 584), (264, 256, 64)]
    probs = _group(g, shapes, colsum={0: 2, 1: 1, 2: 1})
    dev, _ = _on_gpu(probs)
    placed, t = G._place_colsums(list(dev), True, False, tile)
    assert sum("colsum_folded" in q for q in placed) == (3 if fold and tile else 0)
    _run_group(probs, f"colsum tile {tile} splits {splits} fold {fold}", tile=tile, splits=splits)


def test_grouped_thirteen_problems_and_two_launch_classes():
    """13 problems (chunks of GMAX = 12), and one call whose problems fall into two launch
    classes: fp32 ``b`` operands beside the bf16 ones operand of a separate column sum."""
    from dinunet_implementations_amd.ops import gemm as G
    assert G.GMAX == 12
    g = torch.Generator().manual_seed(80)
    shapes = [(8 * (1 + i % 5), 8 * (2 + i % 3), (64, 200, 136)[i % 3]) for i in range(13)]
    _run_group(_group(g, shapes), "13 problems", splits=3)
    probs = _group(g, [(72, 136, 200), (65, 63, 129)], dtype=BF, bdt=F32, colsum={0: 1, 1: 2})
    dev, _ = _on_gpu(probs)
    placed, _ = G._place_colsums(list(dev), True, False, 0)
    assert len({G._launch_class(q, True, False) for q in placed}) == 2
    _run_group(probs, "two classes", splits=2)


@pytest.mark.parametrize("on", [True, False])
def test_grouped_xcd_order_is_exact(on, monkeypatch):
    """The slot -> tile permutation on and off: each equal to the reference."""
    from dinunet_implementations_amd.ops import gemm as G
    monkeypatch.setattr(G, "XCD_ORDER", on)
    g = torch.Generator().manual_seed(90)
    probs = _group(g, [(264, 136, 200), (136, 520, 584), (264, 72, 64)], colsum={2: 1})
    dev, _ = _on_gpu(probs)
    arrs = dict(M=[264, 136, 264], N=[136, 520, 72], K=[200, 584, 64],
                A=[q["a"].data_ptr() for q in dev], B=[q["b"].data_ptr() for q in dev])
    assert G._xcd_order(arrs, 128, torch.device(DEV)) is not None   # the order is not the plain one
    _run_group(probs, f"xcd order {on}", tile=1, splits=3)


def test_grouped_deferred_reduce_leaves_the_documented_slab():
    """``slab_sink`` takes the combine: the launch writes problem i's raw partials at ``slab +
    splits * sum_{j<i} M_j N_j`` as ``[splits][M_i][N_i]`` and launches no reduce; summed over the
    splits they are the exact products (no alpha, beta, bias or row map applied), empty slices
    zero, and the outputs are untouched."""
    from dinunet_implementations_amd.ops import gemm as G
    g = torch.Generator().manual_seed(95)
    shapes = [(72, 136, 584), (65, 63, 64), (8, 264, 200)]
    probs = _group(g, shapes, dtype=F32)
    dev, checks = _on_gpu(probs)
    seen = {}

    def sink(descs, slab):
        seen.update(descs=descs, slab=slab)
        return True
    before = G.reduce_launches()
    _poison(3 * sum(M * N for M, N, _ in shapes))
    G.mm_grouped(dev, trans_a=True, splits=3, tile=0, slab_sink=sink)
    torch.cuda.synchronize()
    assert G.reduce_launches() == before and len(seen["descs"]) == 3
    slab, off = seen["slab"].cpu(), 0
    for i, ((M, N, K), q, d) in enumerate(zip(shapes, probs, seen["descs"])):
        assert (d.M, d.N, d.splits) == (M, N, 3)
        assert d.slab == seen["slab"].data_ptr() + 4 * off
        parts = slab[off:off + 3 * M * N].view(3, M, N)
        want = q["a"].double().t() @ q["b"].double()
        ref.assert_exact(parts.double().sum(0), want, 64, f"slab of problem {i}")
        kchunk = (-(-K // 3) + 63) // 64 * 64
        for z in range(3):
            k0, k1 = min(K, z * kchunk), min(K, (z + 1) * kchunk)
            wz = q["a"].double()[k0:k1].t() @ q["b"].double()[k0:k1]
            ref.assert_exact(parts[z], wz, 64, f"slice {z} of problem {i}")
        off += 3 * M * N
        ref.assert_exact(dev[i]["out"].cpu(), q["out"], 64, f"output of problem {i}")
    for n, c in checks:
        c(f"deferred reduce: surround of {n}")


# ---------------------------------------------------------------------------------------------
# 6. rows gathered from the dataset

@pytest.mark.parametrize("S", [64, 70, 98])
@pytest.mark.parametrize("tile", [0, 1, 2])
def test_gathered_rows_are_exact(S, tile):
    """``rows_from``: a k-contiguous A and a k-major B (``splits=3``) read in place from the
    dataset through subject indices that repeat and include the dataset's last subject; K = B * S
    ends on a subject boundary, where the k-major stream still loads ``subj[b0 + 1]`` (the spare
    entry).  The registered buffer itself is NaN: reading it shows."""
    from dinunet_implementations_amd.ops import gemm as G
    g = torch.Generator().manual_seed(100 + S)
    n_subj, F, O = 9, 136, 72
    subj = torch.tensor([3, n_subj - 1, 3, 0, n_subj - 1, 5], dtype=torch.int64)  # last: spare
    B = subj.numel() - 1
    Xb = torch.full(((n_subj + 2) * S, F), NAN, dtype=BF)
    Xb[S:-S] = _ints(g, n_subj * S, F, dtype=BF)
    Xd = Xb.to(DEV)
    X = Xd[S:-S]
    rows = (subj[:B, None] * S + torch.arange(S)[None, :]).reshape(-1)
    xc = Xb[S:-S][rows]
    w = _ints(g, O, F, dtype=BF)
    dy = _ints(g, B * S, O, dtype=BF)
    buf = torch.full((B * S, F), NAN, dtype=BF, device=DEV)
    wv, cw = ref.embed(w, fill=NAN, device=DEV)
    dyv, cdy = ref.embed(dy, fill=NAN, device=DEV)
    y, cy = ref.embed(torch.full((B * S, O), ref.SENTINEL, dtype=BF), device=DEV)
    dw, cdw = ref.embed(torch.full((O, F), ref.SENTINEL), device=DEV)
    _poison(3 * O * F)
    with G.rows_from(buf, X, subj.to(DEV), S):
        G.mm(buf, wv, trans_b=True, out=y, tile=tile)
        G.mm(dyv, buf, trans_a=True, out=dw, tile=tile, splits=3)
    torch.cuda.synchronize()
    for what, c in (("w", cw), ("dy", cdy), ("y", cy), ("dw", cdw)):
        c(f"gather S={S} tile {tile}: surround of {what}")
    assert torch.equal(Xd.cpu().view(torch.int16), Xb.view(torch.int16))
    ref.assert_exact(y.cpu(), ref.gemm(xc, w, trans_b=True, out_dtype=BF), 64, f"y, S={S}")
    ref.assert_exact(dw.cpu(), ref.gemm(dy, xc, trans_a=True), 64, f"dW, S={S}")


# ---------------------------------------------------------------------------------------------
# 7. rounding and numerics

def test_fp32_operands_are_rounded_to_nearest_even():
    """Operands that are exact ties between two bf16 values: a truncating ``to_bf`` gives other
    products, so the exact result proves RNE, on both stagers and either fp32 side."""
    for s in ref.NUMERICS:
        case = ref.make_case(s)
        want = ref.reference(case)
        assert ref.mismatch(ref.reference(case, to_bf=ref.trunc_bf), want).count > 0
    _exact(ref.NUMERICS)


@pytest.mark.parametrize("name", [s["name"] for s in ref.GAUSS])
def test_gaussian_operands_within_the_rule(name):
    """N(0, 1) fp32 operands, not pre-rounded, three shapes per staging path and K = 4096."""
    s = ref.find(name)
    case = ref.make_case(s)
    got = _launch(case)
    S = ref.scale(case)
    ref64 = ref.reference(case, torch.float64, None)
    base = ref.reference(case, F32)
    e_k, e_b = ref.elem_err(got, ref64, S), ref.elem_err(base, ref64, S)
    print(f"{name} [{s['path']}]: E_kernel {e_k:.3e} E_base {e_b:.3e} "
          f"ratio {e_k / max(e_b, ref.U23):.2f}")
    _record("gemm", name, e_k, e_b)
    ref.assert_close(got, ref64, base, S, f"{name} [{s['path']}]")
