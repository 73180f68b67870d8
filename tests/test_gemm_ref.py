"""The reference of ``tests/gemm_ref.py`` held to account, on the CPU: against an independent
composite in fp64, against the CPU path of ``ops.gemm.mm`` / ``mm_grouped`` (the oracle the
model-level tests lean on), the exactness condition of every exact case of
``tests/test_gemm_exact_gpu.py``, the kernel each of its launches is meant to reach (``route``),
the deliberately wrong results (each must be caught by ``mismatch`` or the rule; the table of the
ones the older whole-matrix bound misses is asserted), and ``embed``."""
import math

import pytest
import torch

import gemm_ref as ref

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16


def _composite(a, b, ta, tb, alpha, beta, bias, relu, mask, row_map, ncol, c0):
    """torch.matmul in fp64 plus explicit loops for the row map and ncol."""
    A = (a.t() if ta else a).to(BF).double()
    B = (b.t() if tb else b).to(BF).double()
    v = torch.matmul(A, B) * alpha
    out = c0.double().clone()
    M, N = v.shape
    for i in range(M):
        o = i if row_map is None else int(row_map[i])
        if o < 0:
            continue
        for j in range(N if not ncol else min(N, ncol)):
            x = float(v[i, j])
            if bias is not None:
                x += float(bias[j])
            if relu and x < 0:
                x = 0.0
            if mask is not None and not float(mask[i, j]) > 0:
                x = 0.0
            if beta != 0:
                x += beta * float(c0[o, j])
            out[o, j] = x
    return out


@pytest.mark.parametrize("lay", range(4))
@pytest.mark.parametrize("opts,ncol", [((), 0), (("alpha",), 0), (("bias",), 0), (("relu",), 0),
                                       (("mask",), 0), (("beta",), 0), (("rmap",), 0), ((), 1),
                                       ((), 5), (ref.OPTS, 5), (ref.OPTS, 0)])
def test_gemm_equals_independent_composite(lay, opts, ncol):
    s = ref.spec("c", 13, 9, 21, lay=lay, kind="gauss", adt="fp32", bdt="fp32", opts=opts,
                 ncol=ncol)
    c = ref.make_case(s)
    kw = c["kw"]
    want = _composite(c["a"], c["b"], kw["trans_a"], kw["trans_b"], kw.get("alpha", 1.0),
                      kw.get("beta", 0.0), kw.get("bias"), kw.get("relu", False), kw.get("mask"),
                      kw.get("row_map"), kw.get("ncol"), c["c0"])
    got = ref.reference(c, F64, None)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    if "rmap" in opts:   # dropped rows and the five spare rows keep c0
        rm = kw["row_map"].long()
        untouched = sorted(set(range(c["c0"].shape[0])) - set(rm[rm >= 0].tolist()))
        assert len(untouched) == 5 + int((rm < 0).sum())
        assert torch.equal(got[untouched], c["c0"].double()[untouched])
    if ncol:
        assert torch.equal(got[:, ncol:], c["c0"].double()[:, ncol:])


def test_reference_keeps_nan_through_relu_and_selects_the_mask():
    a = torch.tensor([[1.0, math.nan], [1.0, 2.0]])
    b = torch.eye(2)
    r = ref.gemm(a, b, relu=True)
    assert bool(torch.isnan(r[0]).all()) and torch.equal(r[1], torch.tensor([1.0, 2.0]))
    m = torch.tensor([[-1.0, 0.0], [-0.0, 1.0]]).to(BF)
    r = ref.gemm(a, b, relu=True, mask=m)
    assert torch.equal(r, torch.tensor([[0.0, 0.0], [0.0, 2.0]]))
    m = torch.tensor([[1.0, math.nan], [1.0, 1.0]]).to(BF)
    r = ref.gemm(a, b, mask=m)
    assert math.isnan(float(r[0, 0])) and float(r[0, 1]) == 0.0


# ---------------------------------------------------------------------------------------------
# the CPU path of ops.gemm (plumbing / oracle)

@pytest.mark.parametrize("lay", range(4))
@pytest.mark.parametrize("opts", [(), ("alpha", "bias", "relu"), ("mask",), ("beta",), ("rmap",),
                                  ref.OPTS])
@pytest.mark.parametrize("out", ["fp32", "bf16"])
def test_cpu_mm_agrees_with_reference(lay, opts, out):
    from dinunet_implementations_amd.ops.gemm import mm
    c = ref.make_case(ref.spec("c", 37, 21, 40, lay=lay, opts=opts, out=out))
    kw = c["kw"]
    o = c["c0"].clone()
    r = mm(c["a"], c["b"], trans_a=kw["trans_a"], trans_b=kw["trans_b"], out=o,
           bias=kw.get("bias"), relu=kw.get("relu", False), alpha=kw.get("alpha", 1.0),
           beta=kw.get("beta", 0.0), row_map=kw.get("row_map"), mask=kw.get("mask"))
    assert r is o
    ref.assert_exact(o, ref.reference(c), what=f"cpu mm {opts}")


def test_cpu_mm_without_out_and_row_map_branch():
    from dinunet_implementations_amd.ops.gemm import mm
    c = ref.make_case(ref.spec("c", 12, 8, 16, opts=("rmap", "bias")))
    kw = c["kw"]
    r = mm(c["a"], c["b"], trans_b=True, bias=kw["bias"], row_map=kw["row_map"])
    want = ref.gemm(c["a"], c["b"], trans_b=True, bias=kw["bias"], row_map=kw["row_map"])
    assert r.shape == want.shape == (int(kw["row_map"].max()) + 1, 8)
    ref.assert_exact(r, want, what="row_map, out=None")
    r = mm(c["a"], c["b"], trans_b=True, out_dtype=BF)
    assert r.dtype == BF
    ref.assert_exact(r, ref.gemm(c["a"], c["b"], trans_b=True, out_dtype=BF), what="out=None")


def test_cpu_mm_mask_is_a_select_for_non_finite_values():
    """A NaN product under ``mask <= 0`` is 0 (the kernel's select, torch's ReLU backward), not
    NaN * 0."""
    from dinunet_implementations_amd.ops.gemm import mm
    c = ref.make_case(ref.spec("c", 9, 8, 16, lay=1, opts=("mask",)))
    a = c["a"].float()
    a[2, 3] = math.nan
    a[5, 0] = math.inf
    m = c["kw"]["mask"]
    assert bool((m[2] <= 0).any()) and bool((m[2] > 0).any())
    got = mm(a, c["b"], mask=m)
    want = ref.gemm(a, c["b"], mask=m)
    ref.assert_exact(got, want, what="mask over NaN")
    assert bool((got[2][m[2] <= 0] == 0).all()) and bool(torch.isnan(got[2][m[2] > 0]).all())


def _grouped_problems(g, device="cpu"):
    def ints(*shape):
        return torch.randint(-15, 16, shape, generator=g).float()
    K = 24
    a0, b0 = ints(K, 10).to(BF), ints(K, 16).to(BF)
    a1, b1 = ints(K, 7).to(BF), ints(K, 8).to(BF)
    rm = torch.tensor([3, -1, 0, 8, 5, 1, 9], dtype=torch.int32)
    ones = torch.ones(K, 8, dtype=BF)
    return [dict(a=a0, b=b0, out=ints(10, 16), beta=1.0, alpha=0.5, bias=ints(16) / 4,
                 colsum=(ints(10), ints(10))),
            dict(a=a1, b=b1, out=ints(10, 8), beta=1.0, row_map=rm, colsum=(ints(10),)),
            dict(a=a1, b=ones, out=ints(7, 1), out2=ints(7, 1), beta=1.0, ncol=1)]


def test_cpu_mm_grouped_agrees_with_reference():
    from dinunet_implementations_amd.ops.gemm import mm_grouped
    g = torch.Generator().manual_seed(3)
    probs = _grouped_problems(g)
    want = ref.grouped(probs, trans_a=True)
    mm_grouped(probs, trans_a=True)
    for q, w in zip(probs, want):
        ref.assert_exact(q["out"], w["out"], what="grouped out")
        if "out2" in w:
            ref.assert_exact(q["out2"], w["out2"], what="grouped out2")
        for k, x in zip(("x1", "x2"), q.get("colsum") or ()):
            assert torch.equal(x, w[k]), k
    # the column sums are the exact integer sums; a dropped row leaves its place untouched
    first = _grouped_problems(torch.Generator().manual_seed(3))
    a1 = probs[1]["a"].double()
    assert torch.equal(want[2]["out"][:, 0].double(), first[2]["out"][:, 0].double() + a1.sum(0))
    x1, x0 = want[1]["x1"].double(), first[1]["colsum"][0].double()
    assert float(x1[3]) == float(x0[3] + a1[:, 0].sum()) and float(x1[2]) == float(x0[2])


@pytest.mark.parametrize("name", ["epi-dma64-f-ncol5-all", "epi-gen128-b-ncol1-all",
                                  "epi-dma64-b-ncol1"])
def test_cpu_mm_grouped_ncol_into_a_wider_output(name):
    """``ncol`` with an output as wide as ``b`` (and a bias of N entries): the columns from
    ``ncol`` on keep what they held, as on the GPU."""
    from dinunet_implementations_amd.ops.gemm import mm_grouped
    c = ref.make_case(ref.find(name))
    kw = c["kw"]
    out = c["c0"].clone()
    q = dict(a=c["a"], b=c["b"], out=out, alpha=kw.get("alpha", 1.0), beta=kw.get("beta", 0.0),
             ncol=kw["ncol"], bias=kw.get("bias"), row_map=kw.get("row_map"))
    mm_grouped([q], trans_a=kw["trans_a"], trans_b=kw["trans_b"])
    ref.assert_exact(out, ref.reference(c), what=name)


# ---------------------------------------------------------------------------------------------
# the cases of the GPU file

def _all_specs():
    out = []
    for name, L in ref.EXACT_LISTS.items():
        out += [(name, s) for s in L]
    out += [("nan", s) for _, s, _, _ in ref.NAN_SITES]
    return out


def test_case_names_are_unique_and_within_the_size_limit():
    specs = [s for _, s in _all_specs()] + ref.GAUSS
    names = [s["name"] for s in specs]
    assert len(set(names)) == len(names)
    for s in specs:
        assert max(s["M"], s["N"]) <= 520, s["name"]
        assert s["K"] <= (4096 if "k4096" in s["name"] else 1024), s["name"]


@pytest.mark.parametrize("which", list(ref.EXACT_LISTS) + ["nan"])
def test_exact_ok_holds_for_every_exact_case(which):
    specs = [s for n, s in _all_specs() if n == which]
    assert specs
    for s in specs:
        assert s["kind"] in ("int", "tie")
        assert ref.exact_ok(ref.make_case(s)), s["name"]


def test_exact_ok_refuses_what_is_not_exact():
    c = ref.int_case(8, 8, 64)
    assert ref.exact_ok(c)
    # the claim the exact tests rest on, at its stated limit: fp32 equals fp64 bit for bit
    big_k = ref.int_case(129, 72, 4096, lay=1)
    assert ref.exact_ok(big_k) and 2.0 ** 17 < float(ref.scale(big_k).max()) < 2.0 ** 24
    assert ref.exact_ok(ref.tie_case(72, 65, 1024)) and ref.exact_ok(ref.tie_case(9, 8, 1024, "b"))
    assert not ref.exact_ok(ref.gauss_case(8, 8, 64))
    big = dict(c, a=c["a"] * 2048, b=c["b"] * 2048)       # sums past 2^24
    assert not ref.exact_ok(big)
    frac = dict(c, a=(c["a"].float() + 1 / 3).to(BF))     # fp32 sums round
    frac["b"] = (c["b"].float() * 1.37).to(BF)
    assert not ref.exact_ok(frac)
    assert not ref.exact_ok(ref.make_case(ref.spec("g", 8, 8, 64, kind="gauss")))


@pytest.mark.parametrize("which", list(ref.EXACT_LISTS) + ["nan", "gauss"])
def test_every_launch_is_routed_to_the_kernel_it_names(which):
    """``route`` (the dispatch of ``run_group`` / ``launch`` mirrored) on the tensors as
    ``place`` lays them out: what forces each path is the shape, the types, the ``embed``
    offsets, ``tile``, ``splits`` and the LDS-DMA switch of the spec."""
    specs = ref.GAUSS if which == "gauss" else [s for n, s in _all_specs() if n == which]
    seen = set()
    for s in specs:
        c = ref.make_case(s)
        a, b, out, mk, _ = ref.place(c)
        got = ref.route(s, a, b, out, mk.get("mask"), inlaunch=which == "inlaunch")
        assert got == s["path"], (s["name"], got)
        seen.add(got)
    if which == "paths":
        assert {"gen64/scalar", "gen128/scalar", "vec64/scalar", "vec128/scalar", "dma64r4/vepi",
                "dma64r2/reduce4", "dma128/vepi", "g256/vepi", "dma128/scalar"} <= seen
        for adt, bdt in ref.DTYPES:   # VEC=false: every type pair, off by shape, base and ld
            for how in ("shape", "base", "ld"):
                assert any(s["name"].startswith(f"gen64-{how}-{adt[0]}{bdt[0]}") for s in specs)
        for k in ("gen64-shape", "vec64", "dma64r4", "dma128", "g256", "dma64r2"):
            assert {s["lay"] for s in specs if s["name"].startswith(k)} == {0, 1, 2, 3}, k


def test_shape_edges_are_all_used():
    P = ref.PATHS
    for T, key, sets in ((64, "dma64r4", ref.mn8(64)), (128, "dma128", ref.mn8(128)),
                         (64, "vec64", ref.mn8(64))):
        L = [s for s in P if s["name"].startswith(key)]
        assert {s["M"] for s in L} >= set(sets) and {s["N"] for s in L} >= set(sets), key
    assert {s["K"] for s in P} >= set(ref.KS)
    assert ref.eff_splits(584, 8) == 5 and ref.eff_splits(584, 10) == 10
    assert ref.eff_splits(200, 11) == 4 and ref.eff_splits(200, 2) == 2


# ---------------------------------------------------------------------------------------------
# mutations

EXACT_MUT = {"one_element": "split-t0-opts", "stale_vector": "split-t0-opts-bf",
             "drop_last_kchunk": "split-t0-opts", "double_k_at_split": "split-t0-opts",
             "truncation": "tie-vec64-0", "bias_last8": "epi-dma64-b-all",
             "beta_per_split": "split-t0-opts", "rowmap_shift": "split-t0-opts",
             "mask_lt0": "epi-dma64-f-mask", "store_at_ncol": "split-t0-ncol",
             "relu_nan_to_zero": "nan-dma64"}


def test_every_mutation_has_a_case():
    assert set(EXACT_MUT) == set(ref.MUTATIONS)


@pytest.mark.parametrize("name", ref.MUTATIONS)
def test_mutation_is_a_mismatch_at_a_named_tile(name):
    s = dict(ref.NAN_SITES[1][1]) if EXACT_MUT[name] == "nan-dma64" else ref.find(EXACT_MUT[name])
    c = ref.make_case(s)
    wrong, right = ref.mutated(name, c)
    odt = ref.DT[s["out"]]
    m = ref.mismatch(wrong.to(odt), right.to(odt))
    assert m.count > 0 and m.tile == (m.first[0] // 64, m.first[1] // 64)
    with pytest.raises(AssertionError, match=r"tile \(\d+, \d+\) of 64 x 64"):
        ref.assert_exact(wrong.to(odt), right.to(odt), what=name)
    assert ref.mismatch(right.to(odt), right.to(odt)).count == 0


# The arithmetic mutations on Gaussian operands: at the shapes of the GPU file, and at the two
# shapes tests/test_kernels_gpu.py judges by its whole-matrix bound.  (mutation, case, the rule
# catches it, it slips under the older bound.)  Measured here, worst E_mut / max(E_base, 2^-23)
# left to right: fp32 outputs 1e4 .. 2e6; a bias missing from a bf16 output 3 .. 8, which is the
# size of the output rounding itself (|bias| ~ 1 beside values ~ sqrt(K) kept to 8 bits) -- that
# one only the exact cases see.
_OLD = {"old-333": ref.spec("old-333", 333, 197, 420, kind="gauss", adt="fp32", bdt="fp32"),
        "old-333-bf": ref.spec("old-333-bf", 333, 197, 420, kind="gauss", adt="fp32", bdt="fp32",
                               out="bf16", opts=("bias", "relu")),
        "old-3136": ref.spec("old-3136", 3136, 256, 1000, kind="gauss", adt="fp32", bdt="fp32"),
        "old-3136-bf": ref.spec("old-3136-bf", 3136, 256, 1000, kind="gauss", out="bf16",
                                opts=("bias", "relu"))}
GAUSS_MUT = [("one_element", "gauss-vec-2", True, False),
             ("one_element", "gauss-gen-1", True, False),
             ("one_element", "old-333", True, True),
             ("one_element", "old-3136", True, True),
             ("drop_last_kchunk", "gauss-vec-2", True, True),
             ("drop_last_kchunk", "gauss-dma-1", True, True),
             ("drop_last_kchunk", "old-333", True, False),
             ("drop_last_kchunk", "old-3136", True, False),     # 6.5e-3 against 2e-3
             ("bias_last8", "gauss-relu-bf", False, True),
             ("bias_last8", "old-333-bf", False, True),
             ("bias_last8", "old-3136-bf", False, True),
             ("double_k_at_split", "gauss-k4096-split", True, False),
             ("double_k_at_split", "old-3136", True, False),
             ("truncation", "gauss-vec-2", True, False)]


@pytest.mark.parametrize("name,case,rule_catches,old_misses", GAUSS_MUT)
def test_mutation_against_the_rule_and_the_old_bound(name, case, rule_catches, old_misses):
    s = _OLD.get(case) or ref.find(case)
    c = ref.make_case(s)
    odt = ref.DT[s["out"]]
    wrong, right = ref.mutated(name, c)
    S = ref.scale(c)
    base = ref.reference(c, F32)
    e_k, e_b = ref.elem_err(wrong.to(odt), right, S), ref.elem_err(base, right, S)
    whole = ref.whole_err(wrong.to(odt), right)
    print(f"{name} on {case}: E_mut {e_k:.3e} E_base {e_b:.3e} whole {whole:.3e}")
    assert ref.within_rule(e_b, e_b)
    assert ref.within_rule(e_k, e_b) != rule_catches, (e_k, e_b)
    if rule_catches:
        with pytest.raises(AssertionError):
            ref.assert_close(wrong.to(odt), right, base, S, name)
    assert (whole < ref.OLD_BOUND[odt]) == old_misses, whole
    # the same fault on the exact operands of the same shape is a mismatch in every case
    ci = ref.make_case(dict(s, kind="int"))
    wi, ri = ref.mutated(name, ci)
    if name != "truncation":          # (integers in [-15, 15] are bf16 values: nothing to round)
        assert ref.mismatch(wi.to(odt), ri.to(odt)).count > 0


@pytest.mark.parametrize("case", [s["name"] for s in ref.GAUSS])
def test_baseline_passes_its_own_rule(case):
    """The fp32 evaluation against the fp64 one is within the rule, and ``S`` is nowhere near
    zero."""
    c = ref.make_case(ref.find(case))
    S = ref.scale(c)
    assert float(S.min()) > 1e-3
    right = ref.reference(c, F64, None)
    base = ref.reference(c, F32)
    e_k, e_b = ref.assert_close(base, right, base, S, case)
    assert e_k == e_b


# ---------------------------------------------------------------------------------------------
# rounding, embed

def test_tie_operands_tell_rne_from_truncation():
    c = ref.make_case(ref.find("tie-gen64-0"))
    a = c["a"].float()
    assert bool(((a.abs() >= 257) & (a.abs() <= 511) & (a.abs() % 2 == 1)).all())
    r, t = ref.bf(a), ref.trunc_bf(a)
    assert bool(((r - a).abs() == 1).all()) and bool(((t - a).abs() == 1).all())
    assert bool((t.abs() < a.abs()).all())
    frac = float((r != t).float().mean())
    assert 0.4 < frac < 0.6            # RNE goes up to the even neighbour half of the time
    assert torch.equal(ref.trunc_bf(torch.tensor([1.0, -2.5, 0.0])), torch.tensor([1.0, -2.5, 0.0]))


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("offset", [0, 1, (1, 0), (0, 1)])
def test_embed_round_trips_and_its_check_fires(dtype, offset):
    t = torch.arange(5 * 13, dtype=F32).reshape(5, 13).to(dtype)
    v, check = ref.embed(t, fill=math.nan, offset=offset)
    assert torch.equal(v, t) and v.stride(1) == 1 and v.stride(0) > 13
    ob, ol = (offset, offset) if isinstance(offset, int) else offset
    assert v.stride(0) % 8 == ol and v.storage_offset() % 8 == ob
    check("untouched")
    v[2, 3] = 99.0            # inside: not the check's business
    check("inside")
    base = v.storage_offset()
    flat = v.as_strided((base + 5 * v.stride(0) + 8,), (1,), 0)
    for where in (base - 1, base + 13, base + 4 * v.stride(0) + 13, 0, base - v.stride(0)):
        old = flat[where].clone()
        flat[where] = 1.0
        with pytest.raises(AssertionError, match="outside the view"):
            check("one element")
        flat[where] = old
        check("restored")
    x, cx = ref.embed(torch.arange(7.0))
    assert x.shape == (7,) and x.is_contiguous()
    cx()
