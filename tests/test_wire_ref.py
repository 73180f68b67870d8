"""The wire-format model of ``tests/wire_ref.py`` against ``parallel.collective``'s CPU path (bit
for bit), against the fp64 mean (the derived per-element bound), on poisoned gradients, and
against its own deliberately wrong variants.  No GPU: the kernels meet the same model in
``tests/test_wire_gpu.py`` and ``tests/test_peer_gpu.py``.

One limit of the format shows here and is stated, not tested away: the W site values are summed
in fp32 BEFORE the division by W, so ``sum_w |x_w|`` has to stay below 2^128 (``mean_bound``
returns inf otherwise, and the edge set keeps clear of it)."""
import numpy as np
import pytest
import torch

import wire_ref as R
from dinunet_implementations_amd.parallel import collective as C

TORCH_DT = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
SHAPES = R.shapes()
BIG = SHAPES[-1]


def bits_of(t, wire):
    """wire bits (numpy) of a torch payload tensor."""
    if wire == "fp32":
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.view(torch.int16).numpy().view(np.uint16)


def tensor_of(bits, wire):
    if wire == "fp32":
        return torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)
    return torch.from_numpy(bits.view(np.int16).copy()).view(TORCH_DT[wire])


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("poison", [False, True], ids=["edge", "poisoned"])
@pytest.mark.parametrize("wire,scaled", R.MODES, ids=[f"{w}{'' if s else '-unscaled'}" for w, s in R.MODES])
@pytest.mark.parametrize("n,W", SHAPES, ids=[f"n{n}-W{W}" for n, W in SHAPES])
def test_model_equals_collective_cpu(n, W, wire, scaled, poison):
    """pack, rowsum and unpack of the model and of collective.py's CPU path agree in every bit
    (both-NaN positions apart) at scales 1, 1/2 and 1/3."""
    xs, _ = R.inputs(n, W, poison)
    chunk = R.chunk_for(n, W)
    assert chunk == C.chunk_for(n, W) and R.numel(chunk) == C.payload_numel(chunk)
    blk = R.numel(chunk)
    dt = TORCH_DT[wire]
    for scale in R.SCALES:
        sent, means, out = R.staged(n, W, wire, scaled, scale, poison)
        for w in range(W):
            dst = torch.full((W * blk,), 7.0, dtype=dt)
            C.to_payload(torch.from_numpy(np.array(xs[w])), dst, W, chunk, scale, scaled)
            bad = R.mismatches(bits_of(dst, wire), sent[w], wire)
            assert bad.size == 0, ("pack", scale, w, bad[:8])
        red = float(np.float32(scale) / np.float32(W))
        for r in range(W):
            src = tensor_of(np.concatenate([s[r * blk:(r + 1) * blk] for s in sent]), wire)
            dst = torch.full((blk,), 7.0, dtype=dt)
            C.rowsum(src, dst, W, chunk, red)
            bad = R.mismatches(bits_of(dst, wire), means[r], wire)
            assert bad.size == 0, ("rowsum", scale, r, bad[:8])
        got = torch.full((n,), 7.0)
        C.from_payload(tensor_of(np.concatenate(means), wire), got, W, chunk, scale)
        bad = R.mismatches(f32_bits(got.numpy()), f32_bits(out), "fp32")
        assert bad.size == 0, ("unpack", scale, bad[:8])


@pytest.mark.parametrize("wire", R.WIRES)
@pytest.mark.parametrize("n,W", SHAPES, ids=[f"n{n}-W{W}" for n, W in SHAPES])
def test_model_mean_within_the_derived_bound(n, W, wire):
    """|model mean - fp64 mean| <= the bound of wire_ref's docstring at every element.  (The
    model's own worst ratio: about 0.99997 on fp16, reached where both roundings fall the same
    way at a sub-block maximum just above a power of two.)"""
    xs, _ = R.inputs(n, W, False)
    out = R.site_mean(xs, wire)
    assert np.array_equal(f32_bits(out), f32_bits(R.staged(n, W, wire, True, 1.0, False)[2]))
    assert np.all(np.isfinite(out))
    ratio = R.err_ratio(out, xs, wire)
    print(f"wire {wire} n {n} W {W}: error / bound = {ratio:.5f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("wire", R.WIRES)
@pytest.mark.parametrize("n,W", SHAPES, ids=[f"n{n}-W{W}" for n, W in SHAPES])
def test_poison_reaches_the_mean_and_nothing_else(n, W, wire):
    """The planted NaN is NaN in the mean, +inf against -inf is NaN, a lone infinity keeps its
    sign; no other element is NaN, and every sub-block without a plant is bit-identical to the
    clean run's."""
    xs, _ = R.inputs(n, W, False)
    ys, planted = R.inputs(n, W, True)
    clean, dirty = R.site_mean(xs, wire), R.site_mean(ys, wire)
    want_nan = sorted(i for i, k in planted.items() if k == "nan")
    assert np.flatnonzero(np.isnan(dirty)).tolist() == want_nan
    assert len(want_nan) == (1 if len(planted) == 1 else 2)
    for i, k in planted.items():
        if k != "nan":
            assert dirty[i] == (np.inf if k == "+inf" else -np.inf), (i, k, dirty[i])
    touched = {i // R.SB for i in planted}
    keep = np.ones(n, dtype=bool)
    for g in touched:
        keep[g * R.SB:(g + 1) * R.SB] = False
    assert np.array_equal(f32_bits(clean)[keep], f32_bits(dirty)[keep])
    if (n, W) == BIG:
        assert sorted(planted.values()) == ["+inf", "-inf", "nan", "nan"]


def _subblocks_with(name, n, W):
    """(site, sub-block) pairs of the grid's inputs that hold the named pattern."""
    seed = n % 1000 + W
    return [(w, g) for w in range(W) for g in range(-(-n // R.SB))
            if R.PATTERNS[R.pattern_of(g, w, seed)] == name]


# mutation -> (shape, poisoned, the stage that first differs, the pattern that shows it or None)
CAUGHT_BY = {
    "amax_first_wave": (BIG, False, "pack", "last_only"),
    "amax_ignores_nan": (BIG, True, "pack", None),       # the header of the NaN's sub-block
    "emax": (BIG, False, "rowsum", None),                 # sixteen sites, sixteen exponents
    "round_every_add": (BIG, False, "rowsum", None),      # sixteen addends, each sum rounded
    "truncate": (BIG, False, "pack", "wide"),
    "header_late": ((1, 1), False, "pack", None),
    "pad_not_zeroed": ((2049, 3), False, "pack", None),   # 2047 + 2 * 2048 elements of padding
    "clamp_m100": (BIG, False, "pack", "max_2^116"),
}


def test_every_mutation_is_named():
    assert set(CAUGHT_BY) == set(R.MUTATIONS)


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutation_changes_a_bit(mut):
    (n, W), poison, stage, pattern = CAUGHT_BY[mut]
    xs, _ = R.inputs(n, W, poison)
    out, sent, means = R.site_mean(xs, "fp16", stages=True)
    out_m, sent_m, means_m = R.site_mean(xs, "fp16", mut=mut, stages=True)
    if stage == "pack":
        diff = [(w, int(i) // R.SBS) for w in range(W)
                for i in R.mismatches(sent_m[w], sent[w], "fp16")]
        assert diff
        if pattern is not None:
            hit = _subblocks_with(pattern, n, W)
            assert hit and set(hit) <= set(diff), (hit, sorted(set(diff))[:8])
        if mut == "amax_ignores_nan":
            assert (W - 1, 0) in diff
    else:
        assert all(R.mismatches(a, b, "fp16").size == 0 for a, b in zip(sent_m, sent))
        assert any(R.mismatches(a, b, "fp16").size for a, b in zip(means_m, means))
        assert R.mismatches(f32_bits(out_m), f32_bits(out), "fp32").size


def _range_cases():
    top = np.float32(2.0 - 2.0 ** -10)          # the largest 11-bit significand
    cases = [(k, [np.float32(2.0 ** k)] * 2) for k in (100, 114, 115, 116, 117, 120, 126)]
    cases += [(k, [np.float32(2.0 ** k) * top]) for k in (115, 116, 127)]
    cases += [(127, [np.float32(2.0 ** 127) * np.float32(1.5), np.float32(-2.0 ** 127)])]
    return cases


@pytest.mark.parametrize("k,vals", _range_cases(),
                         ids=[f"2^{k}-W{len(v)}-{i}" for i, (k, v) in enumerate(_range_cases())])
def test_finite_gradients_give_finite_fp16_means(k, vals):
    """Up to the top of fp32 (|x| with 11 significant bits, sum_w |x_w| < 2^128) the fp16 wire
    returns the mean exactly, in the model and in collective.py's CPU path: the sub-block
    exponent reaches down to -113.  (Clamped at -100, 2^116 and above left as inf.)"""
    W, n = len(vals), 5
    xs = [np.full(n, v, dtype=np.float32) for v in vals]
    for x in xs:
        x[1:] *= np.float32(2.0 ** -3)
    want = R.truth(xs)
    assert np.all(np.abs(want) < 2.0 ** 128)
    out = R.site_mean(xs, "fp16")
    assert np.array_equal(out.astype(np.float64), want), (out, want)
    chunk = C.chunk_for(n, W)
    blk = C.payload_numel(chunk)
    sent = []
    for x in xs:
        s = torch.zeros(W * blk, dtype=torch.float16)
        C.to_payload(torch.from_numpy(x), s, W, chunk)
        sent.append(s)
    means = []
    for r in range(W):
        m = torch.zeros(blk, dtype=torch.float16)
        C.rowsum(torch.cat([s[r * blk:(r + 1) * blk] for s in sent]), m, W, chunk, 1.0 / W)
        means.append(m)
    got = torch.zeros(n)
    C.from_payload(torch.cat(means), got, W, chunk)
    assert np.array_equal(got.numpy().astype(np.float64), want), (got, want)


def test_gather_model_is_a_round_trip():
    x = R.edge_gradients(5003, 1, seed=3)[0]
    for wire in R.WIRES:
        y = R.gathered(x, wire)
        if wire == "fp32":
            assert np.array_equal(f32_bits(y), f32_bits(x))
        else:
            assert R.err_ratio(y, [x], wire) <= 1.0
