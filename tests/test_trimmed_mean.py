"""Coordinate-wise trimmed mean / median engine (``agg_engine: trimmedMean``) on the CPU: the numpy
mirror against a per-coordinate Python ``sorted()`` with explicit fp32 adds, the torch path of
``TrimmedState.combine`` against the mirror, the engine across three gloo processes with a NaN
and a blown-up site (bit for bit against the mirror; dSGD lets the NaN through), configuration,
refusals, the file transport through the COINSTAC simulator and the counters' resume state.
"""
import struct

import numpy as np
import pytest
import torch
import torch.nn as nn

from mp_util import run_world

from dinunet_implementations_amd.ops import reference as ref

WS = (1, 2, 3, 4, 5, 6, 8, 16)
FLT_MAX = np.float32(3.4028234663852886e38)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _from_bits(b):
    return np.asarray(b, dtype=np.uint32).view(np.float32)


def _key(x) -> int:
    """The total-order key from the value's packed bytes (independent of the mirror's numpy)."""
    u = struct.unpack("<I", struct.pack("<f", x))[0] if not isinstance(x, np.float32) else \
        struct.unpack("<I", np.float32(x).tobytes())[0]
    return (u ^ 0x80000000) if not (u & 0x80000000) else (~u & 0xFFFFFFFF)


def _model_coordinate(col, b):
    """One coordinate spelled out: sorted() on (key, site), fp32 adds in sorted order."""
    W = len(col)
    order = sorted(range(W), key=lambda w: (_key(col[w]), w))
    with np.errstate(all="ignore"):
        s = np.float32(col[order[b]])
        for p in range(b + 1, W - b):
            s = np.float32(s + np.float32(col[order[p]]))
        if W - 2 * b != 1:
            s = np.float32(s * (np.float32(1) / np.float32(W - 2 * b)))
    return s, order[:b] + order[W - b:], order[b:W - b]


def _model(rows, b):
    W, n = rows.shape
    out = np.zeros(n, np.float32)
    trimmed = np.zeros(W, np.int64)
    kept_nan = np.zeros(n, bool)
    for i in range(n):
        out[i], ends, kept = _model_coordinate([rows[w, i] for w in range(W)], b)
        for w in ends:
            trimmed[w] += 1
        kept_nan[i] = any(np.isnan(rows[w, i]) for w in kept)
    return out, trimmed, kept_nan


def special_rows(W, seed=0):
    """Hand-placed special values, [W, n]: one column per case."""
    nan_p, nan_n = _from_bits([0x7FC00000])[0], _from_bits([0xFFC00001])[0]
    den_p, den_n = _from_bits([0x00000001])[0], _from_bits([0x80000003])[0]
    specials = [np.float32(0.0), np.float32(-0.0), np.float32(np.inf), np.float32(-np.inf),
                nan_p, nan_n, den_p, den_n, FLT_MAX, -FLT_MAX, np.float32(1.5), np.float32(-2.25)]
    rng = np.random.default_rng(seed + W)
    cols = []
    for v in specials:                         # all sites equal
        cols.append([v] * W)
    for v in specials:                         # one special value among ordinary ones, each site
        for w in range(min(W, 3)):
            c = list(rng.standard_normal(W).astype(np.float32))
            c[(w * 5) % W] = v
            cols.append(c)
    for _ in range(12):                        # special values only, with repeats across sites
        cols.append([specials[j] for j in rng.integers(0, len(specials), W)])
    cols.append([FLT_MAX if w % 2 == 0 else FLT_MAX for w in range(W)])      # the sum overflows
    cols.append([FLT_MAX if w < W // 2 + 1 else -FLT_MAX for w in range(W)])
    cols.append([np.float32(0.0) if w % 2 else np.float32(-0.0) for w in range(W)])
    cols.append([den_p if w % 3 else den_n for w in range(W)])
    cols.append([np.float32(w % 2) for w in range(W)])                       # duplicates
    cols.append([np.float32(7.0)] * (W - 1) + [nan_p])
    cols.append([nan_n] + [np.float32(7.0)] * (W - 1))
    return np.ascontiguousarray(np.array(cols, dtype=np.float32).T)


def _same(got, want, nan_ok, what):
    """Bits equal; where the kept range held a NaN: NaN at the same positions."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    strict = ~nan_ok
    assert np.array_equal(_bits(got)[strict], _bits(want)[strict]), what


@pytest.mark.parametrize("W", WS)
def test_mirror_equals_the_sorted_model(W):
    rows = special_rows(W)
    for b in range((W + 1) // 2):
        out, trimmed = ref.trimmed_mean(rows, b)
        assert out.dtype == np.float32 and trimmed.dtype == np.int64
        mo, mt, kept_nan = _model(rows, b)
        _same(out, mo, kept_nan, (W, b))
        assert np.array_equal(trimmed, mt), (W, b)
        assert trimmed.sum() == 2 * b * rows.shape[1]


def test_mirror_order_and_consequences():
    nan = np.float32(np.nan)
    rows = np.array([[1.0, nan, -0.0, 3.0], [2.0, 5.0, 0.0, 3.0], [9.0, 4.0, 0.0, 3.0]], np.float32)
    out, trimmed = ref.trimmed_mean(rows, 1)                  # the median of three
    assert list(out[:2]) == [2.0, 5.0] and _bits(out)[2] == 0 and out[3] == 3.0
    # column 2: -0 (site 0) < +0 (site 1) < +0 (site 2); column 3: ties go by site index
    # and the NaN of column 1 sits last, so site 1 is never at an end
    assert list(trimmed) == [4, 0, 4]
    assert np.isnan(ref.trimmed_mean(rows, 0)[0][1])          # b = 0 is a mean: the NaN gets in
    neg_nan = _from_bits([0xFFC00000])[0]
    o, t = ref.trimmed_mean(np.array([[neg_nan], [1.0], [2.0], [nan]], np.float32), 1)
    assert o[0] == 1.5 and list(t) == [1, 0, 0, 1]            # -NaN first, +NaN last; even W
    one = np.array([[nan, 1.0, -0.0]], np.float32)
    o, t = ref.trimmed_mean(one, 0)                           # W = 1: the identity
    assert np.array_equal(_bits(o), _bits(one[0])) and list(t) == [0]
    assert ref.trimmed_b(3) == 1 and ref.trimmed_b(4) == 1 and ref.trimmed_b(16) == 7
    assert ref.trimmed_b(1) == 0 and ref.trimmed_b(5, 2) == 2
    for W, b in ((1, 1), (2, 1), (4, 2), (3, -1)):
        with pytest.raises(ValueError, match="2b"):
            ref.trimmed_mean(np.zeros((W, 3), np.float32), b)


@pytest.mark.parametrize("W", WS)
def test_torch_cpu_path_matches_the_mirror(W):
    from dinunet_implementations_amd.ops import TrimmedState
    rows = special_rows(W, seed=1)
    n = rows.shape[1]
    for b in range((W + 1) // 2):
        st = TrimmedState("cpu", n, W, b)
        buf = st.gather_buffer()
        assert buf.shape == (W, -(-n // 4) * 4)
        buf.fill_(float("nan"))
        buf[:, :n].copy_(torch.from_numpy(rows))
        out = torch.full((n,), 7.0)
        st.combine(buf, out)
        want, trimmed = ref.trimmed_mean(rows, b)
        kept_nan = _model(rows, b)[2]
        _same(out.numpy(), want, kept_nan, (W, b))
        assert st.counts().dtype == torch.int64 and list(st.counts()) == list(trimmed)
        st.combine(buf, out)                                   # cumulative
        assert list(st.counts()) == list(2 * trimmed)


def test_state_errors():
    from dinunet_implementations_amd.ops import TrimmedState
    for W, b in ((0, 0), (17, 0), (2, 1), (3, 2), (3, -1)):
        with pytest.raises(ValueError, match="trimmed mean"):
            TrimmedState("cpu", 8, W, b)
    with pytest.raises(ValueError, match="elements"):
        TrimmedState("cpu", 0, 3, 1)
    st = TrimmedState("cpu", 6, 3, 1)
    rows, out = st.gather_buffer(), torch.zeros(6)
    for bad_rows, bad_out in ((rows.double(), out), (rows[:2], out), (rows, out.double()),
                              (rows, torch.zeros(7)), (rows[:, :5], out),
                              (torch.zeros(3, 7)[:, :6], out), (rows.t().contiguous().t(), out)):
        with pytest.raises(ValueError, match="TrimmedState.combine"):
            st.combine(bad_rows, bad_out)
    with pytest.raises(ValueError, match="counters"):
        st.load_state_dict({"trimmed": torch.zeros(4, dtype=torch.int64)})


# ---- the engine across gloo processes ------------------------------------------------------------
def _model_nn():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(12, 8), nn.ReLU(), nn.Linear(8, 6), nn.ReLU(), nn.Linear(6, 3))


def _data(rank, n=10):
    g = torch.Generator().manual_seed(100 + rank)
    return torch.randn(n, 12, generator=g), torch.randint(0, 3, (n,), generator=g)


def _fresh(rank=0):
    from dinunet_implementations_amd.ops import FlatParams
    m = _model_nn()
    flat = FlatParams(m.parameters())
    x, y = _data(rank)
    flat.zero_grad()
    nn.functional.cross_entropy(m(x), y).backward()
    return m, flat


BAD_RANK = 1


def _spoil(grad, rank, step):
    """Step 1: rank 1's gradient is all NaN; step 2: scaled by 1e30."""
    if rank == BAD_RANK and step == 1:
        grad.fill_(float("nan"))
    if rank == BAD_RANK and step == 2:
        grad.mul_(1e30)


def w_engine(grp, name, cfg, steps):
    """``steps`` reductions of fresh local gradients; returns ([(local, reduced, scale)], ...)."""
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    m = _model_nn()
    flat = FlatParams(m.parameters())
    eng = make_engine(name, m, flat, grp, cfg)
    out, counts = [], []
    for s in range(steps):
        x, y = _data(grp.rank + 10 * s)
        flat.zero_grad()
        nn.functional.cross_entropy(m(x), y).backward()
        _spoil(flat.grad, grp.rank, s)
        local = flat.grad.clone()
        scale = eng.reduce()
        out.append((local, flat.grad.clone(), scale))
        if name == "trimmedMean":
            counts.append(eng.state.counts())
    extra = (eng.b, eng.comm_bytes, eng.capturable, eng.trimmed_share()) \
        if name == "trimmedMean" else None
    return out, counts, extra


def test_three_ranks_keep_a_nan_site_and_a_blown_up_site_out():
    world, steps = 3, 3
    outs = run_world(w_engine, world, "trimmedMean", {"trim_sites": 1}, steps)
    n = outs[0][0][0][0].numel()
    b, comm, capturable, share = outs[0][2]
    assert b == 1 and comm == 4 * n and capturable is False
    total = np.zeros(world, np.int64)
    for s in range(steps):
        rows = np.stack([outs[r][0][s][0].numpy() for r in range(world)])
        want, trimmed = ref.trimmed_mean(rows, 1)
        total += trimmed
        if s == 1:
            assert np.isnan(rows[BAD_RANK]).all() and trimmed[BAD_RANK] == n
        if s == 2:  # blown up by 1e30: at an end wherever its gradient is not (almost) zero
            huge = int((np.abs(rows[BAD_RANK]) > 1e20).sum())
            assert huge > n // 4 and trimmed[BAD_RANK] >= huge
        for r in range(world):
            local, reduced, scale = outs[r][0][s]
            assert scale == 1.0
            assert bool(torch.isfinite(reduced).all()), (s, r)
            assert torch.equal(reduced, outs[0][0][s][1])  # identical across ranks
            assert np.array_equal(_bits(reduced.numpy()), _bits(want)), (s, r)
            assert list(outs[r][1][s]) == list(total), (s, r)  # the counters blame rank 1
        if s == 2:
            assert float(np.abs(want).max()) < 1e3
    assert share == pytest.approx([float(c) / (n * steps) for c in total])
    # the same NaN step through dSGD reaches every site's update: the point of the feature
    dense = run_world(w_engine, world, "dSGD", {}, 2)
    for r in range(world):
        _, reduced, scale = dense[r][0][1]
        assert not bool(torch.isfinite(reduced * scale).any())


def test_default_is_the_median_and_zero_is_a_value_ordered_mean():
    outs = run_world(w_engine, 3, "trimmedMean", {}, 1)
    rows = np.stack([outs[r][0][0][0].numpy() for r in range(3)])
    assert outs[0][2][0] == 1
    assert np.array_equal(_bits(outs[2][0][0][1].numpy()), _bits(np.sort(rows, axis=0)[1]))
    outs = run_world(w_engine, 2, "trimmedMean", {"trim_sites": 0}, 1)
    rows = np.stack([outs[r][0][0][0].numpy() for r in range(2)])
    assert outs[0][2][0] == 0 and not outs[0][1][0].any()
    assert np.array_equal(_bits(outs[1][0][0][1].numpy()), _bits(ref.trimmed_mean(rows, 0)[0]))
    np.testing.assert_allclose(outs[0][0][0][1].numpy(), rows.mean(0), rtol=1e-6, atol=1e-7)


def test_config():
    from dinunet_implementations_amd.config import FRAMEWORK_DEFAULTS, generate_compspec, validate
    from dinunet_implementations_amd.parallel import ENGINES
    assert FRAMEWORK_DEFAULTS["trim_sites"] == "median"
    assert ENGINES["trimmedMean"].name == "trimmedMean"
    cfg = validate(dict(FRAMEWORK_DEFAULTS, agg_engine="trimmedMean"))
    assert cfg["agg_engine"] == "trimmedMean" and cfg["trim_sites"] == "median"
    for ok in ("median", 0, 2):
        assert validate(dict(FRAMEWORK_DEFAULTS, trim_sites=ok))["trim_sites"] == ok
    for bad in (-1, 1.5, True, "mean"):
        with pytest.raises(ValueError, match="trim_sites"):
            validate(dict(FRAMEWORK_DEFAULTS, trim_sites=bad))
    # ignored by the other engines, as topk_ratio is
    assert validate(dict(FRAMEWORK_DEFAULTS, agg_engine="dSGD", trim_sites=3))["trim_sites"] == 3
    inputs = generate_compspec()["computation"]["input"]
    assert "trimmedMean" in inputs["agg_engine"]["values"] and "trim_sites" not in inputs
    import json
    import os
    import dinunet_implementations_amd.config as C
    with open(os.path.join(os.path.dirname(C.__file__), "compspec.json")) as f:
        assert json.load(f) == generate_compspec()  # the committed file is the generated one


def test_engine_refusals():
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    m, flat = _fresh()
    for cfg in ({"precision_bits": "16"}, {"payload_dtype": "bf16"}):
        with pytest.raises(ValueError, match="trimmedMean.*fp32"):
            make_engine("trimmedMean", m, flat, SiteGroup(), cfg)
    with pytest.raises(ValueError, match="dp_clip_norm.*dense gradient"):
        make_engine("trimmedMean", m, flat, SiteGroup(), {"dp_clip_norm": 1.0})
    with pytest.raises(ValueError, match="secure_agg.*dense gradient"):
        make_engine("trimmedMean", m, flat, SiteGroup(), {"secure_agg": True})
    for world, trim in ((3, 2), (2, 1), (4, 2)):  # 2b >= W: both numbers are named
        with pytest.raises(ValueError, match=rf"trim_sites = {trim}.*W = {world}"):
            make_engine("trimmedMean", m, flat, SiteGroup(rank=0, world=world),
                        {"trim_sites": trim})
    with pytest.raises(ValueError, match="GPUs per site"):
        make_engine("trimmedMean", m, flat, SiteGroup(rank=0, world=4, replicas=2), {})
    for bad in (-1, 1.5, True, "mean"):
        with pytest.raises(ValueError, match="trim_sites"):
            make_engine("trimmedMean", m, flat, SiteGroup(), {"trim_sites": bad})
    eng = make_engine("trimmedMean", m, flat, SiteGroup(rank=0, world=4), {})
    assert eng.b == 1 and not eng.supports_dp and not eng.supports_secure_agg
    assert not hasattr(eng, "pre_reduce")


def test_one_site_leaves_the_gradient_alone():
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    m, flat = _fresh()
    flat.grad[3] = float("nan")
    flat.grad[5] = -0.0
    local = flat.grad.clone()
    eng = make_engine("trimmedMean", m, flat, SiteGroup(), {})
    assert eng.capturable and eng.reduce() == 1.0 and eng.last_scale == 1.0
    assert torch.equal(flat.grad.view(torch.int32), local.view(torch.int32))
    assert eng.comm_bytes == 4 * local.numel() and not eng.state.counts().any()


def test_file_transport_equals_collective_path():
    from dinunet_implementations_amd.parallel import TrimmedMeanEngine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    world, cfg = 3, {"trim_sites": 1}
    coll = run_world(w_engine, world, "trimmedMean", cfg, 2)
    sites = []
    for r in range(world):
        m, flat = _fresh(r)
        sites.append((m, flat, TrimmedMeanEngine(m, flat, SiteGroup(), cfg)))
    total = torch.zeros(world, dtype=torch.int64)
    for s in range(2):
        for r, (m, flat, _) in enumerate(sites):
            x, y = _data(r + 10 * s)
            flat.zero_grad()
            nn.functional.cross_entropy(m(x), y).backward()
            _spoil(flat.grad, r, s)
        pays = [eng.payload() for _, _, eng in sites]
        assert set(pays[0]) == {"grad", "n"} and pays[0]["grad"].dtype == torch.float32
        agg = TrimmedMeanEngine.aggregate(pays, cfg)
        total += agg["trimmed"]
        assert list(total) == list(coll[0][1][s])
        for r, (_, flat, eng) in enumerate(sites):
            assert eng.apply({k_: v.clone() for k_, v in agg.items()}) == 1.0
            assert np.array_equal(_bits(flat.grad.numpy()), _bits(coll[r][0][s][1].numpy())), (s, r)
    with pytest.raises(ValueError, match="trim_sites = 1.*W = 2"):
        TrimmedMeanEngine.aggregate(pays[:2], cfg)


def test_counters_survive_a_state_dict_round_trip():
    from dinunet_implementations_amd.ops import TrimmedState
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    rows = special_rows(3)
    n = rows.shape[1]
    a = TrimmedState("cpu", n, 3, 1)
    buf = a.gather_buffer()
    buf[:, :n].copy_(torch.from_numpy(rows))
    out = torch.zeros(n)
    a.combine(buf, out)
    sd = a.state_dict()
    assert set(sd) == {"trimmed"} and sd["trimmed"].sum() == 2 * n
    m, flat = _fresh()
    grp = SiteGroup(rank=0, world=3)
    e1 = make_engine("trimmedMean", m, flat, grp, {})
    e1.load_state_dict({"trimmed": sd["trimmed"].clone()})
    assert torch.equal(e1.state_dict()["trimmed"], sd["trimmed"])
    assert e1.trimmed_share() == [0.0, 0.0, 0.0]  # nothing new since the checkpoint
    b = TrimmedState("cpu", n, 3, 1)
    b.load_state_dict(e1.state_dict())
    b.gather_buffer()[:, :n].copy_(torch.from_numpy(rows))
    a.combine(buf, out)
    b.combine(b.gather_buffer(), out)
    assert torch.equal(a.counts(), b.counts()) and torch.equal(a.counts(), 2 * sd["trimmed"])


# ---- through the runtimes ------------------------------------------------------------------------
def test_simulator_three_sites_end_to_end(fs_data_root, tmp_path):
    import json
    import os
    from dinunet_implementations_amd.compat.nodes import LocalNode, RemoteNode
    from dinunet_implementations_amd.compat.simulator import simulate
    from dinunet_implementations_amd.config import load_inputspec
    specs = load_inputspec(os.path.join(fs_data_root, "inputspec.json"))[:3]
    it, locs, rem = simulate(fs_data_root, str(tmp_path), lambda: LocalNode(device="cpu"),
                             RemoteNode, site_inputs=specs,
                             overrides={"epochs": 2, "agg_engine": "trimmedMean"})
    assert len(locs) == 3
    ws = [locs[s].trainer.flat.data for s in sorted(locs)]
    assert all(torch.equal(w, ws[0]) for w in ws)
    r = json.load(open(os.path.join(str(tmp_path), "output", "remote", "simulatorRun",
                                    "FS-Classification", "fold_0", "logs.json")))
    assert r["agg_engine"] == "trimmedMean" and len(r["test_metrics"]) == 6
    share = r["trimmed_share"]
    assert len(share) == 2 and all(len(row) == 3 for row in share)  # per epoch, per site
    for row in share:  # the median of three drops two of three sites at every coordinate
        assert sum(row) == pytest.approx(2.0, abs=1e-4) and all(0 <= v <= 1 for v in row)


def test_site_run_logs_the_trimmed_share(fs_data_root, tmp_path):
    from test_resume import _logs
    from test_runtime_e2e import w_site
    a = str(tmp_path / "a")
    run_world(w_site, 3, fs_data_root, a,
              {"patience": 100, "seed": 3, "agg_engine": "trimmedMean", "epochs": 2})
    for site in ("local0", "local1", "remote"):
        la = _logs(a, site, "FS-Classification")
        assert la["agg_engine"] == "trimmedMean"
        share = la["trimmed_share"]
        assert len(share) == 2 and all(len(row) == 3 for row in share)
        for row in share:
            assert sum(row) == pytest.approx(2.0, abs=1e-4)
