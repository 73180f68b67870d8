"""Top-k sparsified gradient engine (``agg_engine: topK``) on the CPU: the numpy mirror against a
brute-force stable sort, the exact invariants of the error feedback, the engine across 2-3 gloo
processes against the mirror (bit for bit), the file transport, resume state and configuration.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from mp_util import run_world

from dinunet_implementations_amd.ops import reference as ref


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _brute(g, err, k):
    """The contract spelled out: sort (-(bits & 0x7fffffff), i), take k, ascending index."""
    acc = np.asarray(g, np.float32) + np.asarray(err, np.float32)
    key = [int(b) & 0x7FFFFFFF for b in _bits(acc)]
    order = sorted(range(acc.size), key=lambda i: (-key[i], i))
    idx = np.array(sorted(order[:k]), dtype=np.int32)
    err_new = acc.copy()
    err_new[idx] = 0.0
    return idx, acc[idx], err_new


def _cases():
    rng = np.random.default_rng(0)
    n = 301
    return {"random": rng.standard_normal(n).astype(np.float32),
            "ties": rng.choice(np.array([0, 1, -1, 2, -2], np.float32), n),
            "zeros": np.zeros(n, np.float32)}


@pytest.mark.parametrize("case", ["random", "ties", "zeros"])
def test_mirror_equals_brute_force(case):
    g = _cases()[case]
    err = np.zeros_like(g)
    for k in (1, 2, g.size // 3, g.size - 1, g.size):
        idx, val, err_new = ref.topk_select(g, err, k)
        bi, bv, be = _brute(g, err, k)
        assert idx.dtype == np.int32 and np.array_equal(idx, bi), (case, k)
        assert np.array_equal(_bits(val), _bits(bv)), (case, k)
        assert np.array_equal(_bits(err_new), _bits(be)), (case, k)


def test_mirror_order_of_special_values():
    g = np.array([1.0, -np.inf, 0.0, np.nan, -0.0, 3.0e38, -1.0], np.float32)
    z = np.zeros_like(g)
    z[4] = -0.0  # (-0 + -0 = -0: the accumulator keeps the sign only then)
    assert list(ref.topk_select(g, z, 1)[0]) == [3]          # NaN first
    assert list(ref.topk_select(g, z, 2)[0]) == [1, 3]       # then inf
    assert list(ref.topk_select(g, z, 4)[0]) == [0, 1, 3, 5]  # |1| ties: the lower index
    idx, _, err = ref.topk_select(g, z, 6)
    assert list(idx) == [0, 1, 2, 3, 5, 6]                   # +0 (2) before -0 (4)
    assert _bits(err)[4] == 0x80000000 and not _bits(err)[idx].any()
    assert ref.topk_k(1000, 0.01) == 10 and ref.topk_k(1001, 0.01) == 11
    assert ref.topk_k(5, 1e-9) == 1 and ref.topk_k(5, 1.0) == 5


def test_sent_and_residual_partition_the_accumulator():
    rng = np.random.default_rng(1)
    g, err = (rng.standard_normal(500).astype(np.float32) for _ in range(2))
    idx, val, err_new = ref.topk_select(g, err, 37)
    sent = ref.topk_combine([(idx, val)], g.size)
    assert not ((sent != 0) & (err_new != 0)).any()  # disjoint support
    assert np.array_equal(sent + err_new, g + err)


def test_error_feedback_conserves_integer_gradients():
    rng = np.random.default_rng(2)
    n, k = 400, 9
    err = np.zeros(n, np.float32)
    total_sent = np.zeros(n, np.float32)
    total_g = np.zeros(n, np.float32)
    for _ in range(5):
        g = rng.integers(-50, 51, n).astype(np.float32)
        idx, val, err = ref.topk_select(g, err, k)
        total_sent += ref.topk_combine([(idx, val)], n)
        total_g += g
    assert np.array_equal(total_sent + err, total_g)


def test_combine_sums_in_rank_order():
    a = (np.array([0, 2], np.int32), np.array([1e8, -0.0], np.float32))
    b = (np.array([0, 3], np.int32), np.array([1.0, 5.0], np.float32))
    c = (np.array([0, 2], np.int32), np.array([-1e8, -0.0], np.float32))
    out = ref.topk_combine([a, b, c], 5)
    assert out[0] == np.float32(np.float32(np.float32(0 + 1e8) + 1.0) - 1e8)  # == 0, not 1
    assert _bits(out)[2] == 0 and _bits(out)[1] == 0 and out[3] == 5.0  # (+0 + -0) + -0 = +0


# ---- the engine across gloo processes ------------------------------------------------------------
def _model():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(12, 8), nn.ReLU(), nn.Linear(8, 6), nn.ReLU(), nn.Linear(6, 3))


def _data(rank, n=10):
    g = torch.Generator().manual_seed(100 + rank)
    return torch.randn(n, 12, generator=g), torch.randint(0, 3, (n,), generator=g)


def _local_grad(rank, seed_off=0):
    from dinunet_implementations_amd.ops import FlatParams
    m = _model()
    flat = FlatParams(m.parameters())
    x, y = _data(rank + seed_off)
    flat.zero_grad()
    nn.functional.cross_entropy(m(x), y).backward()
    return m, flat


def w_topk(grp, cfg, steps):
    """``steps`` reductions of fresh local gradients; returns [(local, reduced, scale)]."""
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    m = _model()
    flat = FlatParams(m.parameters())
    eng = make_engine("topK", m, flat, grp, cfg)
    out = []
    for s in range(steps):
        x, y = _data(grp.rank + 10 * s)
        flat.zero_grad()
        nn.functional.cross_entropy(m(x), y).backward()
        local = flat.grad.clone()
        scale = eng.reduce()
        out.append((local, flat.grad.clone(), scale))
    return out, eng.k, eng.comm_bytes, eng.state_dict()["err"]


def w_dsgd(grp):
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    m = _model()
    flat = FlatParams(m.parameters())
    eng = make_engine("dSGD", m, flat, grp, {})
    x, y = _data(grp.rank)
    flat.zero_grad()
    nn.functional.cross_entropy(m(x), y).backward()
    return (flat.grad * eng.reduce()).clone()


@pytest.mark.parametrize("world", [2, 3])
def test_engine_matches_mirror_bit_for_bit(world):
    steps = 3
    outs = run_world(w_topk, world, {"topk_ratio": 0.1}, steps)
    k = outs[0][1]
    n = outs[0][0][0][0].numel()
    assert k == ref.topk_k(n, 0.1) and outs[0][2] == 8 * k
    errs = [np.zeros(n, np.float32) for _ in range(world)]
    for s in range(steps):
        pairs = []
        for r in range(world):
            idx, val, errs[r] = ref.topk_select(outs[r][0][s][0], errs[r], k)
            pairs.append((idx, val))
        want = ref.topk_combine(pairs, n)
        for r in range(world):
            local, reduced, scale = outs[r][0][s]
            assert torch.equal(reduced, outs[0][0][s][1])  # replicas
            assert np.array_equal(_bits(reduced.numpy()), _bits(want)), (s, r)
            assert scale == 1.0 / world
    for r in range(world):  # the residual the engine would checkpoint
        assert np.array_equal(_bits(outs[r][3].numpy()), _bits(errs[r]))


def test_ratio_one_equals_dsgd():
    world = 2
    outs = run_world(w_topk, world, {"topk_ratio": 1}, 1)
    dense = run_world(w_dsgd, world)[0]
    _, reduced, scale = outs[0][0][0]
    assert torch.allclose(reduced * scale, dense, atol=1e-6)


def test_file_transport_equals_collective_path():
    from dinunet_implementations_amd.parallel import TopKEngine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    world, cfg = 3, {"topk_ratio": 0.1}
    coll = run_world(w_topk, world, cfg, 2)
    sites = []
    for r in range(world):
        m, flat = _local_grad(r)
        sites.append((m, flat, TopKEngine(m, flat, SiteGroup(), cfg)))
    for s in range(2):
        if s:
            for r, (m, flat, _) in enumerate(sites):
                x, y = _data(r + 10 * s)
                flat.zero_grad()
                nn.functional.cross_entropy(m(x), y).backward()
        pays = [eng.payload() for _, _, eng in sites]
        assert set(pays[0]) == {"idx", "val", "n"} and pays[0]["idx"].dtype == torch.int32
        agg = TopKEngine.aggregate(pays, cfg)
        idx = agg["idx"].long()
        assert bool((idx[1:] > idx[:-1]).all()) and idx.numel() <= world * sites[0][2].k
        for r, (_, flat, eng) in enumerate(sites):
            scale = eng.apply({k_: v.clone() for k_, v in agg.items()})
            assert scale == 1.0 / world
            assert np.array_equal(_bits(flat.grad.numpy()), _bits(coll[r][0][s][1].numpy())), (s, r)


def test_state_dict_round_trip_continues_the_same_releases():
    from dinunet_implementations_amd.parallel import TopKEngine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    cfg = {"topk_ratio": 0.05}
    m, flat = _local_grad(0)
    a = TopKEngine(m, flat, SiteGroup(), cfg)
    a.reduce()
    sd = a.state_dict()
    assert set(sd) == {"err"} and sd["err"].abs().sum() > 0
    m2, flat2 = _local_grad(0, seed_off=7)
    b = TopKEngine(m2, flat2, SiteGroup(), cfg)
    b.load_state_dict({"err": sd["err"].clone()})
    flat.grad.copy_(flat2.grad)  # the same fresh gradient on both
    a.reduce(), b.reduce()
    assert torch.equal(flat.grad, flat2.grad)
    assert torch.equal(a.state_dict()["err"], b.state_dict()["err"])


def test_one_site_sparsifies_and_keeps_the_residual():
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    m, flat = _local_grad(0)
    local = flat.grad.clone()
    eng = make_engine("topK", m, flat, SiteGroup(), {"topk_ratio": 0.1})
    assert eng.capturable and eng.reduce() == 1.0
    assert int((flat.grad != 0).sum()) <= eng.k < local.numel()
    assert torch.equal(flat.grad + eng.state.err, local)


def test_config_and_refusals():
    from dinunet_implementations_amd.config import FRAMEWORK_DEFAULTS, generate_compspec, validate
    from dinunet_implementations_amd.parallel import ENGINES, make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    assert FRAMEWORK_DEFAULTS["topk_ratio"] == 0.01 and ENGINES["topK"].name == "topK"
    cfg = validate(dict(FRAMEWORK_DEFAULTS, agg_engine="topK"))
    assert cfg["agg_engine"] == "topK" and cfg["topk_ratio"] == 0.01
    inputs = generate_compspec()["computation"]["input"]
    assert "topK" in inputs["agg_engine"]["values"] and "topk_ratio" not in inputs
    for bad in (0, -0.1, 1.5, float("nan"), "0.1", True):
        with pytest.raises(ValueError, match="topk_ratio"):
            validate(dict(FRAMEWORK_DEFAULTS, topk_ratio=bad))
    m, flat = _local_grad(0)
    for bad in (0, 2, float("inf")):
        with pytest.raises(ValueError, match="topk_ratio"):
            make_engine("topK", m, flat, SiteGroup(), {"topk_ratio": bad})
    for cfg in ({"precision_bits": "16"}, {"payload_dtype": "bf16"}):
        with pytest.raises(ValueError, match="topK"):
            make_engine("topK", m, flat, SiteGroup(), cfg)
    with pytest.raises(ValueError, match="dp_clip_norm.*pairs"):
        make_engine("topK", m, flat, SiteGroup(), {"dp_clip_norm": 1.0})
    with pytest.raises(ValueError, match="secure_agg.*pairs"):
        make_engine("topK", m, flat, SiteGroup(), {"secure_agg": True})
    with pytest.raises(ValueError, match="shares factors"):
        make_engine("powerSGD", m, flat, SiteGroup(), {"secure_agg": True})


# ---- through the runtimes ------------------------------------------------------------------------
def test_simulator_file_transport_keeps_replicas_identical(fs_data_root, tmp_path):
    import json
    import os
    from dinunet_implementations_amd.compat.nodes import LocalNode, RemoteNode
    from dinunet_implementations_amd.compat.simulator import simulate
    it, locs, rem = simulate(fs_data_root, str(tmp_path), lambda: LocalNode(device="cpu"),
                             RemoteNode, overrides={"epochs": 2, "agg_engine": "topK",
                                                    "topk_ratio": 0.05})
    ws = [locs[s].trainer.flat.data for s in sorted(locs)]
    assert all(torch.equal(w, ws[0]) for w in ws)
    assert any(bool(locs[s].engine.state.err.any()) for s in locs)  # the residual is kept
    r = json.load(open(os.path.join(str(tmp_path), "output", "remote", "simulatorRun",
                                    "FS-Classification", "fold_0", "logs.json")))
    assert r["agg_engine"] == "topK" and len(r["test_metrics"]) == 6


def test_site_run_logs_and_resumes_bit_for_bit(fs_data_root, tmp_path):
    from test_resume import _check_same, _logs
    from test_runtime_e2e import w_site
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    base = {"patience": 100, "seed": 3, "agg_engine": "topK", "topk_ratio": 0.05}
    run_world(w_site, 2, fs_data_root, a, dict(base, epochs=4))
    run_world(w_site, 2, fs_data_root, b, dict(base, epochs=2))
    run_world(w_site, 2, fs_data_root, b, dict(base, epochs=4, resume=True))
    _check_same(a, b, "FS-Classification")
    la = _logs(a, "local0", "FS-Classification")
    assert la["topk_ratio"] == 0.05 and la["topk_k"] >= 1
    assert la["topk_exchange"].startswith("all-gather")
