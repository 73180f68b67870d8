"""Secure aggregation on the CPU: the ChaCha20 mirror, the X25519 key agreement, mask cancellation,
the fixed-point edges, the device block's host mirror and the dSGD engine over gloo."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn

from mp_util import run_world

OPENSSL = shutil.which("openssl")


def tkey(i, j, tag=b"k"):
    """The fixed test key of the pair {i, j}."""
    a, b = min(i, j), max(i, j)
    return hashlib.sha256(b"secagg-test-" + tag + bytes([a, b])).digest()


def tkeys(W, rank):
    return [None if j == rank else tkey(rank, j) for j in range(W)]


# ---- generator mirror ---------------------------------------------------------------------------
VECTORS = [
    (bytes(32), (0, 0, 0, 0),
     "76b8e0ada0f13d90405d6ae55386bd28bdd219b8a08ded1aa836efcc8b770dc7"
     "da41597c5157488d7724e03fb8d84a376a43b8f41518a11cc387b669b2ee6586"),
    (bytes(range(32)), (1, 0x09000000, 0x4A000000, 0),
     "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
     "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e"),
]


@pytest.mark.parametrize("key,words,want", VECTORS)
def test_chacha_known_answers(key, words, want):
    from dinunet_implementations_amd.ops import reference
    out = reference.chacha20_blocks(key, [words[0]], *words[1:])
    assert out.shape == (1, 16) and out.dtype == np.uint32
    assert out.astype("<u4").tobytes().hex() == want


@pytest.mark.skipif(OPENSSL is None, reason="no openssl binary on PATH")
def test_chacha_matches_openssl():
    from dinunet_implementations_amd.ops import reference
    rng = np.random.default_rng(7)
    for _ in range(3):
        key = rng.bytes(32)
        words = [int(w) for w in rng.integers(0, 2 ** 32 - 4, 4, dtype=np.uint64)]
        iv = b"".join(int(w).to_bytes(4, "little") for w in words)
        r = subprocess.run([OPENSSL, "enc", "-chacha20", "-K", key.hex(), "-iv", iv.hex()],
                           input=bytes(192), capture_output=True, check=True)
        out = reference.chacha20_blocks(key, [words[0] + b for b in range(3)], *words[1:])
        assert out.astype("<u4").tobytes() == r.stdout


def test_prg_layout():
    from dinunet_implementations_amd.ops import reference
    key, t, dom = tkey(0, 1), (5 << 32) + 9, reference.secagg_domain(3, 1)
    assert dom == 3 * 4096 + 2048
    for n in (4, 8, 12, 2052):
        m = reference.secagg_prg(key, n, t, dom)
        nb = -(-n // 8)
        blocks = reference.chacha20_blocks(key, np.arange(nb + 1), 9, 5, dom)
        words = blocks.astype("<u4").view("<u8").reshape(nb + 1, 8)
        assert m.dtype == np.uint64 and m.size == n + 8
        assert np.array_equal(m[:n], words[:nb].reshape(-1)[:n])
        assert np.array_equal(m[n:], words[nb])  # the tail block is b = ceil(n / 8), at word n


# ---- key agreement ------------------------------------------------------------------------------
def test_x25519_rfc7748_vectors():
    from dinunet_implementations_amd.parallel import secagg
    k = bytes.fromhex("a546e36bf0527c9d3b16154b82465edd62144c0ac1fc5a18506a2244ba449ac4")
    u = bytes.fromhex("e6db6867583030db3594c1a424b15f7c726624ec26b3353b10a903a6d0ab1c4c")
    assert secagg.x25519(k, u).hex() == \
        "c3da55379de9c6908e94ea4df28d084f32eccf03491c71f754b4075577a28552"
    a = bytes.fromhex("77076d0a7318a57d3c16c17251b26645df4c2f87ebc0992ab177fba51db92c2a")
    b = bytes.fromhex("5dab087e624a8a4b79e17f8b83800ee66f3bb1292618b6fd1c2f8b27ff88e0eb")
    _, A = secagg.keypair(a)
    _, B = secagg.keypair(b)
    assert A.hex() == "8520f0098930a754748b7ddcb43ef75a0dbf3a0d26381af4eba4a98eaa9b4e6a"
    assert secagg.x25519(a, B) == secagg.x25519(b, A)
    assert secagg.x25519(a, B).hex() == \
        "4a5d9d5ba4ce2de1728e3bf480350f25e07e21c947d19e3376f09b3c1e161742"


def test_pair_keys_agree_and_differ():
    from dinunet_implementations_amd.parallel import secagg
    pairs = [secagg.keypair(hashlib.sha256(b"sk%d" % i).digest()) for i in range(4)]
    pubs = [p for _, p in pairs]
    tables = [secagg.derive_keys(sk, pubs, r, 2, 0) for r, (sk, _) in enumerate(pairs)]
    seen = set()
    for i in range(4):
        assert tables[i][i] is None
        for j in range(i + 1, 4):
            assert tables[i][j] == tables[j][i] and len(tables[i][j]) == 32  # both ends alike
            seen.add(tables[i][j])
    assert len(seen) == 6  # distinct pairs, distinct keys
    other_fold = secagg.derive_keys(pairs[0][0], pubs, 0, 3, 0)
    other_phase = secagg.derive_keys(pairs[0][0], pubs, 0, 2, 1)
    for j in range(1, 4):
        assert len({tables[0][j], other_fold[j], other_phase[j]}) == 3
    # the derivation as documented
    shared = secagg.x25519(pairs[0][0], pubs[1])
    lo, hi = sorted([pubs[0], pubs[1]])
    want = hashlib.sha256(b"dinunet-secagg-v1" + lo + hi + shared + (2).to_bytes(4, "little")
                          + (0).to_bytes(4, "little")).digest()
    assert tables[0][1] == want
    # fresh ephemeral pairs differ
    assert secagg.keypair()[0] != secagg.keypair()[0]
    with pytest.raises(ValueError):
        secagg.derive_keys(pairs[0][0], [pubs[0], pubs[0]], 0, 0, 0)


@pytest.mark.skipif(OPENSSL is None, reason="no openssl binary on PATH")
def test_shared_secret_matches_openssl(tmp_path):
    from dinunet_implementations_amd.parallel import secagg
    a, A = secagg.keypair(hashlib.sha256(b"openssl-a").digest())
    b, B = secagg.keypair(hashlib.sha256(b"openssl-b").digest())
    priv = tmp_path / "a.der"
    pub = tmp_path / "b.der"
    priv.write_bytes(bytes.fromhex("302e020100300506032b656e04220420") + a)  # PKCS#8, RFC 8410
    pub.write_bytes(bytes.fromhex("302a300506032b656e032100") + B)           # SubjectPublicKeyInfo
    r = subprocess.run([OPENSSL, "pkeyutl", "-derive", "-keyform", "DER", "-inkey", str(priv),
                        "-peerform", "DER", "-peerkey", str(pub)], capture_output=True)
    if r.returncode != 0:
        pytest.skip(f"this openssl cannot derive X25519: {r.stderr[-200:]!r}")
    assert r.stdout == secagg.x25519(a, B)


# ---- cancellation -------------------------------------------------------------------------------
def _grads(W, n, seed=0, scale=0.3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for _ in range(W)]


@pytest.mark.parametrize("W", [2, 3, 5, 16])
@pytest.mark.parametrize("n", [4, 8, 12, 2052])
def test_masks_cancel_in_the_sum(W, n):
    from dinunet_implementations_amd.ops import reference
    grads = _grads(W, n, seed=W * 10000 + n)
    grads[0][0] = 3e5  # one clamped element: the tail block carries a count
    dom = reference.secagg_domain(1, 0)
    with np.errstate(over="ignore"):
        wires = [reference.secagg_mask(g, tkeys(W, r), r, 3, dom) for r, g in enumerate(grads)]
        plain = [reference.secagg_quantize(g)[0] for g in grads]
        total, want = sum(wires), sum(plain)
    assert total.dtype == np.uint64 and total.size == n + 8
    assert np.array_equal(total, want)  # exact, tail block included
    assert int(want[n]) == 0 and int(want[n + 1]) == 1 and not want[n + 2:].any()
    for w, p in zip(wires, plain):
        assert not np.array_equal(w, p) and not np.array_equal(w[n:], p[n:])
    mean, sat, bad = reference.secagg_open(total, W)
    ref, _, _ = reference.secagg_mean(grads)
    assert torch.equal(mean, ref) and (sat, bad) == (1, 0)


def test_a_single_wire_looks_random():
    from dinunet_implementations_amd.ops import reference
    n = 4096 - 8
    g = _grads(1, n, seed=5)[0]
    for W, r in ((2, 0), (2, 1), (5, 2)):
        wire = reference.secagg_mask(g, tkeys(W, r), r, 1, 0)
        plain = reference.secagg_quantize(g)[0]
        x = wire ^ plain
        pop = np.unpackbits(x.view(np.uint8)).sum() / x.size
        assert x.size == 4096 and 28 <= pop <= 36
    # another release, fold or phase: other masks
    a = reference.secagg_mask(g, tkeys(2, 0), 0, 1, 0)
    for t, dom in ((2, 0), (1, reference.secagg_domain(1, 0)), (1, reference.secagg_domain(0, 1)),
                   (1 + (1 << 32), 0)):
        b = reference.secagg_mask(g, tkeys(2, 0), 0, t, dom)
        assert np.unpackbits((a ^ b).view(np.uint8)).sum() / a.size > 28


# ---- quantisation edges -------------------------------------------------------------------------
def test_quantisation_edges():
    from dinunet_implementations_amd.ops import reference
    tiny = float(np.float32(1e-45))  # the smallest denormal
    vals = [0.0, -0.0, 2.0 ** -41, -2.0 ** -41, 2.0 ** -40, -2.0 ** -40, tiny, -tiny, 1e-39,
            2.0 ** 18, -2.0 ** 18, 2.0 ** 18 + 0.0625, -3e5, 3e38, 1.0, -1.5, 0.1, 1e-7, 123.456,
            2.0 ** 18 - 2.0 ** -6]
    g = torch.tensor(vals, dtype=torch.float32)
    assert g.numel() % 4 == 0
    wire, sat, bad = reference.secagg_quantize(g)
    q = wire.view(np.int64)
    n = g.numel()
    assert list(q[:9]) == [0, 0, 0, 0, 1, -1, 0, 0, 0]  # rint: ties to even
    assert q[9] == 2 ** 58 and q[10] == -2 ** 58
    assert q[11] == 2 ** 58 and q[12] == -2 ** 58 and q[13] == 2 ** 58  # clamped ...
    assert (sat, bad) == (3, 0) and q[n] == 0 and q[n + 1] == 3         # ... and counted
    assert q[14] == 2 ** 40 and q[15] == -3 * 2 ** 39
    assert not q[n + 2:].any()
    # 16 parties at the clamp fit int64
    assert 16 * 2 ** 58 < 2 ** 63


def test_mean_is_the_formula_and_within_the_bound():
    from dinunet_implementations_amd.ops import reference
    for W in (2, 3, 16):
        grads = _grads(W, 2052, seed=W, scale=2.0)
        grads[0][:4] = torch.tensor([2.0 ** 18, -2.0 ** 18, 2.0 ** -40, 1e-30])
        for k in range(1, W):
            grads[k][:2] = torch.tensor([2.0 ** 18, -2.0 ** 18])  # the sum at its largest
        mean, sat, bad = reference.secagg_mean(grads)
        assert mean.dtype == torch.float32 and (sat, bad) == (0, 0)
        q = sum(np.rint(g.numpy().astype(np.float64) * 2.0 ** 40).astype(np.int64) for g in grads)
        want = (q.astype(np.float64) * (2.0 ** -40 / W)).astype(np.float32)
        assert np.array_equal(mean.numpy(), want)  # bit-equal to the mirror formula
        m = torch.stack(grads).double().mean(0)
        bound = 2.0 ** -41 + 2.0 ** -24 * m.abs() + 2.0 ** -52 * m.abs()
        assert bool(((mean.double() - m).abs() <= bound).all())
        assert float(mean[0]) == 2.0 ** 18 and float(mean[1]) == -2.0 ** 18


@pytest.mark.parametrize("badval", [float("nan"), float("inf"), float("-inf")])
def test_nonfinite_at_one_party_makes_every_mean_nan(badval):
    from dinunet_implementations_amd.ops import SecAggState
    W, n = 3, 12
    grads = _grads(W, n, seed=9)
    grads[1][5] = badval
    grads[2][0] = -4e5
    states = [SecAggState("cpu", W, r, tkeys(W, r), 7) for r in range(W)]
    wires = [s.mask_(g, s.wire_like(g)) for s, g in zip(states, grads)]
    total = wires[0] + wires[1] + wires[2]
    for s, g in zip(states, grads):
        out = g.clone()
        s.open_(total.clone(), out)
        assert bool(torch.isnan(out).all())
        assert (s.nonfinite, s.saturated, s.last_saturated, s.releases) == (1, 1, 1, 1)


# ---- the block's host mirror --------------------------------------------------------------------
def test_state_cpu_release_round_trip_and_no_key_bytes():
    from dinunet_implementations_amd.ops import SecAggState, reference
    W, n = 3, 20
    grads = _grads(W, n, seed=3)
    states = [SecAggState("cpu", W, r, tkeys(W, r), 4096) for r in range(W)]
    for rel in (1, 2):
        wires = [s.mask_(g, s.wire_like(g)) for s, g in zip(states, grads)]
        for r, (w, g) in enumerate(zip(wires, grads)):
            want = reference.secagg_mask(g, tkeys(W, r), r, rel, 4096)
            assert np.array_equal(w.numpy().view(np.uint64), want)
        total = wires[0] + wires[1] + wires[2]  # torch's int64 add wraps
        outs = []
        for s, g in zip(states, grads):
            o = g.clone()
            s.open_(total, o)
            outs.append(o)
        want, _, _ = reference.secagg_mean(grads)
        assert all(torch.equal(o, want) for o in outs) and states[0].releases == rel
    sd = states[0].state_dict()
    assert json.loads(json.dumps(sd)) == {"t": 2, "saturated": 0, "nonfinite": 0,
                                          "last_saturated": 0}
    blob = repr(sd).encode() + repr(vars(states[0]).keys()).encode()
    host = [v for v in vars(states[0]).values() if isinstance(v, (bytes, bytearray, list, tuple))]
    assert not host  # no host copy of a key
    for j in (1, 2):
        assert tkey(0, j) not in blob and tkey(0, j).hex().encode() not in blob
    fresh = SecAggState("cpu", W, 0, [None, tkey(0, 1, b"x"), tkey(0, 2, b"x")], 4096)
    fresh.load_state_dict(sd)
    assert fresh.releases == 2
    w = fresh.mask_(grads[0], fresh.wire_like(grads[0]))  # release 3 under the fresh keys
    want = reference.secagg_mask(grads[0], [None, tkey(0, 1, b"x"), tkey(0, 2, b"x")], 0, 3, 4096)
    assert np.array_equal(w.numpy().view(np.uint64), want)
    for bad in (dict(world=1), dict(world=17), dict(rank=3), dict(domain=2 ** 32)):
        kw = dict(world=W, rank=0, domain=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            SecAggState("cpu", kw["world"], kw["rank"], [None] + [bytes(32)] * (kw["world"] - 1),
                        kw["domain"])
    with pytest.raises(ValueError):
        SecAggState("cpu", 2, 0, [None, b"short"])
    with pytest.raises(ValueError):
        states[0].mask_(torch.zeros(6), torch.zeros(14, dtype=torch.int64))
    with pytest.raises(ValueError):
        states[0].mask_(torch.zeros(8), torch.zeros(8, dtype=torch.int64))


# ---- engines ------------------------------------------------------------------------------------
def _model(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(33, 17), nn.ReLU(), nn.Linear(17, 5))


def _engine(name, cfg, group=None):
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    from dinunet_implementations_amd.parallel.group import SiteGroup
    m = _model()
    flat = FlatParams(m.parameters())
    return m, flat, make_engine(name, m, flat, group or SiteGroup(), {"precision_bits": "32", **cfg})


def test_engine_gating(monkeypatch):
    from dinunet_implementations_amd.config import build_config
    monkeypatch.delenv("DINUNET_SECURE_AGG", raising=False)
    assert build_config()["secure_agg"] is False
    assert build_config(overrides={"secure_agg": True})["secure_agg"] is True
    with pytest.raises(ValueError, match="secure_agg"):
        build_config(overrides={"secure_agg": "yes"})
    for name in ("rankDAD", "powerSGD"):
        with pytest.raises(ValueError, match="dSGD only"):
            _engine(name, {"secure_agg": True})
        assert _engine(name, {})[2].sa is None
    with pytest.raises(ValueError, match="precision_bits"):
        _engine("dSGD", {"secure_agg": True, "precision_bits": "16"})
    with pytest.raises(ValueError, match="allreduce"):
        _engine("dSGD", {"secure_agg": True, "dsgd_collective": "allreduce"})
    from dinunet_implementations_amd.parallel.group import SiteGroup
    with pytest.raises(ValueError, match="at most 16"):  # (raised before any collective)
        _engine("dSGD", {"secure_agg": True}, SiteGroup(rank=0, world=17, backend="gloo"))
    _, _, off = _engine("dSGD", {})
    assert off.sa is None and not off.secure_agg and off.state_dict() == {}
    # one party: no masks, no quantisation, the parent's step
    _, flat, one = _engine("dSGD", {"secure_agg": True})
    g = torch.randn(flat.numel)
    flat.grad.copy_(g)
    assert one.secure_agg and one.sa is None and one.reduce() == 1.0
    assert torch.equal(flat.grad, g) and one.state_dict() == {}
    with pytest.raises(RuntimeError, match="file transport"):
        one.payload()
    # the switch applies where the key is unset
    monkeypatch.setenv("DINUNET_SECURE_AGG", "1")
    assert _engine("dSGD", {})[2].secure_agg
    with pytest.raises(ValueError, match="dSGD only"):
        _engine("powerSGD", {})


def test_coinstac_phase_machines_refuse(fs_data_root, tmp_path, monkeypatch):
    from dinunet_implementations_amd.compat.nodes import LocalNode, RemoteNode
    from dinunet_implementations_amd.compat.simulator import simulate
    monkeypatch.delenv("DINUNET_SECURE_AGG", raising=False)
    with pytest.raises(ValueError, match="in-process runtime"):
        simulate(fs_data_root, str(tmp_path), lambda: LocalNode(device="cpu"), RemoteNode,
                 overrides={"secure_agg": True, "epochs": 1})


def w_sa_sites(grp, cfg, bad_rank):
    import warnings
    from dinunet_implementations_amd.ops import FlatParams
    from dinunet_implementations_amd.parallel import make_engine
    m = _model()
    flat = FlatParams(m.parameters())
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        eng = make_engine("dSGD", m, flat, grp, {"precision_bits": "32", "dsgd_bucket_mb": 0.001,
                                                 "secure_agg": True, **cfg})
        eng2 = make_engine("dSGD", m, flat, grp, {"precision_bits": "32", "secure_agg": True, **cfg})
    own = torch.randn(flat.numel, generator=torch.Generator().manual_seed(100 + grp.rank)) * 0.1
    own[3] = 3e5 * (grp.rank + 1)  # clamped on every party
    flat.grad.copy_(own)
    eng.launch_bucket(0)  # ready before reduce(): nothing may leave yet
    early = (len(eng._handles), eng.early_launches, bool(torch.equal(flat.grad, own)))
    scale = eng.reduce()
    first = flat.grad.clone()
    flat.grad.copy_(own)
    if grp.rank == bad_rank:
        flat.grad[7] = float("nan")
    eng.reduce()
    second = flat.grad.clone()
    sd = eng.state_dict()
    eng2.load_state_dict(json.loads(json.dumps(sd)))
    return {"own": own, "first": first, "second": second, "scale": scale, "early": early,
            "buckets": len(eng.buckets), "prefers_split": eng.prefers_split, "sd": sd,
            "overlap": eng.overlap, "capturable": eng.capturable, "transport": eng.sa_transport,
            "releases": eng.sa.releases, "saturated": eng.sa.saturated,
            "nonfinite": eng.sa.nonfinite, "comm_bytes": eng.comm_bytes,
            "resumed": (eng2.sa.releases, eng2.sa.saturated, eng2.sa.nonfinite),
            "dp": None if eng.dp is None else (eng.dp.stream, eng.dp.releases),
            "warned": sum("2 parties" in str(w.message) for w in caught),
            "domain": eng.sa.domain, "calibration": eng.calibration}


@pytest.mark.parametrize("W,coll", [(2, "auto"), (3, "direct"), (3, "calibrate")])
def test_gloo_sites_hold_the_mirror_mean_bit_for_bit(W, coll):
    from dinunet_implementations_amd.ops import reference
    res = run_world(w_sa_sites, W, {"dsgd_collective": coll, "dp_fold": 2}, W - 1)
    want, sat, bad = reference.secagg_mean([o["own"] for o in res])
    assert (sat, bad) == (W, 0)
    for out in res:
        assert out["scale"] == 1.0 and torch.equal(out["first"], want)  # bit for bit, every rank
        assert out["early"] == (0, 0, True) and out["buckets"] == 1
        assert out["prefers_split"] is False and out["overlap"] is False
        assert out["transport"] == "direct" and out["capturable"] is False
        assert out["domain"] == 2 * 4096
        assert out["comm_bytes"] == (out["own"].numel() + 8) * 8
        assert bool(torch.isnan(out["second"]).all())  # one party's NaN: every mean NaN
        assert (out["releases"], out["saturated"], out["nonfinite"]) == (2, 2 * W, 1)
        assert out["sd"] == {"secure_agg": {"t": 2, "saturated": 2 * W, "nonfinite": 1,
                                            "last_saturated": W}}
        assert out["resumed"] == (2, 2 * W, 1)
        assert out["warned"] == (1 if W == 2 else 0)  # once, however many engines
        if coll == "calibrate":
            assert out["calibration"]["choice"] == "direct"
    m = torch.stack([o["own"].clamp(-2.0 ** 18, 2.0 ** 18) for o in res]).double().mean(0)
    bound = 2.0 ** -41 + (2.0 ** -24 + 2.0 ** -52) * m.abs()
    assert bool(((res[0]["first"].double() - m).abs() <= bound).all())


def test_privatise_precedes_mask():
    from dinunet_implementations_amd.ops import reference
    dp = {"dp_clip_norm": 0.5, "dp_noise_multiplier": 0.3, "dp_seed": 21}
    res = run_world(w_sa_sites, 2, dict(dp, dp_fold=1), -1)
    rel = [reference.dp_privatize(o["own"], 0.5, 0.3, 21, o["dp"][0], 1).float() for o in res]
    want, sat, bad = reference.secagg_mean(rel)
    assert (sat, bad) == (0, 0)  # the clip came first: nothing left to clamp
    for out in res:
        assert out["dp"][1] == 2 and torch.equal(out["first"], want)
    raw, _, _ = reference.secagg_mean([o["own"] for o in res])
    assert not torch.equal(want, raw)


# ---- the site loop ------------------------------------------------------------------------------
def w_fs_site(grp, data_path, out, overrides):
    from dinunet_implementations_amd.config import build_config, load_inputspec
    from dinunet_implementations_amd.runtime.site import FederatedSite
    from dinunet_implementations_amd.tasks import get_task
    specs = load_inputspec(os.path.join(data_path, "inputspec.json"))
    cfg = build_config(site_input=specs[grp.rank], overrides=overrides)
    state = {"baseDirectory": os.path.join(data_path, "input", f"local{grp.rank}", "simulatorRun")}
    T, D, H = get_task(cfg["task_id"])
    logs = FederatedSite(cfg, grp, T, D, H, state, out, verbose=False).run()
    return [{k: v for k, v in l.items() if "secure_agg" in k or k == "replica_check"}
            for l in logs]


def test_site_loop_logs_the_aggregation(fs_data_root, tmp_path, monkeypatch):
    monkeypatch.delenv("DINUNET_SECURE_AGG", raising=False)
    out = str(tmp_path)
    res = run_world(w_fs_site, 2, fs_data_root, out, {"epochs": 2, "check_replicas": True,
                                                      "secure_agg": True})
    blocks = []
    for r in range(2):
        assert all(res[r][0]["replica_check"])
        with open(os.path.join(out, f"local{r}", "FS-Classification", "fold_0", "logs.json")) as f:
            logs = json.load(f)
        sa = logs["secure_agg"]
        assert {k: sa[k] for k in ("frac_bits", "prg", "key_agreement", "parties", "transport")} \
            == {"frac_bits": 40, "prg": "chacha20", "key_agreement": "x25519", "parties": 2,
                "transport": "direct"}
        assert sa["releases"] > 0 and sa["nonfinite"] == 0 and sa["saturated"] == 0
        assert logs["secure_agg_saturated"] == [0, 0]
        text = json.dumps(logs)
        assert "key" not in text.replace("key_agreement", "")
        blocks.append(sa)
    assert blocks[0] == blocks[1]
