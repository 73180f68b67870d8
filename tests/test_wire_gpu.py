"""The payload kernels (``csrc/kernels/payload.hip``, through ``parallel.collective``) against the
exact wire model of ``tests/wire_ref.py`` and, through it, the fp64 mean: the grid of
``tests/test_wire_ref.py`` (edge and poisoned gradients, every wire, scales 1, 1/2 and 1/3), the
exchange between pack, rowsum and unpack emulated by slicing and concatenating rank-blocks on the
device.  Wire bits after pack and after rowsum and fp32 bits after unpack must equal the model's
(positions where both are NaN apart); the unpacked mean must lie within the model's derived
bound of the fp64 mean.

Every destination is a 16-byte aligned view at an odd multiple of 16 bytes inside a larger tensor
filled with a sentinel, 64 guard elements on both sides, and the WHOLE tensor is compared: headers
1..7 zero, everything inside written, nothing outside.  Sources sit at the same kind of offset.

Each case's worst error / bound goes to ``$DINUNET_ERR_LOG`` (jsonl) when set;
``profiles/wire_codec_errors.md`` is one such run.  Every call here is a legal one: the refusals
are host-side argument checks that launch nothing.

Measured on one MI355X (``profiles/wire_codec_errors.md``): 2,040 payloads of the grid, the
hand-made blocks and the grid-stride case without one mismatching bit; the largest error / bound
0.939 (fp16), 0.918 (bf16), 0.330 (fp32), each the model's own figure.  Against the kernels of
the commit before (exponent clamped at -100) the four fp16 cases that hold a sub-block maximum of
2^115 and above fail (``n37-W2`` and ``n98313-W16``, edge and poisoned) and nothing else does.
"""
import json
import os

import numpy as np
import pytest
import torch

import wire_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
TORCH_DT = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
SHAPES = R.shapes()
IDS = [f"n{n}-W{W}" for n, W in SHAPES]


def _C():
    from dinunet_implementations_amd.parallel import collective as C
    return C


def _record(**row):
    path = os.environ.get("DINUNET_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"test": "wire", **row}) + "\n")


class Guarded:
    """``numel`` elements of ``dtype`` at byte offset 64 * itemsize + 16 of a sentinel-filled
    tensor (16-byte aligned, an odd multiple of 16), 64 guard elements behind them."""

    def __init__(self, numel, dtype):
        es = torch.empty(0, dtype=dtype).element_size()
        self.idt, self.ndt, sentinel = ((torch.int16, np.uint16, 0x5A5A) if es == 2 else
                                        (torch.int32, np.uint32, 0x5A5A5A5A))
        self.lo = GUARD + 16 // es
        self.numel = numel
        self.whole = torch.empty(self.lo + numel + GUARD, dtype=dtype, device=DEV)
        self.whole.view(self.idt).fill_(sentinel)
        self.view = self.whole[self.lo:self.lo + numel]
        assert self.view.data_ptr() % 32 == 16
        self.sentinel = self.ndt(sentinel)

    def put(self, t):
        self.view.copy_(t)
        return self.view

    def bits(self):
        return self.whole.view(self.idt).cpu().numpy().view(self.ndt)

    def expect(self, want_bits, wire):
        """Mismatching positions of the whole tensor: guards = sentinel, inside = ``want_bits``
        (shorter than the view: the rest must still be the sentinel)."""
        want = np.full(self.whole.numel(), self.sentinel, dtype=self.ndt)
        want[self.lo:self.lo + len(want_bits)] = want_bits
        return R.mismatches(self.bits(), want, wire)


def dev_bits(bits, wire):
    """model wire bits -> a device tensor of the wire type."""
    idt = np.int32 if wire == "fp32" else np.int16
    return torch.from_numpy(bits.view(idt).copy()).to(DEV).view(TORCH_DT[wire])


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("poison", [False, True], ids=["edge", "poisoned"])
@pytest.mark.parametrize("wire,scaled", R.MODES, ids=[f"{w}{'' if s else '-unscaled'}" for w, s in R.MODES])
@pytest.mark.parametrize("n,W", SHAPES, ids=IDS)
def test_kernels_equal_the_model(n, W, wire, scaled, poison):
    C = _C()
    xs, _ = R.inputs(n, W, poison)
    chunk = C.chunk_for(n, W)
    blk = C.payload_numel(chunk)
    dt = TORCH_DT[wire]
    compared = 0
    for scale in R.SCALES:
        sent_m, means_m, out_m = R.staged(n, W, wire, scaled, scale, poison)
        sent = []
        for w in range(W):
            src = Guarded(n, torch.float32).put(torch.from_numpy(np.array(xs[w])))
            dst = Guarded(W * blk, dt)
            C.to_payload(src, dst.view, W, chunk, scale, scaled)
            bad = dst.expect(sent_m[w], wire)
            assert bad.size == 0, ("pack", scale, w, bad[:8] - dst.lo)
            sent.append(dst.view)
        red = float(np.float32(scale) / np.float32(W))
        means = []
        for r in range(W):
            src = Guarded(W * blk, dt).put(torch.cat([s[r * blk:(r + 1) * blk] for s in sent]))
            dst = Guarded(blk, dt)
            C.rowsum(src, dst.view, W, chunk, red)
            bad = dst.expect(means_m[r], wire)
            assert bad.size == 0, ("rowsum", scale, r, bad[:8] - dst.lo)
            means.append(dst.view)
        src = Guarded(W * blk, dt).put(torch.cat(means))
        out = Guarded(n, torch.float32)
        C.from_payload(src, out.view, W, chunk, scale)
        bad = out.expect(f32_bits(out_m), "fp32")
        assert bad.size == 0, ("unpack", scale, bad[:8] - out.lo)
        compared += 2 * W + 1
        if scale == 1.0 and scaled and not poison:
            got = out.view.cpu().numpy()
            ratio = R.err_ratio(got, xs, wire)
            print(f"wire {wire} n {n} W {W}: error / bound = {ratio:.5f}")
            _record(case=f"n{n}-W{W}", wire=wire, ratio=float(f"{ratio:.6g}"), mismatches=0)
            assert ratio <= 1.0
    _record(case=f"n{n}-W{W}-{'poisoned' if poison else 'edge'}", wire=wire, scaled=scaled,
            payloads_compared=compared, mismatches=0)


def _handmade(W, wire, seed):
    """W rank-blocks of two sub-blocks: sub-block 0 mixes the exponents -100, 0 and 100 across the
    sites (fp16), sub-block 1 holds 100 everywhere but at one site."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((W, 2, R.SB)) * np.exp2(rng.integers(-10, 14, (W, 2, R.SB))))
    blocks = np.zeros((W, 2, R.SBS), dtype=R.BITS[wire])
    blocks[:, :, R.HDR:] = R.encode(v.astype(np.float32), wire).reshape(W, 2, R.SB)
    if wire == "fp16":
        e = np.empty((W, 2), dtype=np.float32)
        e[:, 0] = [(-100, 0, 100)[w % 3] for w in range(W)]
        e[:, 1] = 100
        if W > 1:
            e[W // 2, 1] = 0
        blocks[:, :, 0] = R.encode(e, wire).reshape(W, 2)
    return blocks.reshape(-1)


@pytest.mark.parametrize("wire", R.WIRES)
@pytest.mark.parametrize("W", [1, 16])
def test_rowsum_on_handmade_blocks(W, wire):
    C = _C()
    chunk = 2 * R.SB
    blocks = _handmade(W, wire, seed=W)
    if wire == "fp16":
        assert sorted(set(R.exponents(blocks, wire).tolist())) == ([-100, 100] if W == 1 else [-100, 0, 100])
    red = np.float32(1.0) / np.float32(W)
    want = R.rowsum(blocks, W, chunk, wire, red)
    src = Guarded(blocks.size, TORCH_DT[wire]).put(dev_bits(blocks, wire))
    dst = Guarded(R.numel(chunk), TORCH_DT[wire])
    C.rowsum(src, dst.view, W, chunk, float(red))
    bad = dst.expect(want, wire)
    assert bad.size == 0, bad[:8] - dst.lo
    assert np.all(np.isfinite(R.decode(want, wire)))
    # the model's sum against fp64: W - 1 fp32 additions, the 1/W product, one wire rounding
    un = np.exp2(-R.exponents(blocks, wire).astype(np.float64)).reshape(W, 2, 1)
    vals = R.decode(blocks, wire).reshape(W, 2, R.SBS)[:, :, R.HDR:].astype(np.float64) * un
    true = vals.sum(axis=0) / W
    got = R.unpack(want, chunk, wire).astype(np.float64).reshape(2, R.SB)
    S = np.abs(vals).sum(axis=0) / W
    g = (W + 1) * 2.0 ** -24 / (1 - (W + 1) * 2.0 ** -24)
    bound = (g * S + np.maximum(R.U[wire] * np.abs(got), R.H[wire] * un.max(axis=0))
             + 2.0 ** -149)
    assert np.all(np.abs(got - true) <= bound)


def test_grid_stride_loops():
    """fp16, W = 2, n = 2 * 8193 * 2048 - 3: 16,386 sub-blocks to pack and unpack and 8,193 to sum
    per rank, against grids of 8,192 workgroups -- every kernel loops, and a workgroup's second
    sub-block has another magnitude (2^((g mod 40) - 30); 8192 mod 40 = 32) than its first, so a
    maximum left over in shared memory would show.  The model is compared on the first, the last
    and 64 evenly spaced sub-blocks of each rank-block, and the guards bit for bit."""
    C = _C()
    W, nsbc, wire = 2, 8193, "fp16"
    n = W * nsbc * R.SB - 3
    chunk = C.chunk_for(n, W)
    assert chunk == nsbc * R.SB
    blk = C.payload_numel(chunk)
    rng = np.random.default_rng(5)
    base = [((1 + rng.random(R.SB)) * np.where(rng.random(R.SB) < 0.5, -1, 1)).astype(np.float32)
            for _ in range(W)]
    g_all = np.arange(W * nsbc)
    mags = [np.exp2(((g_all + 13 * w) % 40) - 30).astype(np.float32) for w in range(W)]
    pick = np.unique(np.concatenate([[0, nsbc - 1], np.linspace(0, nsbc - 1, 64).astype(np.int64)]))

    def host(w, gs):
        x = mags[w][gs][:, None] * base[w][None, :]
        flat = x.reshape(-1)
        if gs[-1] == W * nsbc - 1:
            flat[-3:] = 0          # past n: the pack pads with zeros
        return flat

    def head_tail(gd, what):
        b = torch.cat([gd.whole[:gd.lo], gd.whole[gd.lo + gd.numel:]]).view(gd.idt).cpu().numpy()
        assert np.all(b.view(gd.ndt) == gd.sentinel), what

    sent, sent_m = [], []
    for w in range(W):
        x = (torch.from_numpy(mags[w]).to(DEV)[:, None] * torch.from_numpy(base[w]).to(DEV)[None, :])
        src = Guarded(n, torch.float32).put(x.reshape(-1)[:n])
        del x
        dst = Guarded(W * blk, torch.float16)
        C.to_payload(src, dst.view, W, chunk)
        head_tail(dst, "pack guards")
        rows = dst.view.view(-1, R.SBS)
        assert bool((rows[:, 1:R.HDR].view(torch.int16) == 0).all())
        per_rank = []
        for r in range(W):
            gs = r * nsbc + pick
            want = R.pack(host(w, gs), 1, len(gs) * R.SB, wire)
            got = rows[torch.from_numpy(gs).to(DEV)].reshape(-1).view(torch.int16).cpu().numpy().view(np.uint16)
            assert R.mismatches(got, want, wire).size == 0, ("pack", w, r)
            per_rank.append(want)
        sent.append(dst.view)
        sent_m.append(per_rank)
    means, means_m = [], []
    for r in range(W):
        src = Guarded(W * blk, torch.float16).put(torch.cat([s[r * blk:(r + 1) * blk] for s in sent]))
        dst = Guarded(blk, torch.float16)
        C.rowsum(src, dst.view, W, chunk, 1.0 / W)
        head_tail(dst, "rowsum guards")
        want = R.rowsum(np.concatenate([sent_m[w][r] for w in range(W)]), W, len(pick) * R.SB, wire,
                        np.float32(0.5))
        got = dst.view.view(-1, R.SBS)[torch.from_numpy(pick).to(DEV)].reshape(-1)
        assert R.mismatches(got.view(torch.int16).cpu().numpy().view(np.uint16), want, wire).size == 0, r
        means.append(dst.view)
        means_m.append(want)
    del sent
    src = Guarded(W * blk, torch.float16).put(torch.cat(means))
    out = Guarded(n, torch.float32)
    C.from_payload(src, out.view, W, chunk)
    head_tail(out, "unpack guards")
    # every element was written: the inputs are below 2^11, the sentinel reads as 1.5e16
    assert not bool((out.view.view(torch.int32) == 0x5A5A5A5A).any())
    padded = torch.cat([out.view, torch.zeros(3, device=DEV)]).view(-1, R.SB)
    worst = 0.0
    for r in range(W):
        gs = r * nsbc + pick
        want = R.unpack(means_m[r], len(pick) * R.SB, wire)
        got = padded[torch.from_numpy(gs).to(DEV)].reshape(-1).cpu().numpy()
        if r == W - 1:
            want, got = want[:-3], got[:-3]
        assert R.mismatches(f32_bits(got), f32_bits(want), "fp32").size == 0, ("unpack", r)
        xs = [host(w, gs)[:len(got)] for w in range(W)]
        worst = max(worst, R.err_ratio(got, xs, wire))
    print(f"grid-stride: error / bound = {worst:.5f}")
    _record(case="grid-stride", wire=wire, ratio=float(f"{worst:.6g}"), mismatches=0)
    assert worst <= 1.0


def test_entry_points_refuse_bad_arguments():
    """DN_BAD_SHAPE (1) and no launch: chunk not a multiple of 2,048, world * chunk < n,
    misaligned pointers, an unknown type code."""
    C = _C()
    from dinunet_implementations_amd.ops import _lib
    L = _lib.lib()
    st = _lib.stream()
    n, W, chunk = 5000, 2, 4096
    x = Guarded(n, torch.float32)
    pay = Guarded(C.blocks_numel(W, chunk), torch.float16)
    one = Guarded(C.payload_numel(chunk), torch.float16)
    xp, pp, op = x.view.data_ptr(), pay.view.data_ptr(), one.view.data_ptr()
    calls = {
        "pack chunk % 2048": lambda: L.dn_payload_pack(xp, pp, n, W, 4096 - 8, 1.0, 1, 1, st),
        "pack world * chunk < n": lambda: L.dn_payload_pack(xp, pp, n, W, 2048, 1.0, 1, 1, st),
        "pack src misaligned": lambda: L.dn_payload_pack(xp + 4, pp, n - 1, W, chunk, 1.0, 1, 1, st),
        "pack dst misaligned": lambda: L.dn_payload_pack(xp, pp + 2, n, W, chunk, 1.0, 1, 1, st),
        "pack type": lambda: L.dn_payload_pack(xp, pp, n, W, chunk, 1.0, 1, 7, st),
        "pack type -1": lambda: L.dn_payload_pack(xp, pp, n, W, chunk, 1.0, 1, -1, st),
        "rowsum chunk % 2048": lambda: L.dn_payload_rowsum(pp, op, W, 4096 - 8, 0.5, 1, st),
        "rowsum src misaligned": lambda: L.dn_payload_rowsum(pp + 2, op, W, chunk, 0.5, 1, st),
        "rowsum dst misaligned": lambda: L.dn_payload_rowsum(pp, op + 8, W, chunk, 0.5, 1, st),
        "rowsum type": lambda: L.dn_payload_rowsum(pp, op, W, chunk, 0.5, 3, st),
        "rowsum world 0": lambda: L.dn_payload_rowsum(pp, op, 0, chunk, 0.5, 1, st),
        "unpack src misaligned": lambda: L.dn_payload_unpack(pp + 2, xp, n, 1.0, 1, st),
        "unpack dst misaligned": lambda: L.dn_payload_unpack(pp, xp + 4, n - 1, 1.0, 1, st),
        "unpack type": lambda: L.dn_payload_unpack(pp, xp, n, 1.0, 7, st),
    }
    for what, call in calls.items():
        assert call() == 1, what
    torch.cuda.synchronize()
    for g in (x, pay, one):
        assert np.all(g.bits() == g.sentinel)
    # and the legal call next to them goes through
    assert L.dn_payload_pack(xp, pp, n, W, chunk, 1.0, 1, 1, st) == 0
    torch.cuda.synchronize()
    assert not np.all(pay.bits()[pay.lo:pay.lo + pay.numel] == pay.sentinel)
