"""Host side of the packing Adam's split-K slab sources (``ops.slabsrc``): the (segment element ->
slab row, column) map against what ``gemm_splitk_reduce`` does with ``row_map`` -- both LSTM
directions, padded units (``Hd < HD``), the column-sum problem and the folded ones column -- and
the descriptor validation that decides between the Adam's own sum and the reduce launch."""
import dataclasses

import numpy as np
import pytest

from dinunet_implementations_amd.ops import slabsrc as ss

GRAD = 0x7000_0000_0000  # a made-up, 16-B aligned flat.grad address
GATE = 0x1234_5600       # ... and the address of THE gate row map
SLAB = 0x7100_0000_0000


def _row_map(Hd, HD):
    """ops.lstm._row_map: kernel gate row m = 4u + g -> reference row g * Hd + u, -1 padded."""
    m = np.arange(4 * HD)
    u, g = m // 4, m % 4
    return np.where(u < Hd, g * Hd + u, -1)


def _plan(I, Hd, O=8, F=12, ndir=2):
    """Pack rows ``(off, n, kind, d, dst, dst2)`` of a 2-direction LSTM + encoder weight / bias,
    sorted by offset, and the offsets by name."""
    rows, offs, off = [], {}, 0

    def add(name, n, kind, d):
        nonlocal off
        offs[name] = off
        rows.append((off, n, kind, d, 1, 1))
        off += (n + 3) // 4 * 4
    add("enc_w", O * F, ss.PK_CAST, 0)
    add("enc_b", O, ss.PK_CAST, 0)
    for d in range(ndir):
        add(f"w_ih{d}", 4 * Hd * I, ss.PK_WIH, d)
        add(f"w_hh{d}", 4 * Hd * Hd, ss.PK_WHH, d)
        add(f"b_ih{d}", 4 * Hd, ss.PK_BIAS, d)
        add(f"b_hh{d}", 4 * Hd, ss.PK_BIAS, d)
    return rows, offs


def _ptr(offs, name):
    return GRAD + 4 * offs[name]


def _desc(M, N, C, splits=3, row_map=None, ncol=0, xcol=-1, C2=None, ldc=None, X1=None, X2=None,
          slab=SLAB, room=0):
    return ss.SlabDesc(slab=slab, slab_elems=splits * M * N + room, M=M, N=N, splits=splits,
                       alpha=1.0, beta=1.0, row_map=row_map, ncol=ncol, xcol=xcol, C=C, C2=C2,
                       ldc=N if ldc is None else ldc, X1=X1, X2=X2)


def _reduce(slab, rmap, n_out, ldc, ncol=0, xcol=-1):
    """What gemm_splitk_reduce + epi_store leave: ``(C, X)`` flat outputs (NaN = never written)."""
    S, M, N = slab.shape
    C = np.full(n_out, np.nan)
    X = np.full(M, np.nan)
    tot = slab.sum(0)
    for m in range(M):
        o = m if rmap is None else rmap[m]
        if o < 0:
            continue
        for c in range(N):
            if ncol > 0 and c >= ncol:
                continue
            if xcol >= 0 and c >= xcol:
                if c == xcol:
                    X[o] = tot[m, c]
                continue
            C[o * ldc + c] = tot[m, c]
    return C, X


def _gather(src, slab, n, Hd):
    tot = slab.sum(0)
    return np.array([tot[ss.slab_rc(src, j, Hd)] for j in range(n)])


@pytest.mark.parametrize("I,Hd,HD", [(16, 8, 8), (12, 44, 64), (8, 5 * 4, 32)])
def test_gate_rows_map_is_the_inverse_of_row_map(I, Hd, HD):
    rows, offs = _plan(I, Hd)
    rmap = _row_map(Hd, HD)
    rng = np.random.default_rng(0)
    for d in (0, 1):
        for name, N in ((f"w_ih{d}", I), (f"w_hh{d}", Hd)):
            desc = _desc(4 * HD, N, _ptr(offs, name), row_map=GATE)
            got = ss.match([desc], rows, GRAD, I, Hd, HD, GATE)
            (si, src), = got.items()
            assert rows[si][0] == offs[name] and src.mode == ss.SRC_ROWS | ss.SRC_GATE
            slab = rng.standard_normal((3, 4 * HD, N))
            want, _ = _reduce(slab, rmap, 4 * Hd * N, N)
            assert not np.isnan(want).any()  # the reduce writes every element of the segment
            assert np.array_equal(_gather(src, slab, 4 * Hd * N, Hd), want)
            # ... and every index stays inside the slab, for the last element too
            r, c = ss.slab_rc(src, 4 * Hd * N - 1, Hd)
            assert 0 <= r < 4 * HD and 0 <= c < N


@pytest.mark.parametrize("Hd,HD", [(8, 8), (44, 64)])
def test_column_sum_problem_feeds_both_biases(Hd, HD):
    I = 16
    rows, offs = _plan(I, Hd)
    rmap = _row_map(Hd, HD)
    rng = np.random.default_rng(1)
    for d in (0, 1):
        desc = _desc(4 * HD, 8, _ptr(offs, f"b_ih{d}"), row_map=GATE, ncol=1, ldc=1,
                     C2=_ptr(offs, f"b_hh{d}"))
        got = ss.match([desc], rows, GRAD, I, Hd, HD, GATE)
        assert sorted(rows[i][0] for i in got) == [offs[f"b_ih{d}"], offs[f"b_hh{d}"]]
        slab = rng.standard_normal((3, 4 * HD, 8))
        want, _ = _reduce(slab, rmap, 4 * Hd, 1, ncol=1)
        for src in got.values():
            assert src.mode == ss.SRC_COL | ss.SRC_GATE
            assert np.array_equal(_gather(src, slab, 4 * Hd, Hd), want)


def test_plain_rows_and_plain_column_sum():
    rows, offs = _plan(16, 8, O=8, F=12)
    rng = np.random.default_rng(2)
    w = _desc(8, 12, _ptr(offs, "enc_w"))
    b = _desc(8, 8, _ptr(offs, "enc_b"), ncol=1, ldc=1, slab=SLAB + 4 * w.slab_elems)
    got = ss.match([w, b], rows, GRAD, 16, 8, 8, GATE)
    assert {rows[i][0]: s.mode for i, s in got.items()} == {offs["enc_w"]: ss.SRC_ROWS,
                                                           offs["enc_b"]: ss.SRC_COL}
    for i, src in got.items():
        slab = rng.standard_normal((3, src.M, src.N))
        n = rows[i][1]
        want, _ = _reduce(slab, None, n, 12 if n > 8 else 1, ncol=0 if n > 8 else 1)
        assert np.array_equal(_gather(src, slab, n, 8), want)


@pytest.mark.parametrize("Hd,HD", [(8, 8), (24, 32)])
def test_folded_ones_column_is_described_but_not_taken(Hd, HD):
    """The folded form (xcol: slab rows of Hd + 4, the sum at column Hd, going to X1 / X2) maps
    like the others; launches that fold run 128 / 256 tiles and keep their reduce, so ``match``
    refuses them."""
    I = 16
    rows, offs = _plan(I, Hd)
    rmap = _row_map(Hd, HD)
    rng = np.random.default_rng(3)
    desc = _desc(4 * HD, Hd + 4, _ptr(offs, "w_hh1"), row_map=GATE, xcol=Hd, ldc=Hd,
                 X1=_ptr(offs, "b_ih1"), X2=_ptr(offs, "b_hh1"))
    one = ss.describe(desc, rows, GRAD, I, Hd, HD, GATE)
    by = {rows[i][0]: s for i, s in one.items()}
    slab = rng.standard_normal((3, 4 * HD, Hd + 4))
    wantC, wantX = _reduce(slab, rmap, 4 * Hd * Hd, Hd, xcol=Hd)
    assert np.array_equal(_gather(by[offs["w_hh1"]], slab, 4 * Hd * Hd, Hd), wantC)
    for name in ("b_ih1", "b_hh1"):
        assert np.array_equal(_gather(by[offs[name]], slab, 4 * Hd, Hd), wantX[:4 * Hd])
    assert ss.match([desc], rows, GRAD, I, Hd, HD, GATE) is None


def test_validation_refuses_what_does_not_fit_its_segment():
    I, Hd, HD = 16, 8, 8
    rows, offs = _plan(I, Hd)
    good = _desc(4 * HD, I, _ptr(offs, "w_ih0"), row_map=GATE)
    assert ss.match([good], rows, GRAD, I, Hd, HD, GATE) is not None
    R = dataclasses.replace
    bad = {
        "one split": R(good, splits=1),
        "too many splits": R(good, splits=ss.MAX_SPLITS + 1, slab_elems=10 ** 9),
        "slab too small": R(good, slab_elems=good.slab_elems - 1),
        "slab misaligned": R(good, slab=SLAB + 4),
        "row length": R(good, N=I + 4, slab_elems=10 ** 9, ldc=I + 4),
        "ldc": R(good, ldc=I + 4),
        "target not a segment start": R(good, C=good.C + 16),
        "target outside flat.grad": R(good, C=GRAD - 64),
        "another segment's count": R(good, C=_ptr(offs, "w_hh0")),
        "not the gate map": R(good, row_map=GATE + 64),
        "M is not 4 HD": R(good, M=4 * HD + 4, slab_elems=10 ** 9),
        "a map on a plain segment": R(good, C=_ptr(offs, "enc_w")),
        "two stored columns": R(good, ncol=2),
        "second output of a weight": R(good, C2=_ptr(offs, "w_ih1")),
        "alpha": R(good, alpha=float("nan")),
    }
    for why, d in bad.items():
        assert ss.match([d], rows, GRAD, I, Hd, HD, GATE) is None, why
    # the same segment fed twice: inside one launch, and by an earlier launch of the step
    assert ss.match([good, good], rows, GRAD, I, Hd, HD, GATE) is None
    si = next(iter(ss.match([good], rows, GRAD, I, Hd, HD, GATE)))
    assert ss.match([good], rows, GRAD, I, Hd, HD, GATE, taken={si: None}) is None
    # one refused descriptor refuses the whole launch (its reduce runs for every problem)
    other = _desc(4 * HD, Hd, _ptr(offs, "w_hh0"), row_map=GATE)
    assert ss.match([other, bad["ldc"]], rows, GRAD, I, Hd, HD, GATE) is None
    assert ss.match([], rows, GRAD, I, Hd, HD, GATE) is None
    # a bias whose element count is no multiple of 4 (the kernel sums four elements per thread)
    rows5, offs5 = _plan(I, 8, O=6)
    b = _desc(6, 8, GRAD + 4 * offs5["enc_b"], ncol=1, ldc=1)
    assert ss.match([b], rows5, GRAD, I, 8, 8, GATE) is None
