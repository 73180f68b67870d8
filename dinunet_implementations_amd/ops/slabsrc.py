"""Split-K slab sources of the packing Adam: what a deferred reduce would have done, matched
against the optimizer's pack segments.

A split grouped weight-gradient launch (``ops.gemm.mm_grouped``) normally ends in
``gemm_splitk_reduce``: per problem it sums the fp32 partials ``[splits][M][N]``, applies ``alpha``
/ ``beta`` and scatters the rows through ``row_map`` into ``flat.grad``, which the fused Adam reads
back one launch later.  With the reduce deferred the launch hands back one :class:`SlabDesc` per
problem instead, and :func:`match` turns them into per-segment sources the Adam launch sums itself
(``optim.hip slab_grad``) -- or refuses, and the launch keeps its reduce.

Everything here is host arithmetic on integers (no tensors, no GPU): :func:`slab_rc` is the
mirror of the kernel's (segment element -> slab row, column) decode.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

# PackKind / SlabMode of csrc/kernels/optim.hip
PK_CAST, PK_WIH, PK_WHH, PK_BIAS = 1, 2, 3, 4
SRC_ROWS, SRC_COL, SRC_GATE = 1, 2, 4
MAX_SPLITS = 64


@dataclass
class SlabDesc:
    """One problem of a split launch whose reduce was not launched (addresses as integers)."""
    slab: int            # base of this problem's partials, fp32 [splits][M][N]
    slab_elems: int      # fp32 elements the slab allocation holds from ``slab`` on
    M: int
    N: int               # slab row length (a folded column sum included: xcol + 4)
    splits: int
    alpha: float
    beta: float
    row_map: Optional[int]  # device address of the int32 [M] output row map, or None
    ncol: int            # > 0: only the first ncol columns are stored (a column-sum problem)
    xcol: int            # >= 0: column xcol is a folded column sum going to X1 / X2
    C: int
    C2: Optional[int]
    ldc: int
    X1: Optional[int] = None
    X2: Optional[int] = None


@dataclass
class SlabSource:
    """A segment's gradient source (``optim.hip SlabSrc`` plus the host-side column window)."""
    slab: int
    slab_elems: int
    M: int
    N: int
    splits: int
    mode: int
    alpha: float
    beta: float
    R: int = 0      # segment row length (SRC_ROWS; N unless the slab rows carry a folded column)
    col0: int = 0   # slab column of the segment's column 0 (SRC_COL of a folded sum: xcol)


def slab_rc(src: SlabSource, j: int, Hd: int) -> Tuple[int, int]:
    """(slab row, slab column) holding the gradient of segment element ``j``."""
    if src.mode & SRC_COL:
        row, k = j, 0
    else:
        row, k = divmod(j, src.R or src.N)
    if src.mode & SRC_GATE:
        g, u = divmod(row, Hd)
        row = 4 * u + g
    return row, src.col0 + k


def _segment_at(rows: Sequence[tuple], grad_ptr: int, ptr: Optional[int]) -> Optional[int]:
    if ptr is None:
        return None
    for i, r in enumerate(rows):
        if grad_ptr + 4 * r[0] == ptr:
            return i
    return None


def describe(desc: SlabDesc, rows: Sequence[tuple], grad_ptr: int, I: int, Hd: int, HD: int,
             gate_map: Optional[int]) -> Optional[Dict[int, SlabSource]]:
    """Sources ``{segment index: SlabSource}`` of one descriptor against the pack ``rows``
    (``(offset, numel, kind, d, dst, dst2)`` sorted by offset, ``PersistentPack.rows``), or None
    when the descriptor does not describe exactly those segments: element counts, the row length,
    the target addresses inside ``flat.grad`` at the segment offsets, the gate row map (``gate_map``:
    the address of THE ``4u + g -> g * Hd + u`` map of this ``(Hd, HD)``), the slab extent."""
    d = desc
    if not (2 <= d.splits <= MAX_SPLITS) or d.M <= 0 or d.N <= 0 or d.slab % 16 or not d.slab:
        return None
    if d.splits * d.M * d.N > d.slab_elems:
        return None
    if not (math.isfinite(d.alpha) and math.isfinite(d.beta)):
        return None
    gate = d.row_map is not None
    if gate and (gate_map is None or d.row_map != gate_map or Hd <= 0 or HD < Hd or d.M != 4 * HD):
        return None
    nrows = 4 * Hd if gate else d.M
    mode = SRC_GATE if gate else 0
    out: Dict[int, SlabSource] = {}

    def src(mode_, R=0, col0=0):
        return SlabSource(d.slab, d.slab_elems, d.M, d.N, d.splits, mode_, d.alpha, d.beta, R, col0)

    def column(targets, col0) -> bool:
        for t in targets:
            si = _segment_at(rows, grad_ptr, t)
            if si is None or si in out or rows[si][1] != nrows or nrows % 4:
                return False
            if gate and rows[si][2] != PK_BIAS:
                return False
            out[si] = src(mode | SRC_COL, col0=col0)
        return True

    if d.ncol > 0:  # a column sum as its own a^T @ ones problem: column 0 -> C (and C2)
        if d.ncol != 1 or d.xcol >= 0 or d.ldc != 1:
            return None
        return out if column([d.C] + ([d.C2] if d.C2 is not None else []), 0) else None
    if d.C2 is not None:
        return None
    R = d.N
    if d.xcol >= 0:  # folded: the weight's columns [0, xcol), the column sum at xcol
        if d.N != d.xcol + 4 or d.xcol % 8 or d.X1 is None:
            return None
        R = d.xcol
        if not column([d.X1] + ([d.X2] if d.X2 is not None else []), d.xcol):
            return None
    si = _segment_at(rows, grad_ptr, d.C)
    if si is None or si in out or R % 4 or d.ldc != R or rows[si][1] != nrows * R:
        return None
    if gate and not ((rows[si][2] == PK_WIH and R == I) or (rows[si][2] == PK_WHH and R == Hd)):
        return None
    out[si] = src(mode | SRC_ROWS, R=R)
    return out


def match(descs: Sequence[SlabDesc], rows: Sequence[tuple], grad_ptr: int, I: int, Hd: int,
          HD: int, gate_map: Optional[int], taken=()) -> Optional[Dict[int, SlabSource]]:
    """Sources of a whole launch, or None: every descriptor must describe segments no other
    descriptor (of this launch or, ``taken``, an earlier one of the step) feeds, in a form the
    kernel sums.  The folded column sum exists only in launches of 128 x 128 / 256 x 256 tiles,
    which keep their reduce, so the kernel does not take it and it is refused here."""
    got: Dict[int, SlabSource] = {}
    for d in descs:
        one = describe(d, rows, grad_ptr, I, Hd, HD, gate_map)
        if one is None or d.xcol >= 0:
            return None
        if any(k in got or k in taken for k in one):
            return None
        got.update(one)
    return got or None
