"""A catalogue of hand-built region x cell weight tables, aimed at the boundaries the spatial stage names in its own code, with the two
references every route is held to.  Host only, deterministic; shared by tests/test_weight_tables_host.py and tests/test_gpu_weight_tables.py.

Grids.  SMALL: 398 cells (2 x 199) = three two-cell-per-lane wave tiles of 128 cells (six one-cell tiles of 64) and a 14-cell tail.  LARGE:
9230 cells (71 x 130) = 144 tiles of 64 cells (72 of 128) and 14, large enough for one row of 8193 entries.  Every table stays far below
262,144 entries, so the segment length of `afhip_csr_create` is its minimum, 64; AFHIP_SPMM_SEG reaches the others.

The segment rule, worked by hand for seg = 64 (`pieces_of` restates it; rows up to 4 * seg = 256 entries stay whole):
    257  -> want = ceil(257 / 64) = 5,               piece = up64(ceil(257 / 5)) = 64,      pieces = ceil(257 / 64)   = 5
    8192 -> want = min(128, 128) = 128,              piece = up64(64) = 64,                 pieces                    = 128
    8193 -> want = min(128, 129) = 128 (the cap),    piece = up64(ceil(8193 / 128) = 65) = 128, pieces = ceil(8193 / 128) = 65

Value regimes.  INTEGER: weights and cell values are integers of magnitude <= 1024, so every product and partial sum is an integer far below
2^53 and any order of addition gives the same double: the reference is `np.add.at` on int64 (`ref_int`) and every route must equal it bit
for bit.  REAL: wide dynamic range, mixed signs; the reference E is summed in extended precision (`ref_ext`; exact `Fraction`s where the
platform's long double is no wider than double), and a route's sum of n rounded products in any order satisfies
    |got - E| <= (n + 2) * 2^-52 * sum_j |w_j * x_j|
(`bound_excess`; n the row length, + 2 for the piece merge and the mean division the region-fused route moves behind the sum; 2^-52 is twice
the unit roundoff).  Nothing in that bound is measured.
"""
from __future__ import annotations

from collections import namedtuple
from fractions import Fraction

import numpy as np

SMALL = (2, 199)                      # ny, nx: 398 cells
LARGE = (71, 130)                     # 9230 cells
C_SMALL, C_LARGE = SMALL[0] * SMALL[1], LARGE[0] * LARGE[1]

ROW_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 321, 511, 512, 513, 8192, 8193)

#: name, region_idx, cell_idx, weight (float64, integer-valued unless regime says otherwise), n_regions, n_cells, expect, then:
#: aim = the boundary the table is there for; regime = "both" (integer and real), "real" (weights are no integers) or "refused" (a
#: non-finite weight: np.add.at makes w * 0 = NaN of every cell that is not valid, empty periods included; the library refuses the table).
#: expect = {"rf": True (must be seen on the region-fused route) | False (cannot fit it: "why" says so) | None (not asserted)}
Table = namedtuple("Table", "name region_idx cell_idx weight n_regions n_cells expect aim regime")


def _w(n, k=0):
    """n integer weights in 1 .. 1024, no two neighbours alike."""
    return (1 + (np.arange(n, dtype=np.int64) * 389 + 17 * k) % 1024).astype(np.float64)


def _table(name, r, c, w, R, C, aim, rf=None, why="", regime="both"):
    r, c, w = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(w, dtype=np.float64)
    assert len(r) == len(c) == len(w) and len(w) < 262_144
    assert rf is not False or why
    return Table(name, r, c, w, int(R), int(C), {"rf": rf, "why": why}, aim, regime)


def _by_region(reg_of_cell, C, keep=None):
    """One entry per cell (where ``keep``), sorted by region then cell."""
    cells = np.arange(C)
    if keep is not None:
        cells = cells[keep]
    r = np.asarray(reg_of_cell)[cells]
    o = np.argsort(r, kind="stable")
    return r[o], cells[o]


def pieces_of(length: int, seg: int = 64) -> int:
    """Segments `afhip_csr_create` makes of a row (SPMM_MAX_PIECES = 128): the rule restated, for the hand-worked counts above."""
    up64 = lambda x: (x + 63) // 64 * 64
    if length <= 4 * seg:
        return 1
    want = min(128, -(-length // seg))
    piece = up64(-(-length // want))
    return -(-length // piece)


def tables():
    out = []
    C, Cl = C_SMALL, C_LARGE

    # ---- row lengths (large grid): one region per length.  The 26 short rows share cells 0 .. 3607 round-robin, so neighbouring cells
    # belong to different regions; the two long rows walk the grid with stride 3 (coprime to 9230: no cell twice in a row)
    short = [n for n in ROW_LENGTHS if n < 8192]
    left = np.array(short)
    r, c, cell = [], [], 0
    while left.sum():
        for i in np.flatnonzero(left):
            r.append(i); c.append(cell); cell += 1
            left[i] -= 1
    r, c = np.array(r), np.array(c)
    o = np.argsort(r, kind="stable")
    r, c = r[o], c[o]
    for k, n in enumerate((8192, 8193)):
        r = np.concatenate([r, np.full(n, len(short) + k)])
        c = np.concatenate([c, (3 * np.arange(n) + k) % Cl])
    out.append(_table("row_lengths", r, c, _w(len(r)), len(ROW_LENGTHS), Cl,
                      "rows of 0 .. 8193 entries: every unroll remainder, 256 whole / 257 cut in 5, 8192 -> 128 pieces, 8193 -> the piece cap, 65"))

    # ---- empty regions (small grid): eight regions of 50 cells (the last 48), some of them emptied
    base = np.arange(C) // 50
    for name, gone, aim in (("empty_first", [0], "the first region has no cell"), ("empty_last", [7], "the last region has no cell"),
                            ("empty_middle3", [3, 4, 5], "three empty regions in a row in the middle")):
        r, c = _by_region(base, C, ~np.isin(base, gone))
        out.append(_table(name, r, c, _w(len(r), 1), 8, C, aim))
    out.append(_table("empty_all", [], [], [], 8, C, "no entry at all: nnz = 0, every region empty", rf=False, why="the table has no runs at all"))
    out.append(_table("one_region", np.zeros(C, int), np.arange(C), _w(C, 2), 1, C, "n_regions = 1 holding every cell"))

    # ---- runs and tiles
    out.append(_table("parity_small", *_by_region(np.arange(C) % 2, C), _w(C, 3), 2, C,
                      "region = cell parity: every cell its own run, 64 and 128 runs a tile, the most an 8-bit run id holds",
                      rf=False, why="398 runs on 398 cells: more run sums than the area of the per-cell values holds"))
    reg = 2 + np.arange(Cl) // 1024
    reg[:256] = np.arange(256) % 2
    out.append(_table("parity_embedded", *_by_region(reg, Cl), _w(Cl, 4), int(reg.max()) + 1, Cl,
                      "cells 0 .. 255 by parity (128 runs in each of two two-cell tiles, 64 in four one-cell tiles) among runs of 1024 cells", rf=True))
    reg = np.arange(C) // 100 + 1
    reg[:20], reg[20:40], reg[40:64] = 0, 1, 0
    out.append(_table("a_b_a", *_by_region(reg, C), _w(C, 5), 5, C, "a region that comes back inside one tile: A B A in cells 0 .. 63", rf=True))
    reg = np.searchsorted([63, 127, 255, 383], np.arange(C), side="right")
    out.append(_table("tile_edge", *_by_region(reg, C), _w(C, 6), 5, C,
                      "runs that start on the last cell of a tile (63, 127, 255, 383) and continue into the next", rf=True))
    reg = np.searchsorted([64, 128, 256, 384], np.arange(C), side="right")
    out.append(_table("whole_tiles", *_by_region(reg, C), _w(C, 7), 5, C, "runs that are exactly one tile of 64 and of 128 cells"))
    out.append(_table("one_run", np.ones(C, int), np.arange(C), _w(C, 8), 3, C, "one run over every tile, between two empty regions"))
    out.append(_table("last_tile_only", *_by_region((np.arange(C) >= 384).astype(int), C), _w(C, 9), 2, C,
                      "a region that lives only in the partly filled last tile (cells 384 .. 397)"))
    reg = np.ones(C, int); reg[0], reg[-1] = 0, 2
    out.append(_table("corner_cells", *_by_region(reg, C), _w(C, 10), 3, C, "regions that own only cell 0 and only cell C - 1"))
    r, c = _by_region(np.arange(C) // 50, C, np.arange(C) % 3 != 2)
    out.append(_table("gaps", r, c, _w(len(r), 11), 8, C, "every third cell in no region"))

    # ---- membership
    # large grid, 24 regions of 400 cells; of every 64 cells, cell 5 sits in two regions, cell 6 in three, cell 7 in five (the next ones,
    # wrapping at the last): the extras of one region come from every tile its neighbours cover
    b = np.arange(Cl) // 400
    R = int(b.max()) + 1
    extra = np.select([np.arange(Cl) % 64 == 5, np.arange(Cl) % 64 == 6, np.arange(Cl) % 64 == 7], [1, 2, 4], 0)
    r = np.concatenate([b] + [((b + k) % R)[extra >= k] for k in range(1, 5)])
    c = np.concatenate([np.arange(Cl)] + [np.arange(Cl)[extra >= k] for k in range(1, 5)])
    o = np.lexsort((c, r))
    out.append(_table("five_regions", r[o], c[o], _w(len(r), 12), R, Cl, "cells in 1, 2, 3 and 5 regions; extras from several tiles", rf=True))
    # small grid, four regions of 100 cells; five pairs listed twice (tile edges and an interior cell), the copies with other weights
    b = np.arange(C) // 100
    dup = np.array([0, 63, 64, 127, 200])
    r, c = np.concatenate([b, b[dup]]), np.concatenate([np.arange(C), dup])
    o = np.lexsort((c, r))
    out.append(_table("duplicate_pair", r[o], c[o], _w(len(r), 13), 4, C, "the same (region, cell) pair listed twice: np.add.at adds both", rf=True))
    r, c = np.concatenate([b, [2, 2, 3, 3]]), np.concatenate([np.arange(C), [150, 151, 10, 11]])
    o = np.lexsort((c, r))
    out.append(_table("two_regions", r[o], c[o], _w(len(r), 14), 4, C,
                      "cells whose two entries are consecutive regions (150, 151: 1 and 2) and the first and the last region (10, 11: 0 and 3)"))

    # ---- order
    r, c = _by_region(b, C)
    desc = np.lexsort((-c, r))
    out.append(_table("descending", r[desc], c[desc], _w(C, 15), 4, C, "entries of each region in descending cell order", rf=True))
    perm = np.lexsort((np.random.default_rng(7).permutation(C), r))
    out.append(_table("shuffled", r[perm], c[perm], _w(C, 16), 4, C, "entries of each region in a fixed shuffled order"))
    r, c, w = rotated_base()
    out.append(_table("rotated", r, fold(c, LARGE[1]), w, 14, Cl, "every grid row rotated by nx // 2: the 0-360 longitude fold breaks runs at the wrap"))
    r, c = _by_region(b, C)
    perm = np.random.default_rng(8).permutation(C)
    out.append(_table("ungrouped", r[perm], c[perm], _w(C, 17)[perm], 4, C, "triplets not grouped by region: the stable sort of hip.CSR restores table order"))

    # ---- weights (small grid, eight regions of 50 cells)
    b = np.arange(C) // 50
    r, c = _by_region(b, C)
    w = _w(C, 18); w[r == 2] = 0.0
    out.append(_table("zero_region", r, c, w, 8, C, "a whole region of zero weights: den == 0"))
    w = _w(C, 19); w[::5] = 0.0
    out.append(_table("zero_entries", r, c, w, 8, C, "single zero entries"))
    out.append(_table("cancelling_pair", np.concatenate([r, [8, 8]]), np.concatenate([c, [7, 300]]), np.concatenate([_w(C, 20), [5.0, -5.0]]), 9, C,
                      "a two-entry region (+w, -w): den == 0 by cancellation, not by zeros"))
    w = _w(C, 21); w[c % 3 == 0] *= -1.0
    out.append(_table("negative_mixed", r, c, w, 8, C, "negative weights mixed with positive ones"))
    mag = 10.0 ** (-300.0 + 600.0 * r / 7.0)
    out.append(_table("magnitudes", r, c, (1.0 + (np.arange(C) % 9) / 9.0) * mag, 8, C,
                      "1e-300 .. 1e300 inside one table, one magnitude per region so nothing overflows", regime="real"))
    w = _w(C, 22); w[123] = np.nan
    out.append(_table("nan_weight", r, c, w, 8, C, "one NaN weight: refused by afhip_csr_create (AFHIP_E_INVALID)", regime="refused"))
    w = _w(C, 23); w[123] = np.inf
    out.append(_table("inf_weight", r, c, w, 8, C, "one +inf weight: refused likewise", regime="refused"))

    names = [t.name for t in out]
    assert len(set(names)) == len(names)
    return out


def rotated_base():
    """The table whose longitude fold is the catalogue's "rotated" table: 14 regions of 700 cells (the last 130) on the +-180-sorted large grid."""
    r, c = _by_region(np.arange(C_LARGE) // 700, C_LARGE)
    return r, c, _w(C_LARGE, 24)


def fold(c, nx):
    """Sorted-grid cell -> stored cell of a 0-360 grid of even ``nx``: every grid row rotated by nx // 2."""
    iy, ix = np.divmod(np.asarray(c), nx)
    return iy * nx + (ix + nx // 2) % nx


def everything_table():
    """The end-to-end case (large grid, +-180-sorted cell ids; the dataset is 0-360, so the engine folds it): empty regions (ids 0, 5, 6 and 15
    of 16), a cut row (region 1: 2000 cells), junction cells in three regions, a zero-weight region (3), a cancelling pair (region 14)."""
    C = C_LARGE
    reg = np.select([np.arange(C) < 2000, np.arange(C) < 2500, np.arange(C) < 3000, np.arange(C) < 3400],
                    [1, 2, 3, 4], 7 + (np.arange(C) - 3400) // 900)                  # 7 .. 13
    r, c = reg.copy(), np.arange(C)
    j = np.arange(1990, 2010)                                                         # junction cells: also in regions 4 and 7
    r, c = np.concatenate([r, np.full(20, 4), np.full(20, 7)]), np.concatenate([c, j, j])
    w = _w(len(r), 25); w[r == 3] = 0.0
    r, c, w = np.concatenate([r, [14, 14]]), np.concatenate([c, [40, 9000]]), np.concatenate([w, [3.0, -3.0]])
    o = np.lexsort((c, r))
    return r[o], c[o], w[o] / 1024.0, 16


# ---------------------------------------------------------------------------------------------------------------------------------
# properties (plain numpy; tests/test_weight_tables_host.py asserts them per table)
# ---------------------------------------------------------------------------------------------------------------------------------
def row_lengths(t):
    return np.bincount(t.region_idx, minlength=t.n_regions)


def first_two(t):
    """reg[c, e]: the region of cell c's e-th entry (e = 0, 1) in CSR order, -1 = none — what the run tables are built from; and the
    number of entries beyond the second per cell."""
    o = np.argsort(t.region_idx, kind="stable")
    reg = np.full((t.n_cells, 2), -1, dtype=np.int64)
    extras = np.zeros(t.n_cells, dtype=np.int64)
    for r, c in zip(t.region_idx[o], t.cell_idx[o]):
        if reg[c, 0] < 0:
            reg[c, 0] = r
        elif reg[c, 1] < 0:
            reg[c, 1] = r
        else:
            extras[c] += 1
    return reg, extras


def runs_per_tile(t, vec, e=0):
    """Runs of entry e in every wave tile of 64 * vec cells: a run starts at a cell with an entry whose region differs from the cell
    before, or that is the tile's first cell."""
    reg, _ = first_two(t)
    k = reg[:, e]
    tc = 64 * vec
    start = (k >= 0) & ((np.arange(t.n_cells) % tc == 0) | (k != np.concatenate([[-2], k[:-1]])))
    return np.add.reduceat(start.astype(np.int64), np.arange(0, t.n_cells, tc))


def run_edges(t, e=0):
    """(first cells, last cells) of the runs of entry e, ignoring tile cuts."""
    reg, _ = first_two(t)
    k = reg[:, e]
    prev, nxt = np.concatenate([[-2], k[:-1]]), np.concatenate([k[1:], [-2]])
    return np.flatnonzero((k >= 0) & (k != prev)), np.flatnonzero((k >= 0) & (k != nxt))


def regions_per_cell(t):
    return np.bincount(t.cell_idx, minlength=t.n_cells)


def duplicate_pairs(t):
    key = t.region_idx * t.n_cells + t.cell_idx
    u, n = np.unique(key, return_counts=True)
    return u[n > 1] % t.n_cells


# ---------------------------------------------------------------------------------------------------------------------------------
# cell values
# ---------------------------------------------------------------------------------------------------------------------------------
def nan_cells(C):
    """Cells that lose (cell, period) pairs to NaN: the first and last cell of every 64-cell tile and of the grid (the first and last cells
    of the catalogue's runs), the junction cells 5 .. 7 of every 64, the duplicated pairs' cells and a scatter of every 37th cell."""
    c = np.arange(C)
    return np.flatnonzero((c % 64 == 0) | (c % 64 == 63) | (c == C - 1) | ((c % 64 >= 5) & (c % 64 <= 7)) | (c == 200) | (c % 37 == 11))


def block_values(C, Q, regime, seed=0):
    """X[C, Q] float64: integers of magnitude <= 1024, or reals of mixed sign over twelve decades."""
    rng = np.random.default_rng(1000 + seed)
    if regime == "int":
        return rng.integers(-1024, 1025, (C, Q)).astype(np.float64)
    return rng.choice([-1.0, 1.0], (C, Q)) * 10.0 ** rng.uniform(-6, 6, (C, Q))


def real_weights(t, seed=0):
    """The table's weights for the real regime: each integer weight times a factor over eight decades (zeros, signs and non-finite entries
    stay; a table that is "real" keeps its weights)."""
    if t.regime != "both":
        return t.weight
    rng = np.random.default_rng(2000 + seed)
    return t.weight * 10.0 ** rng.uniform(-4, 4, len(t.weight))


def day_values(C, days, regime, seed=0):
    """v[days, C]: the value a cell holds on every step of a day — multiples of 6 in -12 .. 36, so that the mean over a period of one, two or
    three days is an integer too; NaN days by `nan_cells`: cell c loses day (c % days), every eleventh of them all days."""
    rng = np.random.default_rng(3000 + seed)
    v = 6.0 * rng.integers(-2, 7, (days, C)).astype(np.float64)
    if regime == "real":
        v = v + rng.uniform(-0.5, 0.5, (days, C))
    bad = nan_cells(C)
    v[bad % days, bad] = np.nan
    v[:, bad[::11]] = np.nan
    return v


def cube_of_days(v, steps_per_day, dtype, jitter=False, seed=0):
    """[days * steps, C]: each day's value repeated over its steps (integer regime: the day mean is then exact); ``jitter`` (real regime) adds
    a per-step offset.  A NaN day has ONE NaN step, its third, where the day has that many."""
    days, C = v.shape
    cube = np.repeat(np.where(np.isnan(v), 0.0, v), steps_per_day, axis=0)
    if jitter:
        cube = cube + np.random.default_rng(4000 + seed).normal(0.0, 3.0, cube.shape)
    d, c = np.nonzero(np.isnan(v))
    cube[d * steps_per_day + min(2, steps_per_day - 1), c] = np.nan
    return cube.astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def ref_int(region_idx, cell_idx, w, X, R):
    """out[R, Q] int64 = sum_j w[j] * X[cell[j]]: `np.add.at` on int64 (w, X integer-valued float64)."""
    wi, Xi = np.asarray(w).astype(np.int64), np.asarray(X).astype(np.int64)
    assert np.array_equal(wi, w) and np.array_equal(Xi, X), "integer regime: the values must be integers"
    out = np.zeros((R, Xi.shape[1]), dtype=np.int64)
    np.add.at(out, region_idx, wi[:, None] * Xi[cell_idx])
    assert np.abs(out).max(initial=0) < 2 ** 53
    return out


EXTENDED = np.finfo(np.longdouble).nmant >= 63


def ref_fraction(region_idx, cell_idx, w, X, R):
    """(E, A) as nested lists of `Fraction`: E[r][q] = sum_j w_j x_j, A[r][q] = sum_j |w_j x_j|, exactly."""
    Q = X.shape[1]
    E = [[Fraction(0)] * Q for _ in range(R)]
    A = [[Fraction(0)] * Q for _ in range(R)]
    for r, c, wj in zip(region_idx.tolist(), cell_idx.tolist(), np.asarray(w).tolist()):
        fw = Fraction(wj)
        for q in range(Q):
            p = fw * Fraction(float(X[c, q]))
            E[r][q] += p
            A[r][q] += abs(p)
    return E, A


def ref_ext(region_idx, cell_idx, w, X, R):
    """(E, A) [R, Q] in extended precision (long double of >= 64 significant bits; else exact Fractions rounded once)."""
    if not EXTENDED:
        E, A = ref_fraction(region_idx, cell_idx, w, X, R)
        return np.array(E, dtype=object), np.array(A, dtype=object)
    p = np.asarray(w, dtype=np.longdouble)[:, None] * np.asarray(X, dtype=np.longdouble)[cell_idx]
    E, A = np.zeros((R, X.shape[1]), dtype=np.longdouble), np.zeros((R, X.shape[1]), dtype=np.longdouble)
    np.add.at(E, region_idx, p)
    np.add.at(A, region_idx, np.abs(p))
    return E, A


def bound_excess(got, E, A, n_rows):
    """max over the panel of |got - E| - (n_r + 2) * 2^-52 * A (<= 0: inside the bound); got [..., R, Q], n_rows [R]."""
    if EXTENDED:
        err = np.abs(np.asarray(got, dtype=np.longdouble) - E)
        lim = (np.asarray(n_rows, dtype=np.longdouble)[:, None] + 2) * np.longdouble(2.0) ** -52 * A
        return float(np.max(err - lim, initial=0.0))
    worst = Fraction(0)
    for r in range(E.shape[0]):
        for q in range(E.shape[1]):
            worst = max(worst, abs(Fraction(float(got[r, q])) - E[r, q]) - Fraction(int(n_rows[r]) + 2, 2 ** 52) * A[r, q])
    return float(worst)
