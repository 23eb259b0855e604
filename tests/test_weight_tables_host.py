"""The catalogue of tests/weight_tables.py on the host: every table has the property its name claims, the extended-precision reference
equals exact `Fraction` arithmetic, the two oracles (`oracle.ref_spatial.scatter_block`, `oracle.cport.scatter_block`) and the int64
reference agree bit for bit on every integer-regime table, and `engine.weight_triplets` on a +-180 table with absent cells, folded by the
column order of a 0-360 grid as `engine.get_csr` folds it, gives the catalogue's rotated table."""
from fractions import Fraction

import numpy as np
import pandas as pd
import pytest

import weight_tables as wt
from oracle import cport
from oracle.ref_spatial import scatter_block as ref_scatter

TABLES = wt.tables()
BY_NAME = {t.name: t for t in TABLES}


def test_catalogue_is_deterministic_and_well_formed():
    again = wt.tables()
    assert [t.name for t in again] == [t.name for t in TABLES] and len(TABLES) == 29
    for a, b in zip(TABLES, again):
        assert np.array_equal(a.region_idx, b.region_idx) and np.array_equal(a.cell_idx, b.cell_idx)
        assert np.array_equal(a.weight, b.weight, equal_nan=True)
        assert a.n_cells in (wt.C_SMALL, wt.C_LARGE) and a.aim and a.regime in ("both", "real", "refused")
        if len(a.weight):
            assert 0 <= a.region_idx.min() and a.region_idx.max() < a.n_regions and 0 <= a.cell_idx.min() and a.cell_idx.max() < a.n_cells
        if a.regime == "both":
            assert np.array_equal(a.weight, np.rint(a.weight)) and np.abs(a.weight).max(initial=0) <= 1024
    assert wt.C_SMALL == 3 * 128 + 14 and wt.C_LARGE == 144 * 64 + 14
    must = {t.name for t in TABLES if t.expect["rf"] is True}
    assert must == {"parity_embedded", "a_b_a", "tile_edge", "five_regions", "duplicate_pair", "descending"}
    assert {t.name for t in TABLES if t.expect["rf"] is False} == {"parity_small", "empty_all"}


def test_row_lengths_and_the_hand_worked_piece_counts():
    t = BY_NAME["row_lengths"]
    assert wt.row_lengths(t).tolist() == list(wt.ROW_LENGTHS)
    assert wt.regions_per_cell(t).max() == 3 and len(wt.duplicate_pairs(t)) == 0
    # regions interleave: no region of the short rows' area holds two neighbouring cells
    assert (np.diff(t.cell_idx[t.region_idx == 10]) > 1).all()
    assert [wt.pieces_of(n) for n in (256, 257, 320, 321, 511, 512, 513, 8192, 8193)] == [1, 5, 5, 6, 8, 8, 9, 128, 65]
    assert [wt.pieces_of(n, 128) for n in (512, 513)] == [1, 5]
    assert sum(wt.pieces_of(n) for n in wt.ROW_LENGTHS if n > 256) == 234


def test_empty_region_tables():
    for name, gone in (("empty_first", [0]), ("empty_last", [7]), ("empty_middle3", [3, 4, 5]), ("empty_all", list(range(8))), ("one_run", [0, 2])):
        t = BY_NAME[name]
        assert np.flatnonzero(wt.row_lengths(t) == 0).tolist() == gone, name
    t = BY_NAME["one_region"]
    assert t.n_regions == 1 and np.array_equal(np.sort(t.cell_idx), np.arange(t.n_cells))
    assert len(BY_NAME["empty_all"].weight) == 0


def test_runs_and_tiles():
    for name in ("parity_small", "parity_embedded"):
        t = BY_NAME[name]
        assert wt.runs_per_tile(t, 1)[:4].tolist() == [64] * 4 and wt.runs_per_tile(t, 2)[:2].tolist() == [128] * 2, name
    assert wt.runs_per_tile(BY_NAME["parity_small"], 2).sum() == 398
    assert wt.runs_per_tile(BY_NAME["parity_embedded"], 1).sum() < 9230 // 16            # long runs elsewhere: the run sums fit
    reg, _ = wt.first_two(BY_NAME["a_b_a"])
    k = reg[:64, 0]
    assert k[np.concatenate([[True], np.diff(k) != 0])].tolist() == [0, 1, 0] and wt.runs_per_tile(BY_NAME["a_b_a"], 1)[0] == 3
    first, last = wt.run_edges(BY_NAME["tile_edge"])
    assert first.tolist() == [0, 63, 127, 255, 383] and wt.runs_per_tile(BY_NAME["tile_edge"], 1).tolist() == [2, 2, 1, 2, 1, 2, 1]
    first, last = wt.run_edges(BY_NAME["whole_tiles"])
    assert first.tolist() == [0, 64, 128, 256, 384] and last.tolist() == [63, 127, 255, 383, 397]
    assert wt.runs_per_tile(BY_NAME["whole_tiles"], 1).tolist() == [1] * 7 and wt.runs_per_tile(BY_NAME["whole_tiles"], 2).tolist() == [2, 1, 1, 1]
    first, last = wt.run_edges(BY_NAME["one_run"])
    assert first.tolist() == [0] and last.tolist() == [397]
    t = BY_NAME["last_tile_only"]
    assert t.cell_idx[t.region_idx == 1].tolist() == list(range(384, 398))
    t = BY_NAME["corner_cells"]
    assert t.cell_idx[t.region_idx == 0].tolist() == [0] and t.cell_idx[t.region_idx == 2].tolist() == [397]
    t = BY_NAME["gaps"]
    assert np.flatnonzero(wt.regions_per_cell(t) == 0).tolist() == list(range(2, 398, 3))
    assert (wt.run_edges(t)[1] - wt.run_edges(t)[0]).max() == 1                         # runs of two cells between the gaps


def test_membership_and_order():
    t = BY_NAME["five_regions"]
    n = wt.regions_per_cell(t)
    assert sorted(set(n.tolist())) == [1, 2, 3, 5] and len(wt.duplicate_pairs(t)) == 0
    reg, extras = wt.first_two(t)
    # the extras of one region come from several 128-cell tiles
    is_extra = np.array([r not in reg[c] for r, c in zip(t.region_idx, t.cell_idx)])
    assert is_extra.sum() == extras.sum() > 0
    assert len(set((t.cell_idx[is_extra & (t.region_idx == 3)] // 128).tolist())) >= 3
    t = BY_NAME["duplicate_pair"]
    assert wt.duplicate_pairs(t).tolist() == [0, 63, 64, 127, 200] and len(t.weight) == 403
    reg, _ = wt.first_two(t)
    assert (reg[[0, 63, 64, 127, 200], 0] == reg[[0, 63, 64, 127, 200], 1]).all()
    t = BY_NAME["two_regions"]
    reg, _ = wt.first_two(t)
    assert reg[150].tolist() == [1, 2] and reg[10].tolist() == [0, 3] and wt.regions_per_cell(t).max() == 2
    for name, what in (("descending", "desc"), ("shuffled", "none"), ("rotated", "none")):
        t = BY_NAME[name]
        assert (np.diff(t.region_idx) >= 0).all(), name
        for r in range(t.n_regions):
            d = np.diff(t.cell_idx[t.region_idx == r])
            assert (d < 0).all() if what == "desc" else ((d < 0).any() and (d > 0).any()), (name, r)
    assert (np.diff(BY_NAME["ungrouped"].region_idx) < 0).any()
    # the rule that removes (cell, period) pairs hits the first and last cell of a run, a cell with extras and a duplicated pair
    for t in TABLES:
        bad = set(wt.nan_cells(t.n_cells).tolist())
        first, last = wt.run_edges(t) if len(t.weight) else ([], [])
        if len(first):
            assert bad & set(first.tolist()) and bad & set(last.tolist()), t.name
    assert set(np.flatnonzero(wt.first_two(BY_NAME["five_regions"])[1]).tolist()) & set(wt.nan_cells(wt.C_LARGE).tolist())
    assert set(wt.duplicate_pairs(BY_NAME["duplicate_pair"]).tolist()) <= set(wt.nan_cells(wt.C_SMALL).tolist())


def test_weight_tables():
    t = BY_NAME["zero_region"]
    assert (t.weight[t.region_idx == 2] == 0).all() and (t.weight[t.region_idx != 2] > 0).all()
    t = BY_NAME["zero_entries"]
    assert 0 < (t.weight == 0).sum() < len(t.weight) / 4 and (np.bincount(t.region_idx, t.weight) > 0).all()
    t = BY_NAME["cancelling_pair"]
    assert t.weight[t.region_idx == 8].tolist() == [5.0, -5.0]
    t = BY_NAME["negative_mixed"]
    assert (t.weight < 0).any() and (t.weight > 0).any() and all(len(set(np.sign(t.weight[t.region_idx == r]))) == 2 for r in range(8))
    t = BY_NAME["magnitudes"]
    a = np.abs(t.weight)
    assert a.min() < 2e-300 and a.max() > 1e300 and all(a[t.region_idx == r].max() / a[t.region_idx == r].min() < 2 for r in range(8))
    assert np.isnan(BY_NAME["nan_weight"].weight).sum() == 1 and np.isposinf(BY_NAME["inf_weight"].weight).sum() == 1


@pytest.mark.parametrize("name", [t.name for t in TABLES if t.n_cells == wt.C_SMALL and t.regime != "refused"])
def test_extended_reference_equals_fraction_arithmetic(name):
    """`ref_ext` against exact rational sums: the long double sum of n products is within n * 2^-63 of the exact one relative to sum |w x| —
    4096 times below the bound the routes are held to at n = 8193 — and rounds to the same double wherever no cancellation sits in between."""
    t = BY_NAME[name]
    X = wt.block_values(t.n_cells, 2, "real", seed=1)
    w = wt.real_weights(t, seed=1)
    E, A = wt.ref_ext(t.region_idx, t.cell_idx, w, X, t.n_regions)
    Ef, Af = wt.ref_fraction(t.region_idx, t.cell_idx, w, X, t.n_regions)
    n = wt.row_lengths(t)
    for r in range(t.n_regions):
        for q in range(2):
            if not wt.EXTENDED:
                assert E[r, q] == Ef[r][q] and A[r, q] == Af[r][q]
                continue
            # compare through Fractions of the long double's two double halves (hi + lo is exact)
            hi = float(E[r, q]); lo = float(E[r, q] - np.longdouble(hi))
            assert abs(Fraction(hi) + Fraction(lo) - Ef[r][q]) <= Fraction(int(n[r]) + 1, 2 ** 63) * Af[r][q], (name, r, q)
            assert abs(Fraction(float(A[r, q])) - Af[r][q]) <= Fraction(int(n[r]) + 2, 2 ** 52) * Af[r][q]
    # the exact sums are inside the bound of themselves; the longest row without its largest product is not (a small product over these
    # twenty decades can hide inside the bound: the integer regime is the check that misses no entry)
    assert wt.bound_excess(np.array([[float(Ef[r][q]) for q in range(2)] for r in range(t.n_regions)]), E, A, n) <= 0
    if len(w):
        r = int(np.argmax(n))
        rows = np.flatnonzero(t.region_idx == r)
        j = rows[np.argmax(np.abs(w[rows] * X[t.cell_idx[rows], 0]))]
        less = np.array([[float(Ef[rr][q]) for q in range(2)] for rr in range(t.n_regions)])
        less[r] -= w[j] * X[t.cell_idx[j]]
        assert wt.bound_excess(less, E, A, n) > 0


@pytest.mark.parametrize("name", [t.name for t in TABLES if t.regime == "both"])
def test_oracles_and_int64_reference_agree_bit_for_bit(name):
    t = BY_NAME[name]
    X = wt.block_values(t.n_cells, 3, "int", seed=2)
    want = wt.ref_int(t.region_idx, t.cell_idx, t.weight, X, t.n_regions).astype(np.float64)
    a = ref_scatter(X, t.region_idx, t.cell_idx, t.weight, t.n_regions)
    b = cport.scatter_block(X, t.region_idx, t.cell_idx, t.weight, t.n_regions)
    assert np.array_equal(a, want) and np.array_equal(b, want)
    # real values: the two oracles sum in table order, bit for bit
    Xr, w = wt.block_values(t.n_cells, 3, "real", seed=2), wt.real_weights(t, seed=2)
    assert np.array_equal(ref_scatter(Xr, t.region_idx, t.cell_idx, w, t.n_regions), cport.scatter_block(Xr, t.region_idx, t.cell_idx, w, t.n_regions))


def test_weight_triplets_on_a_0_360_grid_give_the_rotated_table():
    import aggfly_amd as af
    from aggfly_amd import engine as eng
    ny, nx = wt.LARGE
    r, c, w = wt.rotated_base()
    # the table as a geodataframe join leaves it: region ids that are no ranks, and entries whose cell is not on the grid
    ids = 100 + 7 * r
    tab = pd.DataFrame({"cell_id": np.concatenate([c[:50], [ny * nx + 5, -3], c[50:]]), "index_right": np.concatenate([ids[:50], [100, 107], ids[50:]]),
                        "weight": np.concatenate([w[:50], [9.0, 9.0], w[50:]])})
    lon = (np.arange(nx) + 0.5) * 360.0 / nx                                   # 0-360, no cell on the 180 meridian
    da = af.DataArray(data=np.zeros((1, ny, nx), dtype=np.float32), dims=["time", "latitude", "longitude"],
                      coords={"time": pd.date_range("2001-01-01", periods=1), "latitude": np.arange(ny) * 0.25, "longitude": lon})
    ds = af.Dataset(da, lon_is_360=True)
    order, _ = ds.lon_order_to_180()
    assert order.tolist() == [(i + nx // 2) % nx for i in range(nx)]
    rows, cols, wv, region_ids = eng.weight_triplets(tab, np.arange(ny * nx))
    iy, ix = np.divmod(cols, nx)
    cols = iy * nx + order[ix]                                                  # the fold of `engine.get_csr`: sorted-grid cell -> stored cell
    t = BY_NAME["rotated"]
    assert np.array_equal(rows, t.region_idx) and np.array_equal(cols, t.cell_idx) and np.array_equal(wv, t.weight)
    assert region_ids.tolist() == (100 + 7 * np.arange(14)).tolist()
