"""One small plan per kernel of the packed short-group menu (aggfly_amd/csrc/gen_variants.py: MORE_MENUS, packed_short_menu), built on
`variant_recipes.Recipe` and the stored-integer helpers of `packed_recipes`.

Pure Python and numpy.  How a recipe selects its kernel (afhip_planner.cpp: choose_packed_short_variant):
  group length     inner groups as `variant_recipes._inner_lengths` has them for the float forms: [2] * 150 (pair), [4] * 75 (quad),
                   [3] * 101 (tri: a lone group in the last block of six rows), _RAG * 10 (rag: one to four rows, length-1 groups)
  periods          eight groups each, the second one empty (`variant_recipes._outer_bounds`)
  columns          K == kmax, every column lean — mean | sum | min | max | sine_dd -> integer power -> sum | mean — as
                   `variant_recipes._columns` writes them for a lean form; the sine-only form: two plain sine_dd columns.  The sine_dd
                   thresholds are moved onto values of stored integers that occur in the cube (`packed_recipes._snap_columns`)
  cells per lane   1100 cells (a multiple of four) for four cells per lane, 1102 (even, no multiple of four) for two, 1101 (odd) for one:
                   each exceeds 256 * vec and is no multiple of a wave's 64 * vec

The menu is not one of `gen_variants.MENUS` (whose keys and counts the older recipe modules know), so `variant_recipes.menu_of` cannot
hand it out: `menu_of` here reads `MORE_MENUS`.

The data (`stored_cube`): `packed_recipes.stored_cube_for` — temperatures around 12 C, the stored extremes -32768 / 32767, the fill in
the FIRST row of some groups, whole groups of fills, three cells that are all fill — plus the fill in the LAST row only of other groups.
"""
from __future__ import annotations

import numpy as np

import packed_recipes as pr
import variant_recipes as vr

KEY = "packed_short"
I16 = pr.I16
GROUP_ROWS = {"pair": (2,), "quad": (4,), "tri": (3,), "rag": (1, 2, 3, 4)}
PERIOD = 8                      # groups per period


def menu_of(kind="full"):
    """The tuples of the packed short-group menu of the build `kind`, in table order."""
    gv = vr.gen_variants()
    return list({k: fn for k, fn, _ in gv.MORE_MENUS}[KEY](kind))


def recipe(v) -> vr.Recipe:
    """The plan for kernel `v` of the menu (a tuple of gen_variants.packed_short_menu, or its `variant_recipes.Variant`)."""
    v = vr.variant(v) if not isinstance(v, vr.Variant) else v
    assert v.dtype == I16 and v.pipe == 0 and v.form and v.lean and v.nthr == 0
    lens = vr._inner_lengths(v.form, 0)
    ib = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ob = vr._outer_bounds(len(lens), PERIOD)
    cols = pr._snap_columns(vr._columns(v, 0, v.kmax, False))
    sine = sorted({x for c in cols if c["inner"] == "sine_dd" for x in c["inner_args"][:2]})
    return vr.Recipe(v.name, I16, int(ib[-1]), pr.n_cells_for(v.vec), ib, ob, cols, True, 0, sine_edges=sine)


def last_row_fill_groups(r: vr.Recipe):
    """The groups whose last row gets the fill for some cells: every fifth non-empty group from the second on, of two rows or more."""
    ib = r.inner_bounds
    return [int(g) for g in np.flatnonzero(np.diff(ib) > 0)[1::5] if ib[g + 1] - ib[g] >= 2]


def stored_cube(r: vr.Recipe, seed=0):
    """int16 [T, n_cells] for recipe `r` (see the module docstring)."""
    q = pr.stored_cube_for(r, seed)
    rng = np.random.default_rng(seed + 1)
    ib = r.inner_bounds
    for g in last_row_fill_groups(r):
        q[ib[g + 1] - 1, rng.choice(r.n_cells, 25, replace=False)] = pr.FILL
    return q


def fill_census(r: vr.Recipe, q):
    """What the planted fills amount to: (cells of some group with the fill in the first row only, ... in the last row only, whole groups
    of fills outside the all-fill cells, the number of all-fill cells)."""
    ib = r.inner_bounds
    f = q == pr.FILL
    ocean = f.all(axis=0)
    first = last = whole = 0
    for g in range(len(ib) - 1):
        a, b = int(ib[g]), int(ib[g + 1])
        if b - a < 2:
            continue
        n = f[a:b].sum(axis=0)
        first += int(((n == 1) & f[a]).sum())
        last += int(((n == 1) & f[b - 1]).sum())
        whole += int(((n == b - a) & ~ocean).sum())
    return first, last, whole, int(ocean.sum())
