"""One small plan per kernel of the packed region-fused menu (aggfly_amd/csrc/gen_variants.py: LATER_MENUS, packed_rf_menu), built on
`variant_recipes.Recipe` and the stored-integer helpers of `packed_recipes`.

Pure Python and numpy.  A twin has no plan of its own: the planner picks its PLAIN kernel (afhip_planner.cpp: choose_packed_variant /
choose_packed_short_variant, at two cells or one per lane) and finds the twin beside it (twin_of), so a recipe is the plain kernel's plan
— its name is the plain kernel's, which is what `describe()` prints — made eligible for the route (rf_plan_ok): several periods, no
`exact_order`, no float32 rounding of the final value, period values that are a large share of the cube.
  cells            71 x 130 = 9,230 for two cells per lane (even, no multiple of four: the four-cell kernels are out of reach, the last wave
                   tile is partly filled), 71 x 129 = 9,159 (odd) for one
  time             general kernels: 60 days of hourly steps; short-group kernels: 60 groups of two (pair), four (quad), three (tri) rows, or
                   of two to four (rag: 6-hourly data with missing steps)
  periods          general kernels: thirteen — twelve of five groups and an EMPTY second one; short-group kernels: six — five of nine to
                   fourteen groups and an empty second one; a daily panel — one period per group, the second one empty — for the
                   threshold-only kernels and the light two-row forms, whose share threshold is the higher one (10 %)
  columns          as many as the kernel holds, its threshold-slot tier filled: `variant_recipes._columns` for the plain kernel, the
                   thresholds moved onto values of stored integers that occur in the cube (`packed_recipes._snap_columns`)

The data (`stored_cube`): `packed_recipes.stored_cube_for` — temperatures around 12 C (the unpack rule ends in the K -> deg C fold), the
stored extremes -32768 / 32767, the fill in the first row of some groups, whole groups of fills, three cells that are all fill — plus a
whole PERIOD of fills for some cells.
"""
from __future__ import annotations

import numpy as np

import packed_recipes as pr
import variant_recipes as vr

KEY = "packed_rf"
I16 = pr.I16
NY = 71
NX = {2: 130, 1: 129}
GROUPS = 60
SHORT_ROWS = {"pair": 2, "quad": 4, "tri": 3}
WHOLE_PERIOD = 3                # the period that is all fill for WHOLE_PERIOD_CELLS cells
WHOLE_PERIOD_CELLS = 6
_MASK = vr.PAIR | vr.LEAN | vr.SS2 | vr.QUAD | vr.TRI | vr.RAG


def menu_of(kind="full"):
    """The tuples of the packed region-fused menu of the build `kind`, in table order."""
    gv = vr.gen_variants()
    return list({k: fn for k, fn, _ in gv.LATER_MENUS}[KEY](kind))


def plain_menus(kind="full"):
    """The production kernels a twin can belong to: the general packed menu and the packed short-group menu."""
    gv = vr.gen_variants()
    return [t for t in vr.menu_of("packed", kind) if t[8]] + [t for t in {k: fn for k, fn, _ in gv.MORE_MENUS}["packed_short"](kind) if t[8]]


def plain_of(v, kind="full"):
    """The plain kernel of twin `v` (a `variant_recipes.Variant`): every field but `depth` equal, the region-fused bit aside.  None: there is none."""
    for t in plain_menus(kind):
        w = vr.variant(t)
        if (w.dtype, w.pipe, w.vec, w.stat, w.nthr, w.kmax, w.feat) == (v.dtype, v.pipe, v.vec, v.stat, v.nthr, v.kmax, v.feat & ~vr.RF):
            return w
    return None


def light_two_row(v):
    """afhip_planner.cpp: rf_share_ok — the two-row forms other than the six-column lean one need period values of 10 % of a packed cube."""
    return v.form == "pair" and not (v.lean == 1 and v.kmax == 6)


def daily_panel(v):
    return light_two_row(v) or (not v.form and v.stat == 0)


def inner_bounds(v):
    if not v.form:
        lens = np.full(GROUPS, 24)
    elif v.form == "rag":
        lens = np.full(GROUPS, 4)
        lens[np.random.default_rng(51).choice(GROUPS, 13, replace=False)] = 3
        lens[[7, 31]] = 2
    else:
        lens = np.full(GROUPS, SHORT_ROWS[v.form])
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def outer_bounds(v):
    if daily_panel(v):
        return np.array([0, 1, 1] + list(range(2, GROUPS + 1)), dtype=np.int64)
    if not v.form:
        return np.array([0, 5, 5, 10, 15, 20, 25, 30, 35, 40, 45, 50, 55, 60], dtype=np.int64)
    return np.array([0, 9, 9, 20, 33, 47, 60], dtype=np.int64)


def share(r: vr.Recipe):
    """Per-cell period values against the cube's bytes (afhip_planner.cpp: rf_share; two bytes an element)."""
    return (len(r.outer_bounds) - 1) * len(r.columns) * 8.0 / (r.T * 2.0)


def recipe(v) -> vr.Recipe:
    """The plan that runs twin `v` (a tuple of gen_variants.packed_rf_menu, or its `variant_recipes.Variant`)."""
    v = vr.variant(v) if not isinstance(v, vr.Variant) else v
    assert v.dtype == I16 and v.pipe == 0 and v.has(vr.RF) and v.vec in NX
    plain = plain_of(v)
    assert plain is not None, v.name
    nslots, K = (0, plain.kmax) if plain.form else vr._shape(plain)
    cols = pr._snap_columns(vr._columns(plain, nslots, K, False))
    edges, sine = set(), set()
    for c in cols:
        if c["inner"] in ("dd", "bins"):
            edges.update(c["inner_args"][:2])
        if c["inner"] == "sine_dd":
            sine.update(c["inner_args"][:2])
        if c.get("transform") == "hinge":
            edges.add(c["transform_arg"])
    ib = inner_bounds(plain)
    return vr.Recipe(plain.name, I16, int(ib[-1]), NY * NX[v.vec], ib, outer_bounds(plain), cols, False, 0, region_fused=True,
                     edges=sorted(edges), sine_edges=sorted(sine))


def whole_period_cells(r: vr.Recipe):
    return [11 + 97 * i for i in range(WHOLE_PERIOD_CELLS)]


def stored_cube(r: vr.Recipe, seed=0):
    """int16 [T, n_cells] for recipe `r` (see the module docstring)."""
    q = pr.stored_cube_for(r, seed)
    ib, ob = r.inner_bounds, r.outer_bounds
    q[ib[ob[WHOLE_PERIOD]]:ib[ob[WHOLE_PERIOD + 1]], whole_period_cells(r)] = pr.FILL
    return q
