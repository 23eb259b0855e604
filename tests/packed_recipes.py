"""One small plan per kernel variant of the int16-packed menu (aggfly_amd/csrc/gen_variants.py: packed_menu), shaped like the float
recipes of `variant_recipes` — as many columns as the kernel holds, its threshold-slot tier filled — with an int16 cube and the
rule that unpacks it.

Pure Python and numpy.  How a recipe selects its variant (afhip_planner.cpp: choose_packed_variant): the statistic, slot and column
tiers as in `variant_recipes`; cells per lane by the row length — a multiple of four for the four-cell kernels (the light shapes
only), even but no multiple of four for the two-cell ones, odd for one cell per lane.  Every row length exceeds one 256-thread
workgroup's cells and is no multiple of them.

The data: stored integers whose values (ERA5-like 0.0017 / 281.3, then - 273.15) are temperatures around 12 C.  Every threshold,
bin edge and hinge knot of the recipe is moved onto the value of a stored integer that occurs in the cube, next to its two
neighbours, so the strict compares meet equality; +-32767 and -32768 are present; the fill value marks first rows of groups, whole
groups and ocean cells.
"""
from __future__ import annotations

import numpy as np

import variant_recipes as vr

I16 = 2                                     # include/aggfly_hip.h: AFHIP_I16
FILL = -32767
PAIRS = [(0.0017, 281.3), (None, -273.15)]   # (multiply, add) in float32; None: that half is left out


def np_unpack(q, pairs=PAIRS, fill=FILL):
    """The unpack rule in numpy float32, one rounded operation at a time; NaN at the fill."""
    q = np.asarray(q, dtype=np.int16)
    f = q.astype(np.float32)
    for m, a in pairs:
        if m is not None:
            f = f * np.float32(m)
        if a is not None:
            f = f + np.float32(a)
    if fill is not None:
        f = np.where(q == np.int16(fill), np.float32(np.nan), f)
    return f


def stored_near(value, pairs=PAIRS):
    """The stored integer whose value is nearest to `value` (the rule is monotone: bisection over int16)."""
    lo, hi = -32766, 32766
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if float(np_unpack([mid], pairs, None)[0]) <= value:
            lo = mid
        else:
            hi = mid
    return lo


def _snap(e):
    return float(np_unpack([stored_near(e)], PAIRS, None)[0])


def _snap_columns(cols):
    out = []
    for c in cols:
        c = dict(c)
        for key in ("inner_args", "outer_args"):
            if key in c:
                a = c[key]
                c[key] = (_snap(a[0]), _snap(a[1]), a[2])
        if c.get("transform") == "hinge":
            c["transform_arg"] = _snap(c["transform_arg"])
        out.append(c)
    return out


def n_cells_for(vec):
    return {4: 1100, 2: 1102, 1: 1101}[vec]


def recipe(v) -> vr.Recipe:
    """The plan for packed variant `v` (a tuple of gen_variants.packed_menu)."""
    v = vr.variant(v) if not isinstance(v, vr.Variant) else v
    assert v.dtype == I16 and v.pipe == 0 and not v.form
    nslots, K = vr._shape(v)
    lens = vr._inner_lengths("", 0)
    ib = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ob = vr._outer_bounds(len(lens), 8)
    cols = _snap_columns(vr._columns(v, nslots, K, False))
    edges, sine = set(), set()
    for c in cols:
        if c["inner"] in ("dd", "bins"):
            edges.update(c["inner_args"][:2])
        if c["inner"] == "sine_dd":
            sine.update(c["inner_args"][:2])
        if c.get("transform") == "hinge":
            edges.add(c["transform_arg"])
    return vr.Recipe(v.name, I16, int(ib[-1]), n_cells_for(v.vec), ib, ob, cols, True, 0, edges=sorted(edges), sine_edges=sorted(sine))


def stored_cube_for(r: vr.Recipe, seed=0):
    """int16 [T, n_cells] for recipe `r` (see the module docstring)."""
    rng = np.random.default_rng(seed)
    T, C = r.T, r.n_cells
    q0, per_deg = stored_near(12.0), 1.0 / 0.0017
    q = np.clip(np.rint(q0 + rng.normal(0.0, 9.0, (T, C)) * per_deg), -32766, 32766).astype(np.int16)
    flat = q.reshape(-1)
    plant = [32767, -32768, 32766, -32766]
    for e in r.edges:
        s = stored_near(e)
        plant += [s, s, s + 1, s - 1]
    plant += [stored_near(e) for e in r.sine_edges for _ in range(4)]
    plant = np.array(plant * max(1, 2000 // len(plant)), dtype=np.int16)
    flat[rng.choice(flat.size, plant.size, replace=False)] = plant
    ib = r.inner_bounds
    ne = np.flatnonzero(np.diff(ib) > 0)
    for g in ne[::5]:                                    # the fill in the first row of a group, for some cells
        q[ib[g], rng.choice(C, 25, replace=False)] = FILL
    for g in ne[2::7]:                                   # whole groups of fills
        q[ib[g]:ib[g + 1], rng.choice(C, 4, replace=False)] = FILL
    q[:, [3, C // 2, C - 1]] = FILL                      # ocean cells, the last one included
    return q
