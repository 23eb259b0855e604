"""One small plan per LDS-histogram kernel for partitions whose INTERIOR widths differ (aggfly_amd/csrc/gen_variants.py: cell_map_menu;
afhip_cell_map.h), beside `end_bins_recipes`, whose helpers it reuses: six to sixteen contiguous strict bins, the first and the last of
them end bins (finite or open), the others of at least three distinct widths — as float32, float64 and int16-packed plans.

Pure Python and numpy.  How a recipe selects its variant (afhip_planner.cpp: find_partition -> find_cell_map, choose_hist_variant): the
storage by the dtype; cells per lane by the row length (packed: even rows take two where the menu holds the form); stat tier by a mean
column; `sl` by identity outers with one period per inner group; the `_cmap` forms by interior widths that no equal-width candidate
fits.  Which ends a recipe gets (open, finite, one of each) rotates with the form.

The data: what `end_bins_recipes` plants around every edge — the value itself, one to three steps to either side (ulps; stored integers on
packed cubes), the outer limits and their neighbours, values far outside, +-0, +-inf, +-max, NaN / the fill — and the same around EVERY
CELL BOUNDARY of the map that is no edge (`cells_of`): the points where the guessed bin changes although the true bin does not, which only
this form can get wrong.  `Recipe.edges` therefore lists the bin edges and the cell boundaries; `planted` says what a cube holds.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

import end_bins_recipes as eb
import packed_hist_recipes as ph
import packed_recipes as pr
import variant_recipes as vr

CM = vr.gen_variants().Feat.CELL_MAP
EB = eb.EB
INF = float("inf")
MAX_CELLS = 254

# interior widths of the per-kernel recipes, in degrees: four distinct values, the smallest 2.5 (cells of 1.25: 60 / 52 of them)
WIDTHS = [10.0, 7.5, 5.0, 5.0, 2.5, 2.5, 5.0, 5.0, 2.5, 2.5, 5.0, 5.0, 7.5, 10.0]
# the issue's eight-bin spec
EIGHT = [(-INF, -10.0), (-10.0, 0.0), (0.0, 10.0), (10.0, 20.0), (20.0, 25.0), (25.0, 30.0), (30.0, 35.0), (35.0, INF)]


def edges_from(e0, widths):
    return [float(x) for x in e0 + np.concatenate([[0.0], np.cumsum(widths)])]


def partition(interior_edges, lower, upper):
    """The bins (t0, t1): the end bin (lower, E[0]), the interior bins, the end bin (E[n], upper)."""
    return eb.with_ends(interior_edges, lower, upper)


def interior_edges(bins):
    b = sorted(bins)
    return [t0 for t0, _ in b[1:]]


def cells_of(bins):
    """(w, M, cell boundaries that are no edge) of the partition's cell map, by the planner's rule: w half of the smallest interior width,
    M = ceil((E[n] - E[0]) / w) with a tolerance of 1e-9 w, boundaries E[0] + g w."""
    e = interior_edges(bins)
    w = 0.5 * min(b - a for a, b in zip(e[:-1], e[1:]))
    m = int(math.ceil((e[-1] - e[0]) / w - 1e-9))
    bounds = [e[0] + g * w for g in range(m)]
    inner = [x for x in bounds if all(abs(x - y) > 1e-9 * w for y in e)]
    return w, m, inner


def distinct_widths(bins):
    e = interior_edges(bins)
    return sorted({round(b - a, 9) for a, b in zip(e[:-1], e[1:])})


ENDS = {(0, 0): "open", (0, 1): "finite", (1, 0): "finite_open", (1, 1): "open_finite"}      # (single level, stat) -> the end bins


def ends_for(kind, dtype):
    lo, hi = (eb.P_LO, eb.P_HI) if eb.is_packed(dtype) else (-99.0, 99.0)
    return {"open": (-INF, INF), "finite": (lo, hi), "finite_open": (lo, INF), "open_finite": (-INF, hi)}[kind]


def first_edge(dtype, sl):
    """Where the interior edges start: single-level recipes get edges no float32 holds, the others exact ones (packed: a stored value)."""
    if sl:
        return -25.15
    return pr._snap(-25.0) if eb.is_packed(dtype) else -25.0


def make_recipe(name, dtype, n_cells, bins, single_level, mean, seed=None) -> vr.Recipe:
    """`end_bins_recipes.make_recipe` with the cell boundaries among the values the data sit on."""
    r = eb.make_recipe(name, dtype, n_cells, bins, single_level, mean, seed=seed)
    return dataclasses.replace(r, edges=sorted(set(r.edges) | set(cells_of(bins)[2])))


def recipe(v) -> vr.Recipe:
    """The plan for cell-map histogram variant `v` (a tuple of gen_variants.cell_map_menu)."""
    v = vr.variant(v) if not isinstance(v, vr.Variant) else v
    assert v.pipe == 0 and v.has(vr.HB) and v.has(vr.TKI) and v.has(EB) and v.has(CM) and not v.has(vr.HA) and v.stat <= 1
    sl = v.has(vr.SL)
    n = 16 - v.stat - 2                                        # stat 1 adds a mean column (K <= 16); two end bins
    lo, hi = ends_for(ENDS[(int(sl), v.stat)], v.dtype)
    bins = partition(edges_from(first_edge(v.dtype, sl), WIDTHS[:n]), lo, hi)
    return make_recipe(v.name, v.dtype, eb.n_cells_for(v.dtype, v.vec), bins, sl, v.stat == 1)


def cube_for(r: vr.Recipe, seed=0):
    return eb.cube_for(r, seed)


def stored_cube(r: vr.Recipe, seed=0):
    return eb.stored_cube(r, seed)


def planted(r: vr.Recipe, values, q=None):
    """`end_bins_recipes.planted` (every value of `Recipe.edges`: bin edges AND cell boundaries) and, by name, what this form adds."""
    out = eb.planted(r, values, q)
    bins = eb.bins_of(r.columns)
    flat = values.reshape(-1)
    dt = values.dtype.type
    w, m, inner = cells_of(bins)
    out["cell boundaries that are no edge"] = len(inner) >= 3 and all(f"around {x}" in out for x in inner)
    for x in inner:                                            # such a value is strictly inside a bin: it must be counted
        near = np.abs(flat.astype(np.float64) - x) <= (0.01 if q is not None else 4 * abs(float(np.spacing(dt(x)))))
        out[f"at cell boundary {x}"] = bool(near.sum() >= 3)
    L, U = bins[0][0], bins[-1][1]
    if np.isfinite(L):
        out["on and beyond L"] = bool((flat < dt(L)).any() and (flat > dt(L)).any())
    if np.isfinite(U):
        out["on and beyond U"] = bool((flat > dt(U)).any() and (flat < dt(U)).any())
    return out
