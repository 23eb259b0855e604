"""One small plan per LDS-histogram kernel of the int16-packed menu (aggfly_amd/csrc/gen_variants.py: packed_hist_menu), beside
`packed_recipes`: a partition of thirteen to sixteen contiguous equal-width strict bins, a mean column for the stat-1 kernels, an
int16 cube around 12 C and the rule that unpacks it.

Pure Python and numpy.  How a recipe selects its variant (afhip_planner.cpp: choose_hist_variant): cells per lane by the row
length (even: two, odd: one); stat tier by the mean column; `sl` by identity outers with one period per inner group; `arith` by
edges the float32 edge fma reproduces exactly — E0 + 5 k, with E0 the VALUE of the stored integer nearest -20 C, so that at least
that edge is met exactly by a stored integer — and the edge table by edges no float32 holds (-19.85 + 3.1 k).

The data (`stored_cube`): what `packed_recipes.stored_cube_for` plants — per edge the stored integers nearest below and above,
+-32767 and -32768 (values far below the first and above the last edge: the guard bins), the fill in first rows of groups, in whole
groups and in whole cells — and, for every edge that IS the value of stored integers, those integers: a strict bin counts them
nowhere.
"""
from __future__ import annotations

import numpy as np

import packed_recipes as pr
import variant_recipes as vr

N_BINS = {(0, 0): 13, (0, 1): 16, (1, 0): 14, (1, 1): 15}      # (stat, single level) -> bins; stat 1 adds a mean column (K <= 16)


def arith_edges(n, width=5.0, near=-20.0, pairs=pr.PAIRS):
    """n + 1 edges E0 + k * width, E0 the value of the stored integer nearest `near`: every edge is a float32 and a stored value's."""
    e0 = float(pr.np_unpack([pr.stored_near(near, pairs)], pairs, None)[0])
    e = e0 + width * np.arange(n + 1)
    assert all(float(np.float32(x)) == x for x in e)
    return e


def table_edges(n, e0=-19.85, width=3.1):
    """n + 1 edges that float32 does not hold: the planner's exact-edge test fails and the plan takes the edge table."""
    e = e0 + width * np.arange(n + 1)
    assert not all(float(np.float32(x)) == x for x in e)
    return e


def bin_columns(edges, outer, mean=False, mean_outer="mean"):
    """The bins of the partition as columns, not in edge order (the kernel finds a column's bin through hb_bin_of_slot), then the mean."""
    n = len(edges) - 1
    order = [int(b) for b in np.random.default_rng(n).permutation(n)]
    cols = [dict(inner="bins", inner_args=(float(edges[b]), float(edges[b + 1]), 0.0), outer=outer) for b in order]
    if mean:
        cols.append(dict(inner="mean", outer="identity" if outer == "identity" else mean_outer))
    return cols


def groups(single_level):
    """(inner bounds, outer bounds): the long groups of `variant_recipes` (an empty one, lengths that are no multiple of a burst);
    eight outer periods of two-level plans, one period per group for `sl`."""
    lens = vr._inner_lengths("", 0)
    ib = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ob = np.arange(len(lens) + 1, dtype=np.int64) if single_level else vr._outer_bounds(len(lens), 8)
    return ib, ob


def recipe(v) -> vr.Recipe:
    """The plan for packed histogram variant `v` (a tuple of gen_variants.packed_hist_menu)."""
    v = vr.variant(v) if not isinstance(v, vr.Variant) else v
    assert v.dtype == pr.I16 and v.pipe == 0 and v.has(vr.HB) and v.has(vr.TKI) and v.stat <= 1
    sl = v.has(vr.SL)
    n = N_BINS[(v.stat, int(sl))]
    edges = arith_edges(n) if v.has(vr.HA) else table_edges(n)
    ib, ob = groups(sl)
    cols = bin_columns(edges, "identity" if sl else "sum", mean=v.stat == 1)
    return vr.Recipe(v.name, pr.I16, int(ib[-1]), pr.n_cells_for(v.vec), ib, ob, cols, True, 0, edges=[float(x) for x in edges])


def stored_on_edges(edges, pairs=pr.PAIRS):
    """{edge: the int16 stored integers whose value is exactly that edge}, searched over all 65,536 of them (edges that nothing
    meets are left out)."""
    q = np.arange(-32768, 32768).astype(np.int16)
    vals = pr.np_unpack(q, pairs, None)
    out = {}
    for e in edges:
        hit = q[vals == np.float32(e)]
        if float(np.float32(e)) == float(e) and hit.size:
            out[float(e)] = hit
    return out


def stored_cube(r: vr.Recipe, seed=0):
    """int16 [T, n_cells] for recipe `r` (see the module docstring)."""
    q = pr.stored_cube_for(r, seed)
    on = stored_on_edges(r.edges)
    if on:
        rng = np.random.default_rng(seed + 1)
        plant = np.concatenate([np.repeat(h, 6) for h in on.values()])
        keep = (q != pr.FILL) & (np.abs(q.astype(np.int32)) < 32766)      # (the planted fills and extremes stay)
        at = rng.choice(np.flatnonzero(keep.reshape(-1)), plant.size, replace=False)
        q.reshape(-1)[at] = plant
    return q
