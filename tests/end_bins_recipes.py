"""One small plan per LDS-histogram kernel for partitions with a wide end bin (aggfly_amd/csrc/gen_variants.py: end_bins_menu), beside
`variant_recipes`, `packed_recipes` and `packed_hist_recipes`: a run of equal-width strict bins between two end bins of another width —
finite (the -99 / 99 of the reference's own documents) or open (-inf / inf) — as float32, float64 and int16-packed plans.

Pure Python and numpy.  How a recipe selects its variant (afhip_planner.cpp: find_partition, choose_hist_variant): the storage by
the dtype; cells per lane by the row length (packed: even rows take two where the menu holds the form); stat tier by a mean column;
`sl` by identity outers with one period per inner group; `arith` by lattice edges the edge fma reproduces exactly in the input
precision (E0 + 5 k), the edge table by edges no float32 holds (-19.85 + 3.1 k); the `_ends` forms by the end bins, whose widths differ
from the lattice's.  Which ends a recipe gets (both open, both finite, one wide end only below / above) rotates with the form.

The data (`cube_for` / `stored_cube`): what the closed recipes plant, and around EVERY edge of the partition — the lattice's, the
first and last of them included, and the finite outer limits L / U — the value itself and its neighbours one to three steps to
either side (ulps of the cube's precision; for packed cubes stored integers), values far beyond, +-0 and, on float cubes, +-inf,
+-max and NaN; on packed cubes the fill and both extreme stored integers.  `planted` says which of these a cube holds.
"""
from __future__ import annotations

import numpy as np

import packed_hist_recipes as ph
import packed_recipes as pr
import variant_recipes as vr

EB = vr.gen_variants().Feat.END_BINS
INF = float("inf")
# the outer limits of the packed recipes: values of stored integers inside the storage's range (-47.5 ... 63.8 C), so that the cube
# holds values on them and beyond them
P_LO, P_HI = pr._snap(-40.0), pr._snap(58.0)


def is_packed(dtype):
    return dtype == pr.I16


def lattice(dtype, n, arith=True):
    """n + 1 equal-width edges: exactly representable ones (5 C from -20; packed: from the value of the stored integer nearest -20) or
    ones no float32 holds."""
    if not arith:
        return ph.table_edges(n)
    return ph.arith_edges(n) if is_packed(dtype) else -20.0 + 5.0 * np.arange(n + 1)


def with_ends(edges, lower=None, upper=None):
    """The bins (t0, t1) of the partition: the lattice `edges`, a wide lower end (lower, E[0]) and / or a wide upper end (E[n], upper)."""
    e = [float(x) for x in edges]
    bins = list(zip(e[:-1], e[1:]))
    if lower is not None:
        assert lower < e[0]
        bins.insert(0, (float(lower), e[0]))
    if upper is not None:
        assert upper > e[-1]
        bins.append((e[-1], float(upper)))
    return bins


def bin_columns(bins, outer, mean=False, seed=None):
    """The bins as columns in shuffled order (a column finds its bin, or its guard bin, through hb_bin_of_slot), then the mean."""
    order = [int(b) for b in np.random.default_rng(len(bins) if seed is None else seed).permutation(len(bins))]
    cols = [dict(inner="bins", inner_args=(bins[b][0], bins[b][1], 0.0), outer=outer) for b in order]
    if mean:
        cols.append(dict(inner="mean", outer="identity" if outer == "identity" else "mean"))
    return cols


def bins_of(columns):
    """The (t0, t1) rows of the bins columns, sorted."""
    return sorted({tuple(c["inner_args"][:2]) for c in columns if c["inner"] == "bins"})


def all_edges(columns):
    return sorted({x for b in bins_of(columns) for x in b})


def wide_ends(bins):
    """(lower is wide, upper is wide) of a sorted contiguous partition whose interior bins share one width."""
    b = sorted(bins)
    w = b[1][1] - b[1][0]
    return abs((b[0][1] - b[0][0]) - w) > 1e-9 * w, abs((b[-1][1] - b[-1][0]) - w) > 1e-9 * w


ENDS = {     # (single level, arithmetic edges) -> which ends the per-kernel recipe gets
    (0, 0): "open", (0, 1): "finite", (1, 0): "lower", (1, 1): "upper",
}


def ends_for(kind, dtype):
    lo, hi = (P_LO, P_HI) if is_packed(dtype) else (-99.0, 99.0)
    return {"open": (-INF, INF), "finite": (lo, hi), "lower": (lo, None), "upper": (None, INF),
            "lower_open": (-INF, None), "upper_finite": (None, hi)}[kind]


def n_cells_for(dtype, vec):
    if is_packed(dtype):
        return pr.n_cells_for(vec)
    return 60 if dtype == vr.F64 else 64                       # 6 x 10 and 4 x 16 cells: a partly filled wave and a full one


def make_recipe(name, dtype, n_cells, bins, single_level, mean, seed=None) -> vr.Recipe:
    ib, ob = ph.groups(single_level)
    cols = bin_columns(bins, "identity" if single_level else "sum", mean=mean, seed=seed)
    finite = [x for x in all_edges(cols) if np.isfinite(x)]
    return vr.Recipe(name, dtype, int(ib[-1]), n_cells, ib, ob, cols, True, 0, edges=finite)


def recipe(v) -> vr.Recipe:
    """The plan for end-bin histogram variant `v` (a tuple of gen_variants.end_bins_menu)."""
    v = vr.variant(v) if not isinstance(v, vr.Variant) else v
    assert v.pipe == 0 and v.has(vr.HB) and v.has(vr.TKI) and v.has(EB) and v.stat <= 1
    sl, ha = v.has(vr.SL), v.has(vr.HA)
    lo, hi = ends_for(ENDS[(int(sl), int(ha))], v.dtype)
    slots = 16 - v.stat                                        # stat 1 adds a mean column (K <= 16)
    n = slots - (lo is not None) - (hi is not None)
    bins = with_ends(lattice(v.dtype, n, ha), lo, hi)
    return make_recipe(v.name, v.dtype, n_cells_for(v.dtype, v.vec), bins, sl, v.stat == 1)


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def _steps(x, dt, k):
    """x moved k ulps (k < 0: down) in precision dt."""
    x = dt(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, dt(np.inf if k > 0 else -np.inf))
    return x


def cube_for(r: vr.Recipe, seed=0):
    """[T, n_cells] float32 / float64 for recipe `r` (see the module docstring)."""
    dt = np.float64 if r.dtype == vr.F64 else np.float32
    cube = vr.cube_for(r, seed)
    rng = np.random.default_rng(seed + 7)
    plant = []
    for e in r.edges:
        plant += [_steps(e, dt, k) for k in (-3, -2, -1, 0, 0, 1, 2, 3)]
    big = np.finfo(dt).max
    plant += [dt(0.0), dt(-0.0), dt(np.inf), dt(-np.inf), big, -big, dt(1e30), dt(-1e30), dt(np.nan), dt(250.0), dt(-250.0)] * 3
    plant = np.array(plant * 3, dtype=dt)
    lo, hi = min(r.edges), max(r.edges)
    inside = rng.uniform(lo - 2.0, hi + 2.0, cube.size // 10).astype(dt)          # a tenth of the cube spread over the whole partition
    flat = cube.reshape(-1)
    at = rng.choice(np.flatnonzero(~np.isnan(flat)), plant.size + inside.size, replace=False)      # (the NaN first rows, groups and cells stay as they are)
    flat[at[:inside.size]] = inside
    flat[at[inside.size:]] = plant
    return cube


def stored_cube(r: vr.Recipe, seed=0):
    """int16 [T, n_cells] for packed recipe `r` (see the module docstring)."""
    q = ph.stored_cube(r, seed)
    rng = np.random.default_rng(seed + 7)
    plant = [32767, -32768, 32766, -32766, pr.FILL] * 3
    for e in list(r.edges) + [0.0]:
        s = pr.stored_near(e)
        plant += [s + k for k in (-3, -2, -1, 0, 0, 1, 2, 3, 4)]
    for hit in ph.stored_on_edges(r.edges).values():
        plant += [int(h) for h in hit] * 3
    plant = np.clip(np.array(plant * 3), -32768, 32767).astype(np.int16)
    lo, hi = pr.stored_near(min(r.edges) - 2.0), pr.stored_near(max(r.edges) + 2.0)
    inside = rng.integers(lo, hi + 1, q.size // 10).astype(np.int16)
    flat = q.reshape(-1)
    at = rng.choice(np.flatnonzero(flat != pr.FILL), plant.size + inside.size, replace=False)      # (the fills of first rows, whole groups and cells stay as they are)
    flat[at[:inside.size]] = inside
    flat[at[inside.size:]] = plant
    return q


def planted(r: vr.Recipe, values, q=None):
    """{what: bool}: which of the listed values the cube `values` (in its own precision; packed: unpacked float32, `q` the stored
    integers) holds."""
    packed = q is not None
    dt = values.dtype.type
    flat = values.reshape(-1)
    bins = bins_of(r.columns)
    lo_w, hi_w = wide_ends(bins)
    L, U = bins[0][0], bins[-1][1]
    out = {}
    uniq = np.unique(flat[np.isfinite(flat)])
    for e in r.edges:
        if not packed:
            out[f"on {e}"] = bool((flat == dt(e)).any()) or float(dt(e)) != e
            out[f"around {e}"] = all((flat == _steps(e, dt, k)).any() for k in (-3, -2, -1, 1, 2, 3))
        else:
            i = int(np.searchsorted(uniq, np.float32(e)))
            out[f"around {e}"] = 3 <= i <= uniq.size - 4                  # three stored values and more on either side of the edge
            if float(np.float32(e)) == e and (pr.np_unpack(np.arange(-32768, 32768).astype(np.int16), fill=None) == np.float32(e)).any():
                out[f"on {e}"] = bool((flat == np.float32(e)).any())
    if lo_w and np.isfinite(L):
        out["beyond L"] = bool((flat < dt(L)).any())
    if hi_w and np.isfinite(U):
        out["beyond U"] = bool((flat > dt(U)).any())
    out["far below"] = bool((flat < dt(min(r.edges) - 5.0)).any())
    out["far above"] = bool((flat > dt(max(r.edges) + 5.0)).any())
    if packed:
        have = set(np.unique(q).tolist())
        out["extremes and fill"] = {32767, -32768, pr.FILL} <= have
        out["zero"] = pr.stored_near(0.0) in have
    else:
        out["zeros"] = bool(((flat == 0) & np.signbit(flat)).any() and ((flat == 0) & ~np.signbit(flat)).any())
        out["inf"] = bool(np.isposinf(flat).any() and np.isneginf(flat).any())
        out["max"] = bool((flat == np.finfo(dt).max).any() and (flat == -np.finfo(dt).max).any())
    out["nan"] = bool(np.isnan(flat).any())
    ib = r.inner_bounds
    v2 = values.reshape(r.T, -1)
    out["a whole group of NaN"] = any(np.isnan(v2[ib[g]:ib[g + 1]]).all(axis=0).any() for g in range(len(ib) - 1) if ib[g + 1] > ib[g])
    out["an empty group"] = bool((np.diff(ib) == 0).any())
    return out


def in_some_bin(r: vr.Recipe, values):
    """[T, cells] bool: the value lies strictly inside the partition (L < v < U) and on none of its edges — such a step is counted by
    exactly one bin of its cell, every other step by none."""
    bins = bins_of(r.columns)
    v = values.reshape(r.T, -1).astype(np.float64)
    inside = (v > bins[0][0]) & (v < bins[-1][1])
    for e in all_edges(r.columns):
        inside &= v != e
    return inside
