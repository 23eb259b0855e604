"""One small plan per production kernel variant (aggfly_amd/csrc/gen_variants.py), shaped to land on that variant at the edge
of its template: as many columns as it holds (K == kmax) and its threshold-slot tier filled as far as the spec grammar allows.

Pure Python and numpy: `tests/test_host_logic.py` checks the recipes' shapes without a GPU, `tests/test_gpu_variant_menu.py`
runs each one against the oracle.  A recipe leaves the planner its default choice (`tuning == 0`, no environment knobs), with
one exception: the float32 two-cells-per-lane kernels with four rows in flight (depth 4), which the planner takes only on grids
of at least cu_count * 2 * WG cells, are pinned with tuning=204 (direct loads, two cells per lane, depth 4).

How a recipe selects its variant (afhip_planner.cpp: build_plan and its stages):
  statistic tier   stat 3: a `nanmean` source;  stat 2: `min` / `max` / `sine_dd`;  stat 1: `mean` / `sum`;  stat 0: thresholds only
  slot tier        distinct `dd` / `bins` argument rows (each column adds at most one, so nthr <= K; nthr <= K - 1 beside a mean /
                   sum / min / max / sine_dd source).  Stat 3 with every column a threshold: a non-integer pow on one of them
  column tier      K == kmax where the slot tier allows it; f32 two cells per lane needs nthr < 4 and K < 8 (K = 7 for a k16 kernel)
  cells per lane   f32: an even cell count for vec 2, an odd one for vec 1 wherever the planner would otherwise take two
  load path        pipe 1: short generic groups (mean below 8 rows for f32, 4 for f64), no sine, n_cells % (16 / elem) == 0
  tki / hb / ha    every slot a `bins` row; hb: a contiguous equal-width partition of 4 or more bins; ha: exactly representable
                   edges (integers); hb without ha: edges 0.15 + 0.7 k, which neither float32 nor the edge fma reproduce
  sl               identity outer reducers and one output period per inner group (exact_order keeps it off the twin route)
  pair forms       inner groups of exactly 2 / 4 / 3 rows (pair / quad / tri) or mixed 1-4 rows (rag); ss: lean columns
                   (mean | sum | min | max | sine_dd -> integer power -> sum | mean); ss=2: plain sine_dd columns, K <= 2
  rf twins         the base variant's recipe with several short periods and exact_order=False: run against a CSR, the plan
                   takes the region-fused route
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG = 256                     # afhip_kernels.h
F32, F64 = 0, 1              # include/aggfly_hip.h


def gen_variants():
    path = os.path.join(ROOT, "aggfly_amd", "csrc")
    if path not in sys.path:
        sys.path.insert(0, path)
    import gen_variants as gv
    return gv


# FEAT bits (gen_variants.py)
_F = gen_variants().Feat
NT, TKI, SL, HB, HA, PAIR, LEAN, SS2 = _F.NT, _F.INT_BINS, _F.SINGLE_LEVEL, _F.HIST, _F.ARITH_EDGES, _F.SHORT_GROUP, _F.LEAN, _F.LEAN_SINE
QUAD, RF, TRI, RAG = _F.FOUR_ROW, _F.REGION_FUSED, _F.THREE_ROW, _F.MIXED


def menu_of(key, kind="full"):
    """The tuples of the kernel menu `key` (gen_variants.py: MENUS — "float", "packed", "packed_hist", "end_bins") of the build `kind`
    ("full" / "arms" / "dev"), in table order."""
    return list({k: fn for k, fn, _ in gen_variants().MENUS}[key](kind))


def production_menu(kind="full"):
    """The production entries of the float menu of `kind`, in table order."""
    return [v for v in menu_of("float", kind) if v[8]]


def loaded_menu_kind():
    """The menu kind of the library the tests load (collection time: the parametrised cases are one per kernel of that build)."""
    try:
        from aggfly_amd import hip
        return hip.build_info()["menu"]
    except Exception:          # no library at collection time: the cases fail on their own, in torch_cuda / FusedPlan
        return "full"


def plan_name(plan):
    """The name of the kernel variant a FusedPlan landed on."""
    return plan.describe().split()[0][len("variant="):]


@dataclass
class Variant:
    name: str
    dtype: int
    pipe: int
    vec: int
    stat: int
    nthr: int
    kmax: int
    depth: int
    feat: int

    def has(self, bit):
        return bool(self.feat & bit)

    @property
    def form(self):
        """Inner-group form: 'pair' (2 rows), 'quad' (4), 'tri' (3), 'rag' (1-4 mixed) or '' (any)."""
        if not self.has(PAIR):
            return ""
        return "quad" if self.has(QUAD) else "tri" if self.has(TRI) else "rag" if self.has(RAG) else "pair"

    @property
    def lean(self):
        return 2 if self.has(SS2) else 1 if self.has(LEAN) else 0


def variant(v) -> Variant:
    dtype, pipe, vec, stat, nthr, kmax, depth, feat, _ = v
    return Variant(gen_variants().name_of(v), dtype, pipe, vec, stat, nthr, kmax, depth, feat)


@dataclass
class Recipe:
    name: str                       # the variant the plan must select (its describe() name; a twin's base for an `_rf` variant)
    dtype: int
    T: int
    n_cells: int
    inner_bounds: np.ndarray
    outer_bounds: np.ndarray
    columns: list
    exact_order: bool
    tuning: int
    region_fused: bool = False      # an `_rf` twin: run against a CSR, the plan must take the region-fused route
    edges: list = field(default_factory=list)      # threshold / bin / hinge edges: the data sit on them and next to them
    sine_edges: list = field(default_factory=list)  # sine_dd thresholds: the data sit on them (see cube_for)


# ---------------------------------------------------------------------------------------------------------------------------
# group lengths per form (none a multiple of the burst depth throughout; an empty group where the form allows one)
# ---------------------------------------------------------------------------------------------------------------------------
_LONG = [9, 13, 0, 11, 7, 10, 12, 1, 14, 10, 11, 9]      # mean 8.9 rows: the direct-load path
_SHORT = [3, 5, 0, 2, 4, 1, 6, 3, 2, 4, 3, 2]            # mean 2.9 rows, not all of 1-4: the LDS-DMA ring, no short-group form
_RAG = [4, 1, 3, 4, 2, 4, 4, 1, 3, 2, 4, 3]              # 1-4 rows, length-1 groups


def _inner_lengths(form, pipe):
    if form == "pair":
        return [2] * 150
    if form == "quad":
        return [4] * 75
    if form == "tri":
        return [3] * 101                                   # an odd number of groups: a lone group in the last block of six rows
    if form == "rag":
        return _RAG * 10
    return _SHORT * 8 if pipe == 1 else _LONG * 3


def _outer_bounds(G1, per=8):
    """Periods of `per` groups (all well under 128 steps: never split over chunks), the second one empty."""
    ob = [0, per, per]
    while ob[-1] + per < G1:
        ob.append(ob[-1] + per)
    ob.append(G1)
    return np.array(ob, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------------------------------
# columns
# ---------------------------------------------------------------------------------------------------------------------------
def _dd_rows(n):
    """n distinct degree-day rows, both base flags."""
    return [(float(-6 + 2 * i), float(-6 + 2 * i + 9 + (i % 3)), float(i % 2)) for i in range(n)]


def _bin_rows(n, kind):
    """n bins: 'overlap' (integer edges, no partition), 'arith' (a partition of width 2 with integer edges), 'inexact' (a partition
    of width 0.7 from 0.15: edges no float32 holds, and no exact edge fma)."""
    if kind == "overlap":
        return [(float(-10 + 3 * i), float(-10 + 3 * i + 7), 0.0) for i in range(n)]
    e = (-12.0 + 2.0 * np.arange(n + 1)) if kind == "arith" else (0.15 + 0.7 * np.arange(-12, n - 11))
    return [(float(e[i]), float(e[i + 1]), 0.0) for i in range(n)]


def _threshold_columns(v: Variant, nslots):
    """nslots columns with distinct threshold rows; at least one `dd` row unless the variant needs bins only (tki)."""
    if nslots == 0:
        return []
    if v.has(TKI):
        kind = ("arith" if v.has(HA) else "inexact") if v.has(HB) else "overlap"
        return [dict(inner="bins", inner_args=r) for r in _bin_rows(nslots, kind)]
    rows = _dd_rows(nslots)
    cols = [dict(inner="dd", inner_args=rows[0])]
    for i, r in enumerate(rows[1:]):       # a bins row now and then beside the degree days
        cols.append(dict(inner="bins" if i % 3 == 2 else "dd", inner_args=r))
    return cols


def _stat_sources(v: Variant):
    if v.stat == 1:
        return [dict(inner="mean"), dict(inner="sum")]
    if v.stat == 2:
        if v.lean == 2:
            return [dict(inner="sine_dd", inner_args=(10.0, 30.0, 0.0)), dict(inner="sine_dd", inner_args=(5.0, 18.0, 1.0))]
        src = [dict(inner="max"), dict(inner="min")]
        if v.pipe == 0:                    # sine_dd keeps a plan off the LDS-DMA ring
            src.insert(1, dict(inner="sine_dd", inner_args=(10.0, 30.0, 0.0)))
        return src + [dict(inner="mean")]
    if v.stat == 3:
        return [dict(inner="nanmean"), dict(inner="max"), dict(inner="mean")]
    return []


def _fanouts():
    """Transforms for columns beyond the distinct sources: even integer powers (no cancellation in their sums) and a hinge."""
    return [dict(transform="pow", transform_arg=2.0), dict(transform="hinge", transform_arg=20.0), dict(transform="pow", transform_arg=4.0)]


def _shape(v: Variant):
    """(slots, K) at the edge of the variant's template."""
    k_lo = {2: 1, 6: 3, 16: 7}[v.kmax]
    K = v.kmax
    if v.dtype == F32 and v.vec == 2 and v.pipe == 0:
        K = min(K, 7)                                      # two cells per lane: K < 8
    if v.nthr == 0:
        return 0, K
    n_lo = {1: 1, 4: 2, 16: 5}[v.nthr]
    n = min(v.nthr, K - (1 if v.stat in (1, 2) else 0))     # stat 3: all K columns may be thresholds (see _columns)
    if v.dtype == F32 and v.vec == 2 and v.pipe == 0:
        n = min(n, 3)                                      # ... and fewer than four slots
    if n < n_lo or K < k_lo:
        raise ValueError(f"{v.name}: no plan fills this template (slots {n} < {n_lo} or columns {K} < {k_lo})")
    return n, K


def _columns(v: Variant, nslots, K, single_level):
    thr = _threshold_columns(v, nslots)
    if v.stat == 3 and nslots == K:                       # no room for a nanmean: the first degree-day column -> x ** 1.5 sets stat 3
        thr[0] = dict(thr[0], transform="pow", transform_arg=1.5)
    src = _stat_sources(v)[:K - nslots]
    base = thr + src
    outers = ["identity"] if single_level else (["sum", "mean"] if v.lean else ["sum", "mean", "max", "min"])
    cols = []
    for i, c in enumerate(base):
        cols.append(dict(c, outer=outers[i % len(outers)]))
    fan, i = _fanouts(), 0
    while len(cols) < K:                                  # fan-outs of the sources (a threshold row repeated shares its slot)
        c = dict(base[i % len(base)])
        f = fan[(i // len(base)) % len(fan)]
        if v.lean and f["transform"] == "hinge":
            f = dict(transform="pow", transform_arg=3.0 if c["inner"] in ("sine_dd", "sum") else 2.0)
        cols.append(dict(c, **f, outer=outers[(len(cols) + 1) % len(outers)]))
        i += 1
    if v.form and not v.lean:                              # the general short-group form: one column the lean form cannot take
        cols[-1] = dict(cols[-1], outer="max")
    return cols


def _n_cells(v: Variant, nslots, K):
    """A multiple of the vector width but not of WG * vec, more than one workgroup; odd where a float32 plan would otherwise
    take two cells per lane."""
    if v.pipe == 1:
        return 1100                                       # multiple of 4 (LDS-DMA rows of 16 bytes), not of 256 * vec
    if v.dtype == F32 and v.vec == 1 and not v.has(HB):
        two = nslots < 4 and K < 8 and not (v.stat <= 1 and nslots == 0 and K <= 2)
        if two:
            return 1101
    if v.dtype == F32 and v.vec == 2:
        return 1102                                       # even, not a multiple of 4 (no LDS-DMA ring)
    return 1101 if v.dtype == F64 and not v.form else 1102


def recipe(v) -> Recipe:
    """The plan for production variant `v` (a menu tuple of gen_variants.menu)."""
    v = variant(v) if not isinstance(v, Variant) else v
    if v.has(RF):
        base = variant_of(v, v.feat & ~RF)
        r = recipe(base)
        r.exact_order = False
        r.region_fused = True
        return r
    single_level = v.has(SL)
    nslots, K = _shape(v)
    lens = _inner_lengths(v.form, v.pipe)
    ib = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    G1 = len(lens)
    ob = np.arange(G1 + 1, dtype=np.int64) if single_level else _outer_bounds(G1, 8 if v.form in ("", "rag") else 10)
    cols = _columns(v, nslots, K, single_level)
    tuning = 204 if (v.dtype == F32 and v.pipe == 0 and v.vec == 2 and v.depth == 4 and not v.form) else 0
    edges, sine = set(), set()
    for c in cols:
        if c["inner"] in ("dd", "bins"):
            edges.update(c["inner_args"][:2])
        if c["inner"] == "sine_dd":
            sine.update(c["inner_args"][:2])
        if c.get("transform") == "hinge":
            edges.add(c["transform_arg"])
    return Recipe(v.name, v.dtype, int(ib[-1]), _n_cells(v, nslots, K), ib, ob, cols, True, tuning, edges=sorted(edges), sine_edges=sorted(sine))


def variant_of(v: Variant, feat) -> Variant:
    for t in production_menu():
        w = variant(t)
        if (w.dtype, w.pipe, w.vec, w.stat, w.nthr, w.kmax, w.depth, w.feat) == (v.dtype, v.pipe, v.vec, v.stat, v.nthr, v.kmax, v.depth, feat):
            return w
    raise KeyError(f"{v.name}: no base variant in the production menu")


def slots_of(columns):
    """Distinct threshold slots a column list lowers to (afhip_planner.cpp: add_thr_slot)."""
    return len({(c["inner"], tuple(c["inner_args"])) for c in columns if c["inner"] in ("dd", "bins")})


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def cube_for(r: Recipe, seed=0):
    """[T, n_cells] in the recipe's dtype: quarter-degree temperatures around 12 C, every edge planted (the value itself in the
    cube's precision and, for the exact compares of dd / bins / hinge, its neighbours on both sides), values below the first and
    above the last edge, NaN in some groups' first rows, whole NaN groups and ocean cells.  (A float64 value one ulp from a sine_dd
    threshold puts the closed forms where the oracle's libm arithmetic loses digits: DESIGN.md §5 holds sine_dd to 50-digit values
    there, tests/test_gpu_sine_fixtures.py.)"""
    dt = np.float64 if r.dtype == F64 else np.float32
    rng = np.random.default_rng(seed)
    T, C = r.T, r.n_cells
    cube = np.round(rng.normal(12.0, 9.0, (T, C)) * 4) / 4
    cube = cube.astype(dt)
    flat = cube.reshape(-1)
    plant = []
    for e in r.edges:
        ev = dt(e)
        plant += [ev, ev, np.nextafter(ev, dt(np.inf)), np.nextafter(ev, dt(-np.inf))]
    plant += [dt(e) for e in r.sine_edges for _ in range(4)]
    every = r.edges + r.sine_edges
    if every:
        plant += [dt(min(every) - 3.5), dt(max(every) + 3.5), dt(min(every) - 40.0), dt(max(every) + 40.0)]
    plant = np.array(plant * max(1, 2000 // max(len(plant), 1)), dtype=dt)
    flat[rng.choice(flat.size, plant.size, replace=False)] = plant
    ib = r.inner_bounds
    ne = np.flatnonzero(np.diff(ib) > 0)
    for g in ne[::5]:                                    # NaN in the first row of a group, for some cells
        cube[ib[g], rng.choice(C, 25, replace=False)] = np.nan
    for g in ne[2::7]:                                   # whole NaN groups
        cube[ib[g]:ib[g + 1], rng.choice(C, 4, replace=False)] = np.nan
    cube[:, [3, C // 2, C - 1]] = np.nan                 # ocean cells, the last one included
    return cube
