"""The generator of the packed-cube fuzz (tests/test_gpu_packed_fuzz.py, tests/test_packed_fuzz_host.py, scripts/fuzz_more.py):
`case(seed)` gives, deterministically from the seed, an int16 / uint16 cube with one to four unpack rules along time, the float32
values a host computes from it, a time axis, a grid with its weights, and four to seven specs for `aggregate_dataset`.

Pure numpy / pandas: no GPU, no torch.cuda.  The time axes and the spec grammar are the float fuzz's (`test_gpu_fuzz._time_axes`,
`_random_steps`, `_dd`); the host values are `packed_recipes.np_unpack` / `test_gpu_unsigned.np_unpack` applied rule by rule to the
pairs that `folded_pairs` restates from the packing and the `preprocess` — nothing of them comes from the library under test.

Every stored field is ONE temperature field in kelvin (`synth.temperature_cube` + 273.15), quantised per rule, so a rule change
moves no value by more than the packings' steps; the `preprocess` (none, K -> C, K -> F) says in which unit the values, and with them
every threshold of the specs, are (`to_unit`).  Half of all thresholds are moved onto the float32 value of a stored integer under one
of the cube's rules (`stored_near`), and that integer with its two neighbours is planted in the rows of that rule.

Strata (`stratum_of`): a stratum pins what the planner's documented rule for a family of kernels asks for — the recipe modules'
docstrings state those rules — and leaves the rest to the seed:
  general        hourly steps (long date groups), the float fuzz's grammar
  short          unbroken 12- / 8- / 6-hourly steps, or such steps with single ones missing (date groups of mixed lengths, none empty);
                 every other trial draws lean columns only (mean | sum | min | max | sine_dd -> integer power -> sum | mean)
  hist-equal     a contiguous equal-width partition of six to fifteen bins and an optional mean, single level and two-level; edges
                 that float32 holds (from the value of a stored integer: the arithmetic-edge forms) and edges it does not (the table)
  hist-ends      the same between wide or open end bins (`end_bins_recipes.with_ends`)
  hist-cellmap   interior bins of unequal widths (`cell_map_recipes`), and per seed one partition the cell map does not take
                 (a width ratio beyond 127, or a gap): it must stay on the per-slot kernels
  wide           three names that lower to more than sixteen columns: more than one pass
  region-fused   3-hourly steps on 48 x 80 cells with a dozen regions; daily, weekly and monthly panels of up to six columns and
                 four threshold slots (`packed_rf_recipes`: the share of the period values and, on rows that are a multiple of
                 four, eight periods and more)
"""
from __future__ import annotations

import dataclasses
import hashlib

import numpy as np
import pandas as pd

from aggfly_amd import synth
from oracle import ref_aggregate as ra

import cell_map_recipes as cm
import end_bins_recipes as eb
import packed_hist_recipes as ph
import packed_recipes as pr
import test_gpu_unsigned as uns
from test_gpu_fuzz import _dd, _random_steps, _time_axes

SMALL_STRATA = ["general", "short", "hist-equal", "hist-ends", "hist-cellmap", "wide"]
SMALL_SEEDS = list(range(36))
RF_SEEDS = list(range(100, 108))
SEEDS = SMALL_SEEDS + RF_SEEDS
BOUNDARY_CLASSES = ("row 1", "row T-1", "inner-group boundary", "inside an inner group", "outer-period boundary", "two inside one inner group")
INF = float("inf")

# (scale_factor, add_offset) in kelvin: ERA5-like, scale only, a power of two without an offset; uint16: test_gpu_unsigned.py's
PACKINGS = {
    "int16": [(0.0017, 281.3), (0.01, None), (2.0 ** -6, None)],
    "uint16": [(0.001, 252.4), (0.1, 220.0), (0.01, None), (2.0 ** -7, None)],
}
FILLS = {"int16": [None, -32767, -32768], "uint16": [None, 65535, 0]}
RANGE = {"int16": (-32768, 32767), "uint16": (0, 65535)}
PREPROCESS = ["none", "celsius", "fahrenheit"]


def celsius(x):
    return x - 273.15


def fahrenheit(x):
    return (x - 273.15) * 1.8 + 32


PREPROCESS_FN = {"none": None, "celsius": celsius, "fahrenheit": fahrenheit}


def to_unit(c, preprocess):
    """A temperature in C in the unit the values of a cube under `preprocess` are in."""
    return {"none": c + 273.15, "celsius": c, "fahrenheit": c * 1.8 + 32.0}[preprocess]


def unit_step(preprocess):
    return 1.8 if preprocess == "fahrenheit" else 1.0


def folded_pairs(scale, offset, preprocess):
    """The (multiply, add) chain of a stored value under `preprocess`, by the rule aggfly_amd/packed.py documents: an addend joins the
    last pair when that has none, a factor opens a new pair."""
    pairs = [] if scale is None and offset is None else [(scale, offset)]
    ops = {"none": [], "celsius": [("add", -273.15)], "fahrenheit": [("add", -273.15), ("mul", 1.8), ("add", 32.0)]}[preprocess]
    for op, c in ops:
        if op == "mul":
            pairs.append((c, None))
        elif pairs and pairs[-1][1] is None:
            pairs[-1] = (pairs[-1][0], c)
        else:
            pairs.append((None, c))
    return pairs


def np_unpack(bits, pairs, fill, unsigned):
    """float32 values of the stored 16 bits (`bits`: int16) under one rule: `packed_recipes.np_unpack`, and test_gpu_unsigned.py's
    restatement for uint16."""
    if unsigned:
        return uns.np_unpack(np.asarray(bits, dtype=np.int16).view(np.uint16), pairs, fill)
    return pr.np_unpack(bits, pairs, fill)


def stored_near(value, pairs, unsigned):
    return uns.stored_near(value, pairs) if unsigned else pr.stored_near(value, pairs)


def value_of(s, pairs, unsigned):
    q = np.array([s], dtype=np.uint16).view(np.int16) if unsigned else np.array([s], dtype=np.int16)
    return float(np_unpack(q, pairs, None, unsigned)[0])


def host_values(bits, rule_pairs, fills, bounds, unsigned):
    """The multi-rule cube's values: rule by rule over its range of rows."""
    return np.concatenate([np_unpack(bits[lo:hi], p, f, unsigned) for p, f, lo, hi in zip(rule_pairs, fills, bounds[:-1], bounds[1:])])


def stratum_of(seed):
    return "region-fused" if seed >= 100 else SMALL_STRATA[(seed // 2) % len(SMALL_STRATA)]


@dataclasses.dataclass
class Case:
    seed: int
    stratum: str
    storage: str                 # "int16" | "uint16"
    preprocess: str              # "none" | "celsius" | "fahrenheit"
    rules: list                  # [(scale_factor, add_offset, fill)] per rule of the FULL cube
    bounds: list                 # rule bounds over the full cube's rows
    build: str                   # "concat" | "rules" | "zarr"
    bits: np.ndarray             # int16 [T_full, ny, nx]: the stored 16 bits
    full_time: object            # the product's time index of the full cube
    full_otime: object           # the oracle's
    window: tuple                # (lo, hi): the rows the trials run on (zarr seeds: a time selection across the first rule boundary)
    time: object                 # product time index of the window
    otime: object                # the oracle's
    host: np.ndarray             # float32 [T, ny, nx]: the host values of the window
    lat: np.ndarray
    lon: np.ndarray
    lon360: bool
    tab: pd.DataFrame
    trials: list                 # [{"spec": ..., "kind": ..., "expect": ...}]
    snapped: list                # [(threshold, rule, stored integer)]
    other_knob: bool             # also run under the other `exact_order`

    @property
    def unsigned(self):
        return self.storage == "uint16"

    @property
    def rule_pairs(self):
        return [folded_pairs(s, o, self.preprocess) for s, o, _ in self.rules]

    @property
    def n_pairs(self):
        return sorted({len(p) for p in self.rule_pairs})

    @property
    def window_bounds(self):
        lo, hi = self.window
        return [min(max(b, lo), hi) - lo for b in self.bounds]

    def boundary_classes(self):
        return classify_boundaries(self.full_otime, self.bounds)

    def digest(self):
        h = hashlib.sha1()
        for a in (self.bits, self.host, self.lat, self.lon, self.tab.to_numpy()):
            h.update(np.ascontiguousarray(a).tobytes())
        h.update(repr((self.rules, self.bounds, self.build, self.window, self.preprocess, self.snapped, _plain(self.trials))).encode())
        return h.hexdigest()


def _plain(x):
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


# ---------------------------------------------------------------------------------------------------------------------------
# time
# ---------------------------------------------------------------------------------------------------------------------------
def group_bounds(time):
    """(date bounds, month bounds) of a time index, as row positions [0, ..., T]."""
    y, m, d = (np.asarray(getattr(time, k)) for k in ("year", "month", "day"))
    day = y * 10000 + m * 100 + d
    mon = y * 100 + m
    ib = np.concatenate([[0], np.flatnonzero(np.diff(day)) + 1, [len(day)]])
    ob = np.concatenate([[0], np.flatnonzero(np.diff(mon)) + 1, [len(mon)]])
    return ib.astype(np.int64), ob.astype(np.int64)


def classify_boundaries(time, bounds):
    """The classes (BOUNDARY_CLASSES) of the inner rule bounds: inner groups are dates, outer periods months."""
    ib, ob = group_bounds(time)
    T = int(ib[-1])
    out, inside = set(), {}
    for b in bounds[1:-1]:
        if b == 1:
            out.add("row 1")
        if b == T - 1:
            out.add("row T-1")
        if b in ob:
            out.add("outer-period boundary")
        elif b in ib:
            out.add("inner-group boundary")
        else:
            out.add("inside an inner group")
            g = int(np.searchsorted(ib, b, side="right")) - 1
            inside[g] = inside.get(g, 0) + 1
    if any(n >= 2 for n in inside.values()):
        out.add("two inside one inner group")
    return out


def _place_boundaries(rng, seed, n_rules, time):
    ib, ob = group_bounds(time)
    T = int(ib[-1])
    long_groups = np.flatnonzero(np.diff(ib) >= 3)
    picked = set()

    def pick(cls):
        if cls == "row 1":
            return [1]
        if cls == "row T-1":
            return [T - 1]
        if cls == "outer-period boundary" and len(ob) > 2:
            return [int(rng.choice(ob[1:-1]))]
        if cls == "inner-group boundary":
            inner = np.setdiff1d(ib[1:-1], ob)
            return [int(rng.choice(inner))]
        if cls == "two inside one inner group" and len(long_groups):
            g = int(rng.choice(long_groups))
            return [int(ib[g]) + 1, int(ib[g]) + 2]
        wide = np.flatnonzero(np.diff(ib) >= 2)
        g = int(rng.choice(wide))
        return [int(rng.integers(ib[g] + 1, ib[g + 1]))]

    k = seed
    while len(picked) < n_rules - 1:
        cls = BOUNDARY_CLASSES[k % len(BOUNDARY_CLASSES)]
        k += 1
        new = [b for b in pick(cls) if 0 < b < T and b not in picked]
        picked.update(new[: n_rules - 1 - len(picked)])
    return [0] + sorted(picked) + [T]


# ---------------------------------------------------------------------------------------------------------------------------
# specs
# ---------------------------------------------------------------------------------------------------------------------------
class _Snapper:
    """Thresholds in the cube's unit; every other one moved onto the value of a stored integer under one of the rules."""

    def __init__(self, rng, rule_pairs, unsigned, preprocess, rows_of_rule):
        self.rng, self.rule_pairs, self.unsigned, self.preprocess = rng, rule_pairs, unsigned, preprocess
        self.rows_of_rule = rows_of_rule          # rules that have rows inside the window
        self.snapped = []
        self.n = 0

    def snap(self, value):
        """`value` (in the cube's unit) on the nearest stored value under a rule drawn among those of the window."""
        r = int(self.rng.choice(self.rows_of_rule))
        s = stored_near(value, self.rule_pairs[r], self.unsigned)
        v = value_of(s, self.rule_pairs[r], self.unsigned)
        self.snapped.append((v, r, int(s)))
        return v

    def threshold(self, c):
        """A threshold given in C."""
        v = float(to_unit(c, self.preprocess))
        self.n += 1
        return self.snap(v) if self.n % 2 else v

    def row(self, r):
        return [self.threshold(r[0]), self.threshold(r[1]), r[2]]

    def steps(self, steps):
        out = []
        for kind, p in steps:
            if kind == "aggregate" and "ddargs" in p:
                dd = p["ddargs"]
                p = dict(p, ddargs=[self.row(r) for r in dd] if isinstance(dd[0], list) else self.row(dd))
            out.append((kind, p))
        return out


def _general_spec(rng, sn, time, max_names=3):
    """The float fuzz's draw: one to three names of one output frequency."""
    out_freq, spec = None, {}
    for v in range(int(rng.integers(1, max_names + 1))):
        for _ in range(20):
            steps = _random_steps(rng)
            if not isinstance(time, pd.DatetimeIndex) and any(p.get("groupby") == "week" for k, p in steps if k == "aggregate"):
                continue
            last = [p["groupby"] for k, p in steps if k == "aggregate"][-1]
            if out_freq in (None, last):
                out_freq = last
                spec[f"v{v}"] = sn.steps(steps)
                break
    return spec


def _outer_choices(time):
    return ["month", "year"] + (["week"] if isinstance(time, pd.DatetimeIndex) else [])


def _lean_spec(rng, sn, time):
    """Lean columns only, six at the most: what the short-group kernels hold."""
    g2 = str(rng.choice(_outer_choices(time)))
    spec, k = {}, 0
    for v in range(int(rng.integers(1, 4))):
        inner = str(rng.choice(["mean", "sum", "min", "max", "sine_dd"]))
        p1 = {"calc": inner, "groupby": "date"}
        if inner == "sine_dd":
            lo = float(rng.choice([0, 5, 10, 12.5]))
            p1["ddargs"] = sn.row([lo, lo + float(rng.choice([10, 20])), int(rng.integers(0, 2))])
        steps = [("aggregate", p1)]
        n = 1
        if rng.random() < 0.5:
            n = int(rng.integers(2, 4))
            steps.append(("transform", {"transform": "power", "exp": np.arange(1, n + 1)}))
        if k + n > 6:
            break
        k += n
        steps.append(("aggregate", {"calc": str(rng.choice(["sum", "mean"])), "groupby": g2}))
        spec[f"v{v}"] = steps
    return spec


def _lattice(rng, sn, n, arith):
    """n + 1 equal-width edges in the cube's unit: from the value of a stored integer, every edge a float32 (`packed_hist_recipes.
    arith_edges`'s rule under this cube's packing), or ones that float32 does not hold (`table_edges`)."""
    u = unit_step(sn.preprocess)
    if not arith:
        return ph.table_edges(n, e0=float(to_unit(-19.85, sn.preprocess)) + 0.0137, width=3.1 * u)
    width = float(rng.choice([4.0, 5.0])) * (2.0 if u != 1.0 else 1.0)
    r = int(rng.choice(sn.rows_of_rule))
    s0 = stored_near(float(to_unit(-20.0, sn.preprocess)), sn.rule_pairs[r], sn.unsigned)
    for s in range(s0, s0 + 4096):
        e = value_of(s, sn.rule_pairs[r], sn.unsigned) + width * np.arange(n + 1)
        if all(float(np.float32(x)) == x for x in e):
            sn.snapped.append((float(e[0]), r, int(s)))
            return e
    raise AssertionError("no stored value starts a float32 lattice")


def _bins_spec(rng, time, bins, two_level, mean):
    g = str(rng.choice(_outer_choices(time)))
    order = [int(b) for b in rng.permutation(len(bins))]
    steps = [("aggregate", {"calc": "bins", "groupby": "date" if two_level else g, "ddargs": [[bins[b][0], bins[b][1], 0] for b in order]})]
    if two_level:
        steps.append(("aggregate", {"calc": "sum", "groupby": g}))
    spec = {"bins": steps}
    if mean:
        spec["tavg"] = ([("aggregate", {"calc": "mean", "groupby": "date"}), ("aggregate", {"calc": "mean", "groupby": g})] if two_level
                        else [("aggregate", {"calc": "mean", "groupby": g})])
    return spec


def _hist_trial(rng, sn, time, stratum, trial):
    two_level, mean = bool((trial + sn.rng.integers(0, 2)) % 2), bool(rng.random() < 0.5)
    arith = trial % 2 == 0
    expect = {"hist-equal": "hist", "hist-ends": "ends", "hist-cellmap": "cmap"}[stratum]
    if stratum == "hist-equal":
        e = _lattice(rng, sn, int(rng.integers(6, 16 - mean)), arith)
        bins = eb.with_ends(e)
    elif stratum == "hist-ends":
        kind = ["open", "finite", "lower", "upper"][int(rng.integers(0, 4))]
        lo_c, hi_c = {"open": (-INF, INF), "finite": (-40.0, 58.0), "lower": (-40.0, None), "upper": (None, INF)}[kind]
        n = int(rng.integers(5, 16 - mean - (lo_c is not None) - (hi_c is not None)))
        e = _lattice(rng, sn, n, arith)
        end = lambda c: None if c is None else (c if np.isinf(c) else sn.snap(float(to_unit(c, sn.preprocess))))      # noqa: E731
        bins = eb.with_ends(e, end(lo_c), end(hi_c))
    else:
        u = unit_step(sn.preprocess)
        e0 = float(to_unit(-25.15, sn.preprocess)) if trial % 2 else sn.snap(float(to_unit(-25.0, sn.preprocess)))
        if trial == 2:       # what the cell map does not take
            if rng.random() < 0.5:       # the range over the smallest width beyond 127
                widths = [10.0, 0.05, 9.95, 5.0, 2.5, 7.5]
                expect = "no-hist"
                bins = cm.partition(cm.edges_from(e0, [w * u for w in widths]), -INF, INF)
            else:                        # a gap
                bins = cm.partition(cm.edges_from(e0, [w * u for w in cm.WIDTHS[:6]]), -INF, INF)
                bins[3] = (bins[3][0], bins[3][1] - 0.5 * u)
                expect = "no-hist"
        else:
            k0 = int(rng.integers(0, 5))
            widths = [w * u for w in cm.WIDTHS[k0:k0 + int(rng.integers(4, 14 - mean - k0 + 1))]]
            lo, hi = [(-INF, INF), (-INF, sn.snap(float(to_unit(58.0, sn.preprocess)))), (sn.snap(float(to_unit(-40.0, sn.preprocess))), INF)][int(rng.integers(0, 3))]
            bins = cm.partition(cm.edges_from(e0, widths), lo, hi)
            if len(cm.distinct_widths(bins)) < 2:
                expect = "hist-any"
    return {"spec": _bins_spec(rng, time, bins, two_level, mean), "kind": stratum, "expect": expect}


def _wide_spec(rng, sn, time):
    """Three names, more than sixteen columns."""
    g2 = str(rng.choice(["month", "year"]))
    lo = float(rng.choice([-10.0, -5.0, 0.0]))
    w = float(rng.choice([5.0, 7.0]))
    n1, n2 = int(rng.integers(6, 9)), int(rng.integers(5, 8))
    rows1 = [sn.row([lo + w * k, lo + w * (k + 1), 0]) for k in range(n1)]
    rows2 = [sn.row([float(2 * k), 30.0, int(k % 2)]) for k in range(n2)]
    return {
        "bins": [("aggregate", {"calc": "bins", "groupby": "date", "ddargs": rows1}), ("aggregate", {"calc": "sum", "groupby": g2})],
        "dd": [("aggregate", {"calc": "dd", "groupby": "date", "ddargs": rows2}), ("aggregate", {"calc": str(rng.choice(["sum", "mean"])), "groupby": g2})],
        "tavg": [("aggregate", {"calc": str(rng.choice(["mean", "max", "nanmean"])), "groupby": "date"}),
                 ("transform", {"transform": "power", "exp": np.arange(1, 18 - n1 - n2)}),
                 ("aggregate", {"calc": "sum", "groupby": g2})],
    }


def _rf_spec(rng, sn, trial):
    """The float region-fused fuzz's draw with a panel frequency per trial: daily (one period per date group), weekly, monthly."""
    g2 = ["date", "week", "month"][trial % 3]
    spec, k = {}, 0
    for v in range(int(rng.integers(1, 4))):
        inner = str(rng.choice(["mean", "sum", "min", "max", "nanmean", "dd", "bins"]))
        p1 = {"calc": inner, "groupby": "date"}
        if inner in ("dd", "bins"):
            p1["ddargs"] = sn.row(_dd(rng, False))
        steps = [("aggregate", p1)]
        n = 1
        if g2 != "date" and rng.random() < 0.5 and inner not in ("dd", "bins"):
            n = int(rng.integers(2, 4))
            steps.append(("transform", {"transform": "power", "exp": np.arange(1, n)}))
            n -= 1
        if k + n > 6:
            break
        k += n
        if g2 != "date":
            outer = str(rng.choice(["sum", "mean", "min", "max", "dd"]))
            p2 = {"calc": outer, "groupby": g2}
            if outer == "dd":
                p2["ddargs"] = sn.row(_dd(rng, False))
            steps.append(("aggregate", p2))
        spec[f"v{v}"] = steps
    return spec


def _trials(rng, sn, time, stratum, n_trials):
    out = []
    for t in range(n_trials):
        if stratum == "region-fused":
            out.append({"spec": _rf_spec(rng, sn, t), "kind": "rf", "expect": None})
        elif stratum == "short" and t % 2 == 0:
            out.append({"spec": _lean_spec(rng, sn, time), "kind": "lean", "expect": None})
        elif stratum.startswith("hist-") and t < 3:
            out.append(_hist_trial(rng, sn, time, stratum, t))
        elif stratum == "wide" and t % 2 == 0:
            out.append({"spec": _wide_spec(rng, sn, time), "kind": "wide", "expect": "passes"})
        else:
            out.append({"spec": _general_spec(rng, sn, time), "kind": "general", "expect": None})
    return out


def resolve_inter(c: Case, spec, seed_key):
    """(oracle spec, product spec): an `inter` step's second array — random, of the inner level's shape, one NaN — filled in, as the
    float fuzz does."""
    rng = np.random.default_rng(seed_key)
    ny, nx = len(c.lat), len(c.lon)
    ods = ra.ODataset(c.host.astype(np.float64), c.otime, c.lat, c.lon, c.lon360)
    ospec, pspec = {}, {}
    for name, steps in spec.items():
        osteps, psteps = [], []
        for k, prm in steps:
            if k == "transform" and isinstance(prm.get("inter"), str) and prm["inter"] == "__OTHER__":
                with np.errstate(invalid="ignore", divide="ignore"):
                    inner = ra.OTemporalAggregator(**steps[0][1]).execute(ods)
                other = rng.normal(1.0, 0.5, inner.values.shape)
                other[rng.integers(0, other.shape[0]), rng.integers(0, ny), rng.integers(0, nx)] = np.nan
                osteps.append((k, dict(prm, inter=other)))
                psteps.append((k, dict(prm, inter=other.copy())))
            else:
                osteps.append((k, prm))
                psteps.append((k, prm))
        ospec[name], pspec[name] = osteps, psteps
    return ospec, pspec


# ---------------------------------------------------------------------------------------------------------------------------
# the cube
# ---------------------------------------------------------------------------------------------------------------------------
def _grid(rng, seed):
    """(ny, nx) with ny * nx = (seed + seed // 12) mod 4 (mod 4): four, two or one cells per lane; below or above one 256-thread
    workgroup's cells at that width (1024, 512, 256)."""
    res = (seed + seed // 12) % 4
    wg = {0: 1024, 2: 512, 1: 256, 3: 256}[res]
    above = bool(rng.integers(0, 2))
    lo, hi = (wg + 1, wg + 90) if above else (40, min(wg - 1, 400))
    for _ in range(10000):
        ny = int(rng.integers(4, 34))
        nx = int(rng.integers(4, 48))
        if lo <= ny * nx <= hi and (ny * nx) % 4 == res:
            return ny, nx
    raise AssertionError("no grid")


def _time_axis(rng, seed, stratum, zarr):
    """(spd, T, product index, oracle index, kept positions | None)."""
    cal_seed = 0 if zarr else 18 + seed % 3                       # (`_time_axes`: CF calendars from seed 16 on, by seed mod 3)
    if stratum == "region-fused":
        T = 8 * int(rng.integers(60, 100))
        t = pd.date_range("2001-01-01 00:00", periods=T, freq="3h")
        return 8, T, t, t, None
    if stratum == "short":
        form = ((seed // 12) * 2 + seed % 2) % 4
        spd = [2, 3, 4, int(rng.choice([2, 3, 4]))][form]
        T = spd * int(rng.integers(400, 800))
        if form < 3:             # unbroken: every date group has spd rows
            t = pd.date_range("2001-11-17 00:00", periods=T, freq=f"{24 // spd}h")
            return spd, T, t, t, None
        time, otime, keep = _time_axes(rng, T, spd, cal_seed, whole_days=False)
        return spd, T, time, otime, keep
    spd = 24 if stratum in ("general", "wide") or rng.random() < 0.6 else int(rng.choice([2, 4]))
    T = spd * int(rng.integers(70, 130)) + int(rng.integers(0, 24)) if spd == 24 else spd * int(rng.integers(400, 800))
    if seed % 4 == 1:            # unbroken, off the day's start
        t = pd.date_range("2001-11-17 05:00", periods=T, freq=f"{24 // spd}h")
        return spd, T, t, t, None
    time, otime, keep = _time_axes(rng, T, spd, cal_seed, whole_days=True)
    return spd, T, time, otime, keep


def _rules(rng, seed, storage, n_rules):
    packs, fills = PACKINGS[storage], FILLS[storage]
    rules, k = [], int(rng.integers(0, len(packs)))
    for i in range(n_rules):
        k = (k + int(rng.integers(1, len(packs)))) % len(packs)          # a neighbour never repeats a packing: no two rules merge
        rules.append((packs[k][0], packs[k][1], fills[(seed // 2 + i + int(rng.integers(0, 2))) % len(fills)]))
    return rules


def _quantise(kelvin, rules, bounds, storage):
    lo, hi = RANGE[storage]
    q = np.empty(kelvin.shape, dtype=np.int32)
    for (s, o, f), a, b in zip(rules, bounds[:-1], bounds[1:]):
        part = np.clip(np.rint((kelvin[a:b] - (o or 0.0)) / s), lo + 1, hi - 1).astype(np.int32)
        q[a:b] = part                                                     # (lo and hi themselves are planted below; a fill is one of them)
    return q


def case(seed) -> Case:
    rng = np.random.default_rng(77000 + seed)
    stratum = stratum_of(seed)
    storage = "uint16" if seed % 2 else "int16"
    unsigned = storage == "uint16"
    zarr = seed % 8 in (2, 5)
    n_rules = [2, 3, 4, 1, 3, 2, 4, 2][seed % 8]
    preprocess = PREPROCESS[(seed // 2 + seed // 6) % 3]
    spd, T, time, otime, keep = _time_axis(rng, seed, stratum, zarr)
    ny, nx = (48, 80) if stratum == "region-fused" else _grid(rng, seed)
    field = synth.temperature_cube(T, ny, nx, dtype=np.float64, seed=500 + seed, steps_per_day=spd, ocean_frac=0.1,
                                   scattered_nan=30 if stratum == "region-fused" else 15)
    if keep is not None:
        field = np.ascontiguousarray(field[keep])
        T = len(keep)
    missing = np.isnan(field)
    kelvin = np.where(missing, 283.15, field + 273.15)
    bounds = _place_boundaries(rng, seed, n_rules, otime) if n_rules > 1 else [0, T]
    rules = _rules(rng, seed, storage, len(bounds) - 1)
    if all(f is None for _, _, f in rules):
        big = int(np.argmax(np.diff(bounds)))
        rules[big] = (rules[big][0], rules[big][1], FILLS[storage][1 + seed // 2 % 2])
    big = int(np.argmax(np.diff(bounds)))
    if rules[big][2] is None:                                             # the longest rule has a fill: whole groups of it exist
        rules[big] = (rules[big][0], rules[big][1], FILLS[storage][1 + seed // 2 % 2])
    rule_pairs = [folded_pairs(s, o, preprocess) for s, o, _ in rules]
    lo_q, hi_q = RANGE[storage]
    q = _quantise(kelvin, rules, bounds, storage).reshape(T, ny * nx)
    C = ny * nx
    # the window of the trials
    if zarr:
        b0 = bounds[1]
        w0 = max(0, b0 - spd * int(rng.integers(10, 30)))
        w1 = T - int(rng.integers(1, 2 * spd))
        if stratum == "short":                                            # whole date groups: the selection leaves the group lengths alone
            days = group_bounds(otime)[0]
            w0, w1 = int(days[np.searchsorted(days, w0, side="right") - 1]), int(days[np.searchsorted(days, w1, side="right") - 1])
        window = (w0, max(w1, b0 + 1))
    else:
        window = (0, T)
    rows = np.arange(window[0], window[1])
    wtime, wotime = time[rows], otime[rows]
    in_window = [r for r, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])) if min(b, window[1]) > max(a, window[0])]
    # specs first: their snapped thresholds are planted
    sn = _Snapper(rng, rule_pairs, unsigned, preprocess, in_window)
    n_trials = 4 if (stratum == "region-fused" or C > 600) else int(rng.integers(4, 8 if C < 200 else 6))
    trials = _trials(rng, sn, wtime, stratum, n_trials)
    # planted: the extremes of the storage type, the snapped thresholds with their neighbours
    flat = q.reshape(-1)
    w_lo, w_hi = window[0] * C, window[1] * C
    ext = np.array([hi_q, lo_q, hi_q - 1, lo_q + 1] * 12)
    flat[rng.choice(np.arange(w_lo, w_hi), ext.size, replace=False)] = ext
    for v, r, s in sn.snapped:
        a, b = max(bounds[r], window[0]), min(bounds[r + 1], window[1])
        at = rng.integers(a * C, b * C, 9)
        flat[at] = np.clip([s, s, s, s + 1, s + 1, s - 1, s - 1, s, s], lo_q, hi_q)
    keep_value = np.zeros(q.shape, bool)                                  # (a snapped value of the first trial stays a value: no fill over it)
    for v, r, s in sn.snapped[:1]:
        a, b = max(bounds[r], window[0]), min(bounds[r + 1], window[1])
        t0 = int(rng.integers(a, b))
        c0 = int(rng.integers(0, C))
        q[t0, c0] = s
        keep_value[t0, c0] = True
    # the fill: where the field is missing, in first rows of date groups, whole date groups, whole cells (the last one included)
    ib, _ = group_bounds(otime)
    for (s_, o_, f), a, b in zip(rules, bounds[:-1], bounds[1:]):
        if f is None:
            continue
        own = q[a:b]
        own[own == f] = f + 1 if f == lo_q else f - 1                     # a value that quantised onto the fill moves one step
        m = np.zeros((b - a, C), bool)
        m |= missing.reshape(T, C)[a:b]
        groups = [g for g in range(len(ib) - 1) if ib[g] >= a and ib[g + 1] <= b]
        for g in groups[::5]:
            m[ib[g] - a, rng.choice(C, max(2, C // 40), replace=False)] = True
        for g in groups[2::7]:
            m[ib[g] - a:ib[g + 1] - a, rng.choice(C, min(4, C), replace=False)] = True
        m[:, [3, C // 2, C - 1]] = True
        m &= ~keep_value[a:b]
        own[m] = f
    big_a, big_b = bounds[big], bounds[big + 1]                           # one whole date group of fills inside the window, whatever the draws above
    gs = [g for g in range(len(ib) - 1) if ib[g] >= max(big_a, window[0]) and ib[g + 1] <= min(big_b, window[1])]
    if gs:
        g = gs[len(gs) // 2]
        blk = q[ib[g]:ib[g + 1], 1]
        if not keep_value[ib[g]:ib[g + 1], 1].any():
            blk[:] = rules[big][2]
    bits = (q.astype(np.uint16) if unsigned else q.astype(np.int16)).view(np.int16).reshape(T, ny, nx)
    fills = [f for _, _, f in rules]
    host = host_values(bits, rule_pairs, fills, bounds, unsigned)[window[0]:window[1]]
    lon360 = bool(seed % 3 == 0)
    if stratum == "region-fused":
        lat, lon = 10 + 0.5 * np.arange(ny), (200.0 if lon360 else -60.0) + 0.5 * np.arange(nx)
        tab = synth.weights_table(ny, nx, 12, seed=seed, secondary=bool(seed % 2), zero_frac=0.1)
        if seed % 4 >= 2:        # junctions of polygons: cells in up to five regions (test_gpu_fuzz.py)
            nreg = int(tab.index_right.max()) + 1
            jc = np.repeat(rng.choice(C, C // 33, replace=False), 3)[: int(rng.integers(C // 33, 3 * (C // 33)))]
            more = pd.DataFrame({"cell_id": jc, "index_right": rng.integers(0, nreg, len(jc)), "weight": rng.uniform(0.05, 0.9, len(jc))})
            tab = (pd.concat([tab[["cell_id", "index_right", "weight"]], more]).drop_duplicates(["index_right", "cell_id"])
                   .sort_values(["index_right", "cell_id"], kind="stable").reset_index(drop=True))
    else:
        lat, lon = -10 + 0.5 * np.arange(ny), (170.0 if lon360 else -30.0) + 0.5 * np.arange(nx)
        tab = synth.weights_table(ny, nx, max(2, min(C // 9, 40)), seed=seed, secondary=bool(seed % 2), zero_frac=0.15)
    build = "zarr" if zarr else ("concat" if (seed // 2) % 2 == 0 else "rules")
    return Case(seed, stratum, storage, preprocess, rules, bounds, build, bits, time, otime, window, wtime, wotime, host, lat, lon, lon360, tab,
                trials, sn.snapped, seed % 4 == 0)


def oracle_frame(c: Case, ospec):
    gr_ids = pd.Series([f"r{i}" for i in range(int(c.tab.index_right.max()) + 1)], name="geoid")
    ow = ra.OWeights(c.tab, np.arange(len(c.lat) * len(c.lon)), gr_ids, "geoid", "nan")
    ods = ra.ODataset(c.host.astype(np.float64), c.otime, c.lat, c.lon, c.lon360)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ra.aggregate_dataset(ow, ods, engine="numba", **ospec)
