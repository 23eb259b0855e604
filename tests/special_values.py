"""What a group holds: windows of degenerate and special values for every kernel form, and a compare that sees them.

Host-only (numpy).  `window` builds the `L` rows of one inner group for a class of values; `class_cube` fills a recipe's own
inner groups with them, one class per cell (cell `c` holds class `c % n_classes`), so the plan still selects the recipe's kernel;
`packed_class_cube` is the twin for stored integers.  `assert_same_kind` is the compare: NaN in the same places, infinities in
the same places with their sign, zeros with their sign where the bar is bit-exact, and the finite values at the given bar —
`np.testing.assert_array_equal` takes 0.0 == -0.0.

The classes (a class that needs more rows than the group has falls back to `flat`; `NEEDS` says how many):
  control     ordinary quarter-degree values
  flat        all rows equal; the value cycles with g over an edge of the plan, 12.25, +0.0 and -0.0
  ties        minimum and maximum attained twice each, one of them in the first and the last row, the other next to them
  zeros_pn    +0.0, -0.0, +0.0, ...            zeros_np    -0.0, +0.0, -0.0, ...
  on_edges    every row one of `edges` (dd / bins / hinge / sine thresholds), cycling
  pinf, ninf  one infinite row, the rest ordinary
  both_inf    +inf and -inf: the sum is NaN without a NaN among the rows
  subnormal   + and - the smallest subnormal of the dtype among zeros
  overflow    float64: two rows of finfo.max, the group sum is +inf (one sign only: weighted sums over cells of both signs would
              overflow or not by the order of their adds);  float32: +-finfo(float32).max in turn — the float64 sum stays finite,
              the float32 store of a sum overflows
  nan_last    a NaN in the last row only       nan_mid     in one middle row only       one_valid   everywhere but one row
`g` moves the special rows through the window, so that first, middle and last rows are all met.

The kernels take an inner min / max with the hardware's min / max instructions, which order -0 < +0; the reference's
`if v < mn: mn = v` keeps the zero it saw first.  `hardware_zero_rule` turns the oracle's inner min / max into the
kernels' on groups that hold zeros of both signs; nothing else differs.
"""
from __future__ import annotations

import numpy as np

CLASSES = ("control", "flat", "ties", "zeros_pn", "zeros_np", "on_edges", "pinf", "ninf", "both_inf", "subnormal", "overflow",
           "nan_last", "nan_mid", "one_valid")
NEEDS = {"ties": 4, "both_inf": 2, "overflow": 2, "nan_mid": 3}        # rows a class needs (every other class: one)
SINE_UNDEFINED = ("pinf", "ninf", "both_inf", "overflow")              # the closed forms subtract infinities: outside sine_dd's contract
PACKED_CLASSES = ("control", "flat", "ties", "on_edges", "fill_last", "fill_mid", "one_valid", "extremes")
PACKED_NEEDS = {"ties": 4, "fill_mid": 3, "extremes": 2}
ROTATIONS = 8                                                           # cells of a class differ in how far their windows are rotated


def _ordinary(L, g, dt):
    """L quarter-degree values around 12 C, no two neighbours equal, different from group to group."""
    i = np.arange(L)
    return (12.25 + (((7 * g + 5 * i) % 23) - 11) * 0.75).astype(dt)


def effective_class(cls, L, edges=(), needs=NEEDS):
    """The class a window of L rows really holds: `flat` where the class needs more rows (or edges) than there are."""
    if L < needs.get(cls, 1) or (cls == "on_edges" and not len(edges)):
        return "flat"
    return cls


def window(cls, L, dtype, edges, g):
    """L values of class `cls` for inner group number `g` (see the module docstring)."""
    dt = np.dtype(dtype).type
    if L == 0:
        return np.empty(0, dtype=dt)
    cls = effective_class(cls, L, edges)
    w = _ordinary(L, g, dt)
    if cls == "control":
        return w
    if cls == "flat":
        choice = [dt(edges[(g // 4) % len(edges)]) if len(edges) else dt(12.25), dt(12.25), dt(0.0), dt(-0.0)][g % 4]
        return np.full(L, choice, dtype=dt)
    if cls == "ties":
        lo, hi = dt(-3.5), dt(27.75)
        w = np.clip(w, dt(0.0), dt(24.0))                   # strictly between the tied extremes
        a, b = (lo, hi) if g % 2 == 0 else (hi, lo)
        w[0], w[1], w[L - 2], w[L - 1] = a, b, b, a
        return w
    if cls in ("zeros_pn", "zeros_np"):
        first = 0 if cls == "zeros_pn" else 1
        return np.where((np.arange(L) + first) % 2 == 0, dt(0.0), dt(-0.0)).astype(dt)
    if cls == "on_edges":
        return np.array([edges[(g + i) % len(edges)] for i in range(L)], dtype=dt)
    if cls == "pinf":
        w[g % L] = np.inf
        return w
    if cls == "ninf":
        w[g % L] = -np.inf
        return w
    if cls == "both_inf":
        w[g % L], w[(g + 1) % L] = np.inf, -np.inf
        return w
    if cls == "subnormal":
        tiny = np.nextafter(dt(0.0), dt(1.0))
        w = np.zeros(L, dtype=dt)
        if L == 1:
            w[0] = tiny if g % 2 == 0 else -tiny
        else:
            w[g % L], w[(g + 1) % L] = tiny, -tiny
        return w
    if cls == "overflow":
        if dt is np.float64:
            big = np.finfo(np.float64).max
            w[g % L], w[(g + 1) % L] = big, big
        else:
            big = np.finfo(np.float32).max
            sign = dt(1.0) if g % 2 == 0 else dt(-1.0)
            w[g % L], w[(g + 1) % L] = sign * big, sign * big
        return w
    if cls == "nan_last":
        w[L - 1] = np.nan
        return w
    if cls == "nan_mid":
        w[1 + g % (L - 2)] = np.nan
        return w
    if cls == "one_valid":
        keep = w[g % L]
        w[:] = np.nan
        w[g % L] = keep
        return w
    raise KeyError(cls)


def _fill_by_class(out, ib, n_classes, make):
    """out[T, C]: cell c's group g <- make(class index c % n_classes, L, g + 2 * ((c // n_classes) % ROTATIONS))[rows].  (An even
    shift: what a class decides by the parity of g — the sign of float32's overflow rows — is the same in every cell of a group, so
    weighted sums over cells do not cancel at 1e38.)"""
    C = out.shape[1]
    for g in range(len(ib) - 1):
        lo, hi = int(ib[g]), int(ib[g + 1])
        if hi == lo:
            continue
        for k in range(n_classes):
            for r in range(ROTATIONS):
                cells = np.arange(k + r * n_classes, C, n_classes * ROTATIONS)
                if len(cells):
                    out[lo:hi, cells] = make(k, hi - lo, g + 2 * r)[:, None]


def class_cube(recipe):
    """(cube [T, n_cells] in the recipe's dtype, class_of_cell [n_cells] of class names) for a `variant_recipes.Recipe`: the recipe's
    own inner groups, every class in every group, edges = recipe.edges + recipe.sine_edges."""
    dt = np.float64 if recipe.dtype == 1 else np.float32          # include/aggfly_hip.h: AFHIP_F64 == 1
    edges = list(recipe.edges) + list(recipe.sine_edges)
    cube = np.empty((recipe.T, recipe.n_cells), dtype=dt)
    _fill_by_class(cube, recipe.inner_bounds, len(CLASSES), lambda k, L, g: window(CLASSES[k], L, dt, edges, g))
    return cube, np.array([CLASSES[c % len(CLASSES)] for c in range(recipe.n_cells)])


def packed_window(cls, L, stored_edges, g, fill, centre, per_degree, limits=(-32768, 32767)):
    """L stored integers of class `cls` for group `g`.  `stored_edges`: the stored integers whose values are nearest the plan's edges;
    `centre` / `per_degree`: the stored integer of 12 C and stored steps per degree; `fill`: the fill value; `limits`: the storage's
    extreme integers.  No infinities, signed zeros or subnormals: the storage cannot hold them."""
    if L == 0:
        return np.empty(0, dtype=np.int64)
    cls = effective_class(cls, L, stored_edges, PACKED_NEEDS)
    i = np.arange(L)
    w = np.rint(centre + (((7 * g + 5 * i) % 23) - 11) * 0.75 * per_degree).astype(np.int64)
    w[w == fill] += 1
    if cls == "control":
        return w
    if cls == "flat":
        near = stored_edges[(g // 3) % len(stored_edges)] if len(stored_edges) else centre
        return np.full(L, [near, centre, near + 1][g % 3], dtype=np.int64)
    if cls == "ties":
        lo, hi = int(w.min() - 3 * per_degree), int(w.max() + 3 * per_degree)
        a, b = (lo, hi) if g % 2 == 0 else (hi, lo)
        w[0], w[1], w[L - 2], w[L - 1] = a, b, b, a
        return w
    if cls == "on_edges":
        return np.array([stored_edges[((g + i) // 3) % len(stored_edges)] + ((g + i) % 3 - 1) for i in range(L)], dtype=np.int64)
    if cls == "fill_last":
        w[L - 1] = fill
        return w
    if cls == "fill_mid":
        w[1 + g % (L - 2)] = fill
        return w
    if cls == "one_valid":
        keep = w[g % L]
        w[:] = fill
        w[g % L] = keep
        return w
    if cls == "extremes":
        w[g % L], w[(g + 1) % L] = limits[0], limits[1]
        return w
    raise KeyError(cls)


def packed_class_cube(recipe, stored_near, fill, np_dtype=np.int16):
    """(stored [T, n_cells], class_of_cell) for a packed recipe; `stored_near(value)` is the recipe's unpack rule inverted (e.g.
    `packed_recipes.stored_near`)."""
    edges = [int(stored_near(e)) for e in list(recipe.edges) + list(recipe.sine_edges)]
    centre = int(stored_near(12.0))
    per_degree = float(stored_near(13.0) - centre)
    info = np.iinfo(np_dtype)
    q = np.empty((recipe.T, recipe.n_cells), dtype=np.int64)
    _fill_by_class(q, recipe.inner_bounds, len(PACKED_CLASSES),
                   lambda k, L, g: packed_window(PACKED_CLASSES[k], L, edges, g, fill, centre, per_degree, (info.min, info.max)))
    assert q.min() >= info.min and q.max() <= info.max
    return q.astype(np_dtype), np.array([PACKED_CLASSES[c % len(PACKED_CLASSES)] for c in range(recipe.n_cells)])


def hardware_zero_rule(out, cube, bounds, calc):
    """The kernels' inner min / max where the reference's is a zero: -0 < +0 (the hardware's min / max), whichever came first.
    `out` [G, ...] is the oracle's resample of `cube` [T, ...] by `calc`; returns it with the zeros' signs re-decided."""
    if calc not in ("min", "max"):
        return out
    out = out.copy()
    zero = (cube == 0)
    neg = zero & np.signbit(cube)
    pos = zero & ~np.signbit(cube)
    for g in range(len(bounds) - 1):
        lo, hi = int(bounds[g]), int(bounds[g + 1])
        if hi == lo:
            continue
        z = out[g] == 0
        if calc == "min":
            out[g] = np.where(z & neg[lo:hi].any(axis=0), -0.0, out[g])
        else:
            out[g] = np.where(z & pos[lo:hi].any(axis=0), 0.0, out[g])
    return out


def mismatches(got, want, *, bit_exact, rtol=0.0, atol=0.0):
    """Boolean array: where `got` is not the same kind of value as `want`, or misses the bar (see assert_same_kind)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.isnan(got) != np.isnan(want)
    bad |= np.isinf(got) != np.isinf(want)
    bad |= np.isinf(want) & np.isinf(got) & (np.signbit(got) != np.signbit(want))
    fin = np.isfinite(got) & np.isfinite(want)
    if bit_exact:
        bad |= fin & (want == 0) & (got == 0) & (np.signbit(got) != np.signbit(want))
    with np.errstate(invalid="ignore", over="ignore"):
        if rtol == 0 and atol == 0:
            bad |= fin & (got != want)
        else:
            bad |= fin & ~(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= atol + rtol * np.abs(want.astype(np.float64)))
    return bad


def assert_same_kind(got, want, *, bit_exact, rtol=0.0, atol=0.0, msg="", cell_class=None):
    """NaN positions equal; +-inf positions equal with sign; zeros equal with sign where `bit_exact`; finite values equal (rtol ==
    atol == 0) or within atol + rtol |want|.  `cell_class` (names along the last axis) puts the class of the first failing cell
    into the message."""
    bad = mismatches(got, want, bit_exact=bit_exact, rtol=rtol, atol=atol)
    if not bad.any():
        return
    got, want = np.asarray(got), np.asarray(want)
    at = tuple(int(i) for i in np.argwhere(bad)[0])
    where = f" (class {cell_class[at[-1]]})" if cell_class is not None else ""
    classes = ""
    if cell_class is not None:
        names, counts = np.unique(np.asarray(cell_class)[np.argwhere(bad)[:, -1]], return_counts=True)
        classes = "; failing cells by class: " + ", ".join(f"{n}={c}" for n, c in zip(names, counts))
    raise AssertionError(f"{msg}: {int(bad.sum())} of {bad.size} differ in kind or value; first at {at}{where}: got {got[at]!r}, want {want[at]!r}"
                         f"{classes}")
