"""The special-value windows keep their promises, and the oracle's two restatements agree on them.

`tests/special_values.py` builds what tests/test_gpu_special_values.py feeds every kernel; the oracle (`oracle.cport`, the C port of
`oracle.ref_temporal`'s numpy restatement of the reference's kernels) is the judge there.  So here, without a GPU: every class
holds what its name says for every window length, the two restatements agree in kind, in the sign of their zeros and in value on
class cubes, and both give a small table of answers that was worked out by reading `aggfly/aggregate/nb_kernels.py:121-251`.
"""
import numpy as np
import pytest

import special_values as sv
import variant_recipes as vr
from oracle import cport
from oracle import ref_temporal as rt

DTYPES = [np.float32, np.float64]
EDGES = [-6.0, 3.0, 10.0, 20.0, 30.0]
INF = float("inf")


# ---- 1. every class keeps its promise ----
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("cls", sv.CLASSES)
def test_every_class_keeps_its_promise(cls, dtype):
    for L in range(0, 15):
        seen_first = seen_last = seen_mid = False
        for g in range(0, 17):
            w = sv.window(cls, L, dtype, EDGES, g)
            assert w.dtype == dtype and w.shape == (L,)
            if L == 0:
                continue
            eff = sv.effective_class(cls, L, EDGES)
            assert eff == (cls if L >= sv.NEEDS.get(cls, 1) else "flat")
            w64 = w.astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                s = np.cumsum(w64)[-1]                       # the reference's order: first row to last
            if eff == "control":
                assert np.isfinite(w).all() and (L < 2 or (np.diff(w) != 0).all()) and (np.abs(w) < 40).all()
            elif eff == "flat":
                assert (w == w[0]).all() and (np.signbit(w) == np.signbit(w[0])).all() and np.isfinite(w[0])
            elif eff == "ties":
                assert (w == w.min()).sum() == 2 and (w == w.max()).sum() == 2 and w.min() < w.max()
                assert w[0] == w[-1] and w[1] == w[-2] and {w[0], w[1]} == {w.min(), w.max()}
            elif eff in ("zeros_pn", "zeros_np"):
                assert (w == 0).all() and np.signbit(w[0]) == (eff == "zeros_np") and (L < 2 or (np.diff(np.signbit(w).astype(int)) != 0).all())
            elif eff == "on_edges":
                assert all(x in [dtype(e) for e in EDGES] for x in w)
            elif eff in ("pinf", "ninf"):
                assert np.isinf(w).sum() == 1 and not np.isnan(w).any() and s == (INF if eff == "pinf" else -INF)
                assert np.isfinite(np.delete(w, np.flatnonzero(np.isinf(w)))).all()
            elif eff == "both_inf":
                assert (w == INF).sum() == 1 and (w == -INF).sum() == 1 and not np.isnan(w).any() and np.isnan(s)
            elif eff == "subnormal":
                tiny = np.nextafter(dtype(0), dtype(1))
                assert tiny > 0 and tiny < np.finfo(dtype).tiny and ((w == 0) | (np.abs(w) == tiny)).all()
                assert (w == tiny).sum() + (w == -tiny).sum() == min(L, 2) and (L < 2 or ((w == tiny).any() and (w == -tiny).any()))
            elif eff == "overflow":
                assert np.isfinite(w).all()
                if dtype is np.float64:
                    assert np.isinf(s) and s > 0
                else:
                    assert np.isfinite(s) and np.isinf(np.float32(s)) and np.abs(w).max() == np.finfo(np.float32).max
            elif eff == "nan_last":
                assert np.isnan(w[-1]) and np.isnan(w).sum() == 1
            elif eff == "nan_mid":
                at = np.flatnonzero(np.isnan(w))
                assert len(at) == 1 and 0 < at[0] < L - 1
            elif eff == "one_valid":
                assert np.isfinite(w).sum() == 1 and np.isnan(w).sum() == L - 1
            special = np.flatnonzero(~np.isfinite(w) | (np.abs(w) > 1e30) | ((w != 0) & (np.abs(w) < 1e-30)))
            if cls == "one_valid":
                special = np.flatnonzero(np.isfinite(w))
            seen_first |= 0 in special
            seen_last |= (L - 1) in special
            seen_mid |= any(0 < p < L - 1 for p in special)
        if L >= 3 and cls in ("pinf", "ninf", "both_inf", "subnormal", "overflow", "one_valid"):
            assert seen_first and seen_mid and seen_last, (cls, L)       # g moves the special rows through the window
    if cls == "overflow" and dtype is np.float32:
        assert {float(np.sign(sv.window(cls, 4, dtype, EDGES, g).astype(np.float64).sum())) for g in range(4)} == {1.0, -1.0}
    if cls == "flat":
        firsts = [sv.window(cls, 3, dtype, EDGES, g)[0] for g in range(40)]
        assert {dtype(e) for e in EDGES} <= set(firsts) and dtype(12.25) in firsts
        assert any(x == 0 and np.signbit(x) for x in firsts) and any(x == 0 and not np.signbit(x) for x in firsts)


def _recipe(dtype, lens, n_cells=len(sv.CLASSES) * sv.ROTATIONS + 5):
    ib = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return vr.Recipe("", vr.F64 if dtype is np.float64 else vr.F32, int(ib[-1]), n_cells, ib, np.array([0, len(lens)]), [], True, 0,
                     edges=[-6.0, 3.0, 20.0], sine_edges=[10.0, 30.0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_class_cube_puts_every_class_in_every_group(dtype):
    r = _recipe(dtype, [4, 0, 9, 1, 3])
    cube, cls = sv.class_cube(r)
    assert cube.shape == (r.T, r.n_cells) and cube.dtype == dtype and list(cls[:len(sv.CLASSES)]) == list(sv.CLASSES)
    assert (cls == np.array([sv.CLASSES[c % len(sv.CLASSES)] for c in range(r.n_cells)])).all()
    edges = r.edges + r.sine_edges
    for c in range(r.n_cells):
        for g, (lo, hi) in enumerate(zip(r.inner_bounds[:-1], r.inner_bounds[1:])):
            want = sv.window(cls[c], hi - lo, dtype, edges, g + 2 * ((c // len(sv.CLASSES)) % sv.ROTATIONS))
            assert np.array_equal(cube[lo:hi, c].view(np.uint32 if dtype is np.float32 else np.uint64), want.view(np.uint32 if dtype is np.float32 else np.uint64))


def test_packed_class_cube_holds_what_the_storage_can():
    import packed_recipes as pr
    r = _recipe(np.float32, [4, 0, 9, 1, 3], n_cells=len(sv.PACKED_CLASSES) * sv.ROTATIONS + 3)
    r.edges, r.sine_edges = [pr._snap(e) for e in r.edges], [pr._snap(e) for e in r.sine_edges]
    q, cls = sv.packed_class_cube(r, pr.stored_near, pr.FILL)
    assert q.dtype == np.int16 and q.shape == (r.T, r.n_cells)
    v = pr.np_unpack(q)
    by = {name: v[:, cls == name] for name in sv.PACKED_CLASSES}
    assert not np.isnan(by["control"]).any() and not np.isnan(by["ties"]).any() and not np.isnan(by["extremes"]).any()
    g9 = slice(4, 13)                                                    # the nine-row group
    assert (by["flat"][g9] == by["flat"][4]).all()
    assert ((by["ties"][g9] == by["ties"][g9].min(axis=0)).sum(axis=0) == 2).all() and ((by["ties"][g9] == by["ties"][g9].max(axis=0)).sum(axis=0) == 2).all()
    assert all((by["on_edges"] == np.float32(e)).any() for e in r.edges + r.sine_edges)              # the edge itself, and both neighbours
    on = q[:, cls == "on_edges"]
    assert all({pr.stored_near(e) - 1, pr.stored_near(e) + 1} <= set(on.reshape(-1).tolist()) for e in r.edges)
    assert np.isnan(by["fill_last"][12]).all() and np.isnan(by["fill_last"][g9]).sum(axis=0).max() == 1
    assert (np.isnan(by["fill_mid"][g9]).sum(axis=0) == 1).all() and not np.isnan(by["fill_mid"][[4, 12]]).any()
    assert (np.isfinite(by["one_valid"][g9]).sum(axis=0) == 1).all()
    assert {-32768, 32767} <= set(q[:, cls == "extremes"].reshape(-1).tolist())
    assert not np.isinf(v).any() and not ((v == 0) & np.signbit(v)).any()


# ---- 2. the oracle's two restatements agree where the GPU tests look ----
CALCS = [("mean", None), ("sum", None), ("min", None), ("max", None), ("nanmean", None),
         ("dd", (-6.0, 3.0, 0.0)), ("dd", (3.0, 20.0, 1.0)), ("dd", (0.0, INF, 0.0)), ("dd", (-INF, 20.0, 1.0)),
         ("bins", (-6.0, 3.0, 0.0)), ("bins", (0.0, INF, 0.0)), ("bins", (-INF, 20.0, 0.0)),
         ("sine_dd", (10.0, 30.0, 0.0)), ("sine_dd", (10.0, 30.0, 1.0))]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("L", [1, 2, 3, 4, 9])
def test_the_two_restatements_agree_on_class_cubes(L, dtype):
    r = _recipe(dtype, [L] * 9)
    cube, cls = sv.class_cube(r)
    cube = cube.reshape(r.T, 1, r.n_cells)
    for calc, args in CALCS:
        with np.errstate(over="ignore", invalid="ignore"):       # the overflow class overflows, as it says
            a = rt.numba_resample(cube, r.inner_bounds, calc, args)
        b = cport.resample(cube, r.inner_bounds, calc, args)
        assert a.dtype == b.dtype == dtype
        # sine_dd: numpy's and libm's acos / atan / sin / cos may differ in the last place; everything else is the same IEEE operations
        bar = dict(rtol=1e-13, atol=1e-13) if calc == "sine_dd" else {}
        sv.assert_same_kind(b.reshape(9, -1), a.reshape(9, -1), bit_exact=calc != "sine_dd", msg=f"{calc} {args} L={L}", cell_class=cls, **bar)


# ---- 3. answers worked out from nb_kernels.py:121-251, not from running anything ----
def _both(window, calc, args=None, dtype=np.float64):
    cube = np.array(window, dtype=dtype).reshape(-1, 1, 1)
    b = np.array([0, len(window)], dtype=np.int64)
    x, y = rt.numba_resample(cube, b, calc, args)[0, 0, 0], cport.resample(cube, b, calc, args)[0, 0, 0]
    return x, y


def _is(value, want):
    if np.isnan(want):
        return np.isnan(value)
    return value == want and np.signbit(value) == np.signbit(want)


TINY64 = float(np.nextafter(0.0, 1.0))
ANSWERS = [
    # min / max start from +-inf and move on a STRICT compare (nb_kernels.py:136-139): of equal values the first seen stays
    ([0.0, -0.0], "min", None, 0.0), ([-0.0, 0.0], "min", None, -0.0), ([0.0, -0.0], "max", None, 0.0), ([-0.0, 0.0], "max", None, -0.0),
    ([0.0, -0.0, 0.0], "sum", None, 0.0), ([-0.0, -0.0], "sum", None, 0.0),              # s starts at +0.0: +0 + -0 = +0
    ([-0.0], "mean", None, 0.0),
    # both infinities: s = inf + -inf = NaN without a NaN row, so hasnan is false and the statistics are returned as they are
    ([1.0, INF, -INF], "mean", None, np.nan), ([1.0, INF, -INF], "sum", None, np.nan), ([1.0, INF, -INF], "nanmean", None, np.nan),
    ([1.0, INF, -INF], "min", None, -INF), ([1.0, INF, -INF], "max", None, INF),
    ([2.0, INF], "mean", None, INF), ([2.0, -INF], "min", None, -INF),
    # a NaN row: every statistic but nanmean is NaN, nanmean divides by the valid rows
    ([1.0, np.nan, 3.0], "min", None, np.nan), ([1.0, np.nan, 3.0], "nanmean", None, 2.0), ([np.nan], "nanmean", None, np.nan),
    # bins: strict compares in float64 (nb_kernels.py:190-196): a subnormal is above 0, a zero of either sign is not, inf is below no t1
    ([TINY64, 0.0, -0.0, -TINY64], "bins", (0.0, 1.0, 0.0), 1.0), ([TINY64, -TINY64], "bins", (-1.0, 0.0, 0.0), 1.0),
    ([5.0, INF], "bins", (0.0, INF, 0.0), 1.0), ([5.0, -INF, np.nan], "bins", (-INF, 10.0, 0.0), 1.0),
    # dd: |v - base| where t0 < v < t1 strictly (nb_kernels.py:166-176); inf is not below t1 = inf
    ([5.0, INF], "dd", (0.0, INF, 0.0), 5.0), ([5.0, -INF], "dd", (-INF, 10.0, 1.0), 5.0), ([5.0, INF], "dd", (0.0, 10.0, 1.0), 5.0),
    ([0.0, -0.0, TINY64], "dd", (0.0, 1.0, 0.0), TINY64), ([5.0, np.nan], "dd", (0.0, 10.0, 0.0), np.nan),
    # sine_dd, cooling (kind 0): part(thr) = tavg - thr where thr <= tmin, 0 where thr >= tmax; the column is part(t0) - part(t1).
    # A flat window has tmin == tmax: no threshold is strictly inside, and the arc is never taken
    ([12.0, 12.0, 12.0], "sine_dd", (10.0, 30.0, 0.0), 2.0),        # above t0: tavg - t0
    ([10.0, 10.0], "sine_dd", (10.0, 30.0, 0.0), 0.0),               # at t0: thr <= tmin holds, tavg - thr = 0
    ([7.0, 7.0], "sine_dd", (10.0, 30.0, 0.0), 0.0),                 # below both
    ([30.0, 30.0], "sine_dd", (10.0, 30.0, 0.0), 20.0),              # at t1: (30 - 10) - (30 - 30)
    ([35.0], "sine_dd", (10.0, 30.0, 0.0), 20.0),                    # above both: (35 - 10) - (35 - 30), one row
    # heating (kind 1): part(thr) = thr - tavg where thr >= tmax; the column is part(t1) - part(t0)
    ([12.0, 12.0], "sine_dd", (10.0, 30.0, 1.0), 18.0), ([7.0, 7.0], "sine_dd", (10.0, 30.0, 1.0), 20.0),
    ([10.0, 10.0], "sine_dd", (10.0, 30.0, 1.0), 20.0), ([35.0, 35.0], "sine_dd", (10.0, 30.0, 1.0), 0.0),
    ([0.0, -0.0], "sine_dd", (0.0, 5.0, 0.0), 0.0),                  # tmin = tmax = 0 = t0: tavg - t0 = 0
]


@pytest.mark.parametrize("case", range(len(ANSWERS)))
def test_both_restatements_give_the_answers_read_off_the_reference(case):
    window, calc, args, want = ANSWERS[case]
    x, y = _both(window, calc, args)
    assert _is(x, want) and _is(y, want), (window, calc, args, want, x, y)


def test_float32_store_of_an_overflowing_sum():
    """+-finfo(float32).max twice: the float64 accumulator holds 2 max, the float32 result is infinite (nb_kernels.py:257-268)."""
    big = float(np.finfo(np.float32).max)
    for sign in (1.0, -1.0):
        x, y = _both([sign * big, sign * big], "sum", dtype=np.float32)
        assert x == y == sign * INF
        x, y = _both([sign * big, sign * big], "mean", dtype=np.float32)
        assert x == y == np.float32(sign * big)


# ---- 4. the compare itself ----
def test_assert_same_kind_sees_what_array_equal_does_not():
    a = np.array([0.0, 1.0, np.nan, INF, -INF, 5e-324])
    sv.assert_same_kind(a, a.copy(), bit_exact=True)
    np.testing.assert_array_equal(np.array([-0.0]), np.array([0.0]))                     # the gap
    with pytest.raises(AssertionError, match="class zeros_pn"):
        sv.assert_same_kind(np.array([-0.0]), np.array([0.0]), bit_exact=True, cell_class=np.array(["zeros_pn"]))
    sv.assert_same_kind(np.array([-0.0]), np.array([0.0]), bit_exact=False, rtol=1e-10)
    for got, want in [([INF], [-INF]), ([INF], [1e308]), ([np.nan], [INF]), ([1.0], [np.nan]), ([1.0 + 1e-9], [1.0])]:
        with pytest.raises(AssertionError):
            sv.assert_same_kind(np.array(got), np.array(want), bit_exact=False, rtol=1e-10)
    sv.assert_same_kind(np.array([1.0 + 1e-12, INF]), np.array([1.0, INF]), bit_exact=False, rtol=1e-10)
    with pytest.raises(AssertionError):
        sv.assert_same_kind(np.array([1.0 + 1e-12]), np.array([1.0]), bit_exact=True)


def test_hardware_zero_rule_only_touches_zeros_of_both_signs():
    cube = np.array([[0.0, -0.0, 0.0, 1.0, -0.0], [-0.0, 0.0, 0.0, -0.0, -0.0]]).reshape(2, 1, 5)
    b = np.array([0, 2])
    mn, mx = cport.resample(cube, b, "min"), cport.resample(cube, b, "max")
    assert list(np.signbit(mn[0, 0])) == [False, True, False, True, True] and list(np.signbit(mx[0, 0])) == [False, True, False, False, True]
    hmn, hmx = sv.hardware_zero_rule(mn, cube, b, "min"), sv.hardware_zero_rule(mx, cube, b, "max")
    assert list(np.signbit(hmn[0, 0])) == [True, True, False, True, True] and list(np.signbit(hmx[0, 0])) == [False, False, False, False, True]
    assert np.array_equal(hmn, mn) and np.array_equal(hmx, mx)                           # by value nothing moved
