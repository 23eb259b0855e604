"""Packed cubes with one unpack rule per range of time steps (`PackedCube.concat`, `afhip_plan_bind_packings`) on the GPU: the unpack
over every stored value, the temporal kernel with rule changes wherever they can fall, chunks that start inside the rule list, the
public route over several Zarr stores of different packings, and what the library refuses.

The yardstick of a multi-rule plan is the float32 plan of the same columns on `materialize()`'s values — which the first test holds,
bit for bit, to numpy's float32 chain per range of rows.  Under `exact_order` the two must agree in every bit, otherwise to 1e-12 (the
project's figure for its fast routes); both are held to the oracle at the project's 1e-10.
"""
import functools
import json
import os
import re

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import synth
from oracle import ref_aggregate as ra

from test_gpu_variant_menu import _oracle_two_level

pytestmark = pytest.mark.gpu


def _same_bits(got, want):
    """float32 arrays equal bit for bit, NaN payloads included (the unpack writes one quiet NaN, numpy's np.nan in float32)."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _np_unpack(bits, pairs, fill, unsigned):
    """The unpack rule in numpy float32, one rounded operation at a time; `bits`: int16 holding the stored 16 bits."""
    w = bits.view(np.uint16).astype(np.int32) if unsigned else bits.astype(np.int32)
    f = w.astype(np.float32)
    for m, a in pairs:
        if m is not None:
            f = f * np.float32(m)
        if a is not None:
            f = f + np.float32(a)
    if fill is not None:
        f = np.where(w == fill, np.float32(np.nan), f)
    return f


def _np_values(bits, rules, bounds, unsigned):
    return np.concatenate([_np_unpack(bits[lo:hi], p, f, unsigned) for (p, f), lo, hi in zip(rules, bounds[:-1], bounds[1:])])


def _f32_rules(rules):
    return [([tuple(None if x is None else np.float32(x) for x in pr) for pr in p], f) for p, f in rules]


def _cube(torch, bits, rules, bounds, unsigned):
    """The multi-rule PackedCube of int16 `bits` [T, ...] in HBM."""
    d = torch.from_numpy(bits).cuda()
    parts = [af.PackedCube(d[lo:hi], fill_value=f, unsigned=unsigned, _pairs=p) for (p, f), lo, hi in zip(_f32_rules(rules), bounds[:-1], bounds[1:])]
    return af.PackedCube.concat(parts)


# Five rule shapes per storage — zero to three pairs, with and without a fill, different scales — whose values are temperatures in C
# (the bare integers of the pair-less rule apart)
def _rule_shapes(unsigned):
    if unsigned:
        return [([(0.0017, 225.6), (None, -273.15)], 65535), ([(0.002, 215.0), (None, -273.15)], 0), ([(0.0015, None), (None, -41.0)], None),
                ([(0.0017, 225.6), (None, -273.15), (1.0, 0.5)], 40000), ([], None)]
    return [([(0.0017, 281.3), (None, -273.15)], -32767), ([(0.002, 285.0), (None, -273.15)], -32768), ([(0.0015, None), (None, 8.0)], None),
            ([(0.0017, 281.3), (None, -273.15), (1.0, 0.5)], 1234), ([], None)]


# ---- 1. the unpack, over every stored value under every rule ----
@pytest.mark.parametrize("unsigned", [False, True], ids=["int16", "uint16"])
def test_unpack_every_stored_value_rule_by_rule(torch_cuda, unsigned):
    rng = np.random.default_rng(3)
    bits = np.stack([rng.permutation(65536).astype(np.uint16).view(np.int16) for _ in range(7)])       # (7, 65536): every value in each row
    bounds = [0, 1, 2, 5, 7]
    if unsigned:
        rules = [([], None), ([(0.0017, 225.6)], 65535), ([(0.002, None), (None, -41.0)], 40000), ([(0.0017, 225.6), (None, -273.15), (1.8, 32.0)], 65535)]
    else:
        rules = [([], None), ([(0.0017, 281.3)], -32767), ([(0.002, None), (None, 8.0)], 1234), ([(0.0017, 281.3), (None, -273.15), (1.8, 32.0)], -32767)]
    cube = _cube(torch_cuda, bits, rules, bounds, unsigned)
    assert cube.n_rules == 4 and cube.rule_bounds == bounds and cube.rules == _f32_rules(rules) and cube.nbytes() == bits.nbytes
    want = _np_values(bits, rules, bounds, unsigned)
    assert [int(np.isnan(want[lo:hi]).sum()) for lo, hi in zip(bounds[:-1], bounds[1:])] == [0, 1, 3, 2]
    _same_bits(cube.materialize().cpu().numpy(), want)
    # ranges of rows that start off the unpack kernel's alignment, and a cube whose time axis is not the first
    _same_bits(cube[:, 3:].materialize().cpu().numpy(), want[:, 3:])
    _same_bits(cube[1:6, 1:-2].materialize().cpu().numpy(), want[1:6, 1:-2])
    _same_bits(cube.permute(1, 0).materialize().cpu().numpy(), want.T)
    from aggfly_amd import hip
    _same_bits(hip.unpack_i16(cube[4:]).cpu().numpy(), want[4:])


# ---- 2. the kernel: rule boundaries wherever they can fall ----
T2 = 24 * 40
CHANGES = [1, 2, 3, 5, 24, 24 * 2 + 7, 24 * 3 + 8, 24 * 3 + 9, 24 * 3 + 10, 240, 24 * 20 + 23, T2 - 1]
BOUNDS2 = [0] + CHANGES + [T2]
IB2 = np.arange(0, T2 + 1, 24, dtype=np.int64)
OB2 = {"month": np.array([0, 31, 40], dtype=np.int64), "year": np.array([0, 40], dtype=np.int64)}
# a light plan (it takes four / two / one cells per lane by the row length) and the other inner statistics
LIGHT = [dict(inner="mean", transform="pow", transform_arg=2.0, outer="sum"), dict(inner="dd", inner_args=(10.0, 30.0, 0.0), outer="sum")]
HEAVY = [dict(inner="bins", inner_args=(0.0, 10.0, 0.0), outer="sum"), dict(inner="min", outer="min"), dict(inner="max", outer="mean"),
         dict(inner="nanmean", outer="sum"), dict(inner="sine_dd", inner_args=(10.0, 30.0, 0.0), outer="sum")]


def _rules_along(bounds, unsigned):
    shapes = _rule_shapes(unsigned)
    return [shapes[i % len(shapes)] for i in range(len(bounds) - 1)]


def _stored(T, n_cells, bounds, rules, seed):
    """int16 bits [T, n_cells]: the whole range, every fill value of the rule list scattered over ALL rows (a fill is missing under
    its own rule only), two cells — the last one included — that are missing wherever their rule has a fill, and whole days of fills
    for three cells."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 65536, (T, n_cells)).astype(np.uint16)
    for f in {f for _, f in rules if f is not None}:
        bits[rng.random((T, n_cells)) < 0.01] = np.uint16(f & 0xffff)
    for (_, f), lo, hi in zip(rules, bounds[:-1], bounds[1:]):
        if f is not None:
            bits[lo:hi, 5] = np.uint16(f & 0xffff)
            bits[lo:hi, n_cells - 1] = np.uint16(f & 0xffff)
            for day in range((lo + 23) // 24, hi // 24)[:2]:
                bits[24 * day:24 * day + 24, 7:10] = np.uint16(f & 0xffff)
    return bits.view(np.int16)


@functools.lru_cache(maxsize=None)
def _case2(unsigned, n_cells):
    import torch
    rules = _rules_along(BOUNDS2, unsigned)
    bits = _stored(T2, n_cells, BOUNDS2, rules, seed=n_cells + unsigned)
    cube = _cube(torch, bits.reshape(T2, 1, n_cells), rules, BOUNDS2, unsigned)
    values = cube.materialize()
    return cube, values, values.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _oracle2(unsigned, n_cells, outer, which):
    return _oracle_two_level(_case2(unsigned, n_cells)[2], IB2, OB2[outer], LIGHT if which == "light" else HEAVY)


def _hold(got_p, got_f, want, cols, exact):
    assert got_p.shape == got_f.shape == want.shape
    for k, col in enumerate(cols):
        msg = f"column {k}: {col}"
        if exact:
            np.testing.assert_array_equal(got_p[k], got_f[k], err_msg=msg)
        else:
            np.testing.assert_allclose(got_p[k], got_f[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=msg)
        atol = 1e-10 if col["inner"] == "sine_dd" else 0           # sine_dd's contract (test_gpu_variant_menu.py: _assert_cells)
        np.testing.assert_allclose(got_p[k], want[k], rtol=1e-10, atol=atol, equal_nan=True, err_msg=msg)
        np.testing.assert_allclose(got_f[k], want[k], rtol=1e-10, atol=atol, equal_nan=True, err_msg=msg)


@pytest.mark.parametrize("exact", [True, False], ids=["exact_order", "fast"])
@pytest.mark.parametrize("outer", ["month", "year"])
@pytest.mark.parametrize("unsigned", [False, True], ids=["int16", "uint16"])
@pytest.mark.parametrize("n_cells,vec", [(1100, 4), (1102, 2), (1101, 1)])
def test_rule_changes_wherever_they_can_fall(torch_cuda, n_cells, vec, unsigned, outer, exact):
    from aggfly_amd import hip
    cube, values, _ = _case2(unsigned, n_cells)
    assert cube.n_rules == len(BOUNDS2) - 1 and cube.rule_bounds == BOUNDS2
    for which, cols in (("light", LIGHT), ("heavy", HEAVY)):
        plan = hip.FusedPlan(T2, n_cells, hip.U16 if unsigned else hip.I16, IB2, OB2[outer], cols, exact_order=exact)
        plan.bind_packing(cube)
        if which == "light":
            assert f"variant=i16_p0_v{vec}_" in plan.describe(), plan.describe()
        got_p = plan.run_temporal(cube).cpu().numpy()
        f32 = hip.FusedPlan(T2, n_cells, hip.F32, IB2, OB2[outer], cols, exact_order=exact)
        got_f = f32.run_temporal(values).cpu().numpy()
        _hold(got_p, got_f, _oracle2(unsigned, n_cells, outer, which), cols, exact)


# ---- 3. chunks that start inside the rule list ----
def test_chunks_start_inside_the_rule_list(torch_cuda):
    """One output period cut into time chunks of whole days; forty rules of 100 steps, so the chunks start inside rules and each
    workgroup has to find its own first rule.  Only the fast route cuts a period (`exact_order` keeps it whole), and it spends at most
    5 % of the cube's bytes on the partials of the cuts (afhip_planner.cpp: lay_chunks): T = 4000 two-byte steps buy the
    five-column plan five cuts."""
    from aggfly_amd import hip
    exact = False
    T, n_cells = 4000, 1102
    bounds = list(range(0, T + 1, 100))
    ib = np.array(list(range(0, T, 24)) + [T], dtype=np.int64)
    ob = np.array([0, len(ib) - 1], dtype=np.int64)
    rules = _rules_along(bounds, False)
    bits = _stored(T, n_cells, bounds, rules, seed=17)
    cube = _cube(torch_cuda, bits.reshape(T, 1, n_cells), rules, bounds, False)
    assert cube.n_rules == 40
    values = cube.materialize()
    want64 = values.cpu().numpy().astype(np.float64)
    for cols in (LIGHT, HEAVY):
        plan = hip.FusedPlan(T, n_cells, hip.I16, ib, ob, cols, exact_order=exact)
        plan.bind_packing(cube)
        got_p = plan.run_temporal(cube).cpu().numpy()
        n_chunks = int(re.search(r"chunks=(\d+)", plan.describe()).group(1))
        assert n_chunks >= 3, plan.describe()
        starts = [int(ib[np.searchsorted(ib, T * i // n_chunks)]) for i in range(1, n_chunks)]       # (where lay_chunks cuts)
        assert any(k % 100 for k in starts), starts
        got_f = hip.FusedPlan(T, n_cells, hip.F32, ib, ob, cols, exact_order=exact).run_temporal(values).cpu().numpy()
        _hold(got_p, got_f, _oracle_two_level(want64, ib, ob, cols), cols, exact)


# ---- 4.-6. the public route over several stores ----
LZ4 = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
NY, NX = 8, 12
LENS = [24 * 10, 24 * 7 + 5, 24 * 13]            # the second boundary falls inside a day
ATTRS = [{"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767},
         {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32768},
         {"add_offset": 290.0}]                 # no scale_factor (whole kelvins), no fill


def _write_store(path, var, stored, time, attrs):
    from aggfly_amd import io as afio
    tv, tattrs = afio._encode_time(time)
    os.makedirs(path)
    json.dump({"zarr_format": 2}, open(os.path.join(path, ".zgroup"), "w"))
    afio._write_array(path, var, stored, ("time", "latitude", "longitude"), (48, NY, NX), attrs, LZ4)
    afio._write_array(path, "time", np.asarray(tv, dtype=np.float64), ("time",), (len(time),), tattrs, None)
    afio._write_array(path, "latitude", 35 + 0.25 * np.arange(NY), ("latitude",), (NY,), {}, None)
    afio._write_array(path, "longitude", 250 + 0.25 * np.arange(NX), ("longitude",), (NX,), {}, None)


def _three_stores(tmp_path, attrs=ATTRS, dtypes=(np.int16,) * 3):
    rng = np.random.default_rng(8)
    time = pd.date_range("2004-03-01", periods=sum(LENS), freq="h")
    paths, k = [], 0
    for i, (n, at, dt) in enumerate(zip(LENS, attrs, dtypes)):
        if "scale_factor" in at:
            stored = rng.integers(-30000, 30000, (n, NY, NX)) if dt == np.int16 else rng.integers(2000, 62000, (n, NY, NX))
        else:
            stored = rng.integers(-40, 40, (n, NY, NX)) if dt == np.int16 else rng.integers(0, 80, (n, NY, NX))
        stored = stored.astype(dt)
        for fv in (-32767, -32768):                                  # both fill values in every store: each is missing in its own only
            stored[rng.random(stored.shape) < 0.02] = np.array(fv).astype(dt) if dt == np.int16 else dt(fv & 0xffff)
        if "_FillValue" in at:
            stored[:, 2, 3] = dt(at["_FillValue"])                   # an ocean cell (where the store has a fill)
        paths.append(str(tmp_path / f"part{i}.zarr"))
        _write_store(paths[-1], "t2m", stored, time[k:k + n], at)
        k += n
    return paths


def _celsius(x):
    return x - 273.15


def _spec(outer):
    return dict(
        dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": outer})],
        tavg=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 4)}),
              ("aggregate", {"calc": "sum", "groupby": outer})],
        bins=[("aggregate", {"calc": "bins", "groupby": "date", "ddargs": [[0, 10, 0], [10, 20, 0]]}), ("aggregate", {"calc": "sum", "groupby": outer})],
    )


def _open3(paths, **kw):
    host = af.dataset_from_path(paths, "t2m", preprocess=_celsius, **kw)
    plain = af.dataset_from_path(paths, "t2m", device="cuda", preprocess=_celsius, **kw)
    packed = af.dataset_from_path(paths, "t2m", device="cuda", keep_packed=True, preprocess=_celsius, **kw)
    return host, plain, packed


def test_three_stores_of_different_packings_stay_packed(torch_cuda, tmp_path):
    from aggfly_amd import engine as eng
    paths = _three_stores(tmp_path)
    host, plain, packed = _open3(paths)
    T = sum(LENS)
    assert packed.is_packed and not plain.is_packed and not host.is_packed
    data = packed.da.data
    assert data.n_rules == 3 and data.rule_bounds == [0, LENS[0], LENS[0] + LENS[1], T]
    k = np.float32(-273.15)
    assert data.rules == [([(np.float32(0.0017), np.float32(281.3)), (None, k)], -32767), ([(np.float32(0.0017), np.float32(281.3)), (None, k)], -32768),
                          ([(None, np.float32(290.0)), (None, k)], None)]
    q = packed.packed_cube().q
    assert q.dtype == torch_cuda.int16 and q.is_cuda and q.numel() * q.element_size() == T * NY * NX * 2      # 2 bytes per cell-step in HBM
    assert packed.packed_cube().rule_bounds == data.rule_bounds and packed.da.dtype == torch_cuda.float32
    cube = packed.cube()
    assert cube.dtype == torch_cuda.float32 and cube.is_cuda
    _same_bits(cube.cpu().numpy(), plain.cube().cpu().numpy())
    np.testing.assert_array_equal(plain.cube().cpu().numpy(), host.cube())
    assert np.isnan(host.cube()).any()
    tab = synth.weights_table(NY, NX, 5, seed=3, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}), regionid="geoid")
    ods = ra.ODataset(host.cube().astype(np.float64), host.time, host.latitude, host.longitude, True)
    ow = ra.OWeights(tab, np.arange(NY * NX), gr.shp["geoid"], "geoid", "nan")
    old = eng.config.exact_order
    try:
        for outer in ("month", "year"):
            spec = _spec(outer)
            want = ra.aggregate_dataset(ow, ods, engine="numba", **spec)
            cols = [c for c in want.columns if c not in ("geoid", "time")]
            for exact in (True, False):
                eng.config.exact_order = exact
                got_p = af.aggregate_dataset(dataset=packed, weights=af.weights_from_objects(packed, gr, table=tab), **spec)
                got_f = af.aggregate_dataset(dataset=plain, weights=af.weights_from_objects(plain, gr, table=tab), **spec)
                assert list(got_p.columns) == list(want.columns) and len(got_p) == len(want)
                if exact:
                    np.testing.assert_array_equal(got_p[cols].values, got_f[cols].values)
                else:
                    np.testing.assert_allclose(got_p[cols].values, got_f[cols].values, rtol=1e-12, atol=0, equal_nan=True)
                np.testing.assert_allclose(got_p[cols].values, want[cols].values, rtol=1e-10, atol=0, equal_nan=True)
                np.testing.assert_allclose(got_f[cols].values, want[cols].values, rtol=1e-10, atol=0, equal_nan=True)
                tp, tf = af.aggregate_time(packed, **spec), af.aggregate_time(plain, **spec)
                assert list(tp) == list(tf)
                for name in tp:
                    a, b = tp[name].cube().cpu().numpy(), tf[name].cube().cpu().numpy()
                    if exact:
                        np.testing.assert_array_equal(a, b)
                    else:
                        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)
    finally:
        eng.config.exact_order = old


def test_a_time_selection_across_the_first_boundary_rebases_the_rules(torch_cuda, tmp_path):
    paths = _three_stores(tmp_path)
    sel = slice("2004-03-08", "2004-03-14")                      # the first store ends with March 10th
    host, plain, packed = _open3(paths, time_sel=sel)
    n = 24 * 7
    assert packed.is_packed and packed.da.data.n_rules == 2 and packed.da.data.rule_bounds == [0, 24 * 3, n]
    assert [f for _, f in packed.da.data.rules] == [-32767, -32768] and len(packed.time) == n
    _same_bits(packed.cube().cpu().numpy(), plain.cube().cpu().numpy())
    np.testing.assert_array_equal(plain.cube().cpu().numpy(), host.cube())
    tab = synth.weights_table(NY, NX, 5, seed=3, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}), regionid="geoid")
    spec = _spec("month")
    got_p = af.aggregate_dataset(dataset=packed, weights=af.weights_from_objects(packed, gr, table=tab), **spec)
    got_f = af.aggregate_dataset(dataset=plain, weights=af.weights_from_objects(plain, gr, table=tab), **spec)
    cols = [c for c in got_f.columns if c not in ("geoid", "time")]
    assert list(got_p.columns) == list(got_f.columns) and len(got_p) == len(got_f)
    np.testing.assert_allclose(got_p[cols].values, got_f[cols].values, rtol=1e-12, atol=0, equal_nan=True)
    assert np.isfinite(got_f[cols].values).any()


def test_stores_of_one_packing_and_of_mixed_signedness(torch_cuda, tmp_path):
    one = _three_stores(tmp_path / "one", attrs=[ATTRS[0]] * 3)
    host, plain, packed = _open3(one)
    assert packed.is_packed and packed.da.data.n_rules == 1 and packed.da.data.n_pairs == 2 and packed.da.data.fill_value == -32767
    _same_bits(packed.cube().cpu().numpy(), plain.cube().cpu().numpy())
    np.testing.assert_array_equal(plain.cube().cpu().numpy(), host.cube())
    # an int16 store beside a uint16 store: one plan reads one storage, so all take the float32 route
    u16 = {"scale_factor": 0.0017, "add_offset": 225.6, "_FillValue": 65535}
    mixed = _three_stores(tmp_path / "mixed", attrs=[ATTRS[0], u16, ATTRS[2]], dtypes=(np.int16, np.uint16, np.int16))
    host, plain, packed = _open3(mixed)
    assert not packed.is_packed and not plain.is_packed
    np.testing.assert_array_equal(packed.cube().cpu().numpy(), host.cube())
    np.testing.assert_array_equal(plain.cube().cpu().numpy(), host.cube())


# ---- 7. refusals ----
def test_binds_the_library_refuses(torch_cuda):
    import ctypes as C
    from aggfly_amd import hip
    T, n_cells = 60, 300
    ib, ob = np.array([0, 8, 20, 60]), np.array([0, 3])
    cols = [dict(inner="mean", outer="sum"), dict(inner="max", outer="max")]
    rng = np.random.default_rng(2)
    bits = rng.integers(-32768, 32768, (T, 1, n_cells)).astype(np.int16)
    lib = hip.load()
    good = af.PackedCube(np.zeros((1,), np.int16), 0.0017, 281.3, -32767).packing()
    other = af.PackedCube(np.zeros((1,), np.int16), 0.002, 270.0, -32768).packing()

    def bind(plan, rules, bounds):
        arr = (hip.Packing * max(len(rules), 1))(*rules)
        b = np.asarray(bounds, dtype=np.int64)
        return lib.afhip_plan_bind_packings(plan._h, arr, b.ctypes.data_as(C.POINTER(C.c_int64)), len(rules))

    for code, lo, hi in ((hip.I16, -32768, 32767), (hip.U16, 0, 65535)):
        plan = hip.FusedPlan(T, n_cells, code, ib, ob, cols)
        cube = _cube(torch_cuda, bits, [([(0.0017, 281.3)], 5), ([(0.002, 270.0)], None)], [0, 13, T], code == hip.U16)
        with pytest.raises(ValueError, match="bind_packing"):                  # never bound: the run is refused
            plan.run_temporal(cube)
        plan.bind_packing(cube)
        first = plan.run_temporal(cube).cpu().numpy()
        bad_fill = af.PackedCube(np.zeros((1,), np.int16), 0.0017, 281.3).packing()
        for fv in (lo - 1, hi + 1):
            bad_fill.has_fill, bad_fill.fill = 1, fv
            assert bind(plan, [good if code == hip.I16 else other, bad_fill], [0, 10, T]) == hip.E_INVALID          # a fill outside the storage's range
        plain = af.PackedCube(np.zeros((1,), np.int16), 0.0017, 281.3).packing()
        assert bind(plan, [], [0]) == hip.E_INVALID                           # n == 0
        assert bind(plan, [plain, plain], [1, 10, T]) == hip.E_INVALID        # bounds[0] != 0
        assert bind(plan, [plain, plain], [0, 10, T - 1]) == hip.E_INVALID    # bounds[n] != T
        assert bind(plan, [plain, plain], [0, 10, T + 1]) == hip.E_INVALID
        assert bind(plan, [plain, plain, plain], [0, 10, 10, T]) == hip.E_INVALID      # a repeated bound
        assert bind(plan, [plain, plain, plain], [0, 20, 10, T]) == hip.E_INVALID
        assert bind(plan, [plain] * (T + 1), list(range(T + 2))) == hip.E_INVALID      # more rules than time steps
        with pytest.raises(ValueError, match="strictly increase"):
            plan.bind_packings([plain, plain], [0, 0, T])
        # after every refused bind the earlier binding still holds
        np.testing.assert_array_equal(plan.run_temporal(cube).cpu().numpy(), first)
        # n == 1 is afhip_plan_bind_packing
        single = af.PackedCube(cube.q, 0.0017, 281.3, 5, unsigned=code == hip.U16)
        plan.bind_packing(single.packing())
        a = plan.run_temporal(single).cpu().numpy()
        assert bind(plan, [single.packing()], [0, T]) == 0
        np.testing.assert_array_equal(plan.run_temporal(single).cpu().numpy(), a)
        assert not np.array_equal(a, first, equal_nan=True)
    f32 = hip.FusedPlan(T, n_cells, hip.F32, ib, ob, cols)
    assert bind(f32, [good], [0, T]) == hip.E_INVALID                         # a float32 plan
    with pytest.raises(ValueError, match="AFHIP_I16"):
        f32.bind_packings([good, other], [0, 10, T])


def test_a_bind_does_not_reach_a_run_that_was_already_issued(torch_cuda):
    """`engine._run_fused_pass` re-binds before every run on the same stream: the earlier run keeps the rules it was launched with."""
    from aggfly_amd import hip
    T, n_cells = 24 * 30, 1102
    ib, ob = np.arange(0, T + 1, 24), np.array([0, 30])
    rng = np.random.default_rng(4)
    bits = rng.integers(-32768, 32768, (T, 1, n_cells)).astype(np.int16)
    shapes = _rule_shapes(False)
    b1, b2 = [0, 100, 333, T], [0, 7, 500, 501, T]
    c1 = _cube(torch_cuda, bits, shapes[:3], b1, False)
    c2 = _cube(torch_cuda, bits, shapes[1:5], b2, False)
    plan = hip.FusedPlan(T, n_cells, hip.I16, ib, ob, LIGHT, exact_order=True)
    f32 = hip.FusedPlan(T, n_cells, hip.F32, ib, ob, LIGHT, exact_order=True)
    want1, want2 = (f32.run_temporal(c.materialize()).cpu().numpy() for c in (c1, c2))
    plan.bind_packing(c1)
    r1 = plan.run_temporal(c1).clone()                   # (enqueued; no synchronisation before the next bind)
    plan.bind_packing(c2)
    r2 = plan.run_temporal(c2).clone()
    plan.bind_packing(c1)
    r3 = plan.run_temporal(c1).clone()
    np.testing.assert_array_equal(r1.cpu().numpy(), want1)
    np.testing.assert_array_equal(r2.cpu().numpy(), want2)
    np.testing.assert_array_equal(r3.cpu().numpy(), want1)
    assert not np.array_equal(want1, want2, equal_nan=True)
