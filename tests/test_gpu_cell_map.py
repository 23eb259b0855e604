"""Bins plans whose interior widths differ on the LDS-histogram kernels with FEAT_CELL_MAP (gen_variants.py: cell_map_menu;
afhip_planner.cpp: find_cell_map, choose_hist_variant; afhip_cell_map.h): every kernel of the menu against the oracle, the partition
shapes, the plans that must not move, the A/B knob, multi-rule and uint16 packed cubes, and the whole pass up to the public route.

Bin counts are integers and the compares are the contract's (L < v < U strictly; a value on an edge, NaN and a value on or
beyond an outer limit in no bin; a value on a CELL BOUNDARY that is no edge in its bin like any other), so every count column is held with
ZERO tolerance to the oracle (`block_bins` of the C port, on the host-unpacked values for packed cubes).  The public route's frame —
weighted means of those counts over regions — is held bit for bit between the packed and the float32 route, and to the oracle's frame at
the suite's bar for frames (1e-10 relative: the order of the weighted adds differs).

Only the kernel-name assertions need the new route: the counts are exact on the earlier route as well, which is the point of them.
"""
import json
import os
import zlib

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import synth

import cell_map_recipes as cm
import end_bins_recipes as eb
import packed_hist_recipes as ph
import packed_recipes as pr
import variant_recipes as vr
import test_gpu_packed_hist as hist_mod
import test_gpu_unsigned as uns
from test_gpu_end_bins import _assert_counts
from test_gpu_packed import _run_recipe
from test_gpu_variant_menu import _assert_cells, _csr_table, _oracle_two_level

pytestmark = pytest.mark.gpu
INF = float("inf")

LOADED = vr.menu_of("cell_map", vr.loaded_menu_kind())
MENU = [vr.variant(t) for t in LOADED]
BY_NAME = {v.name: v for v in MENU}
ANY = vr.Variant("bins plan", pr.I16, 0, 1, 1, 16, 16, 8, 0)          # what _assert_cells reads of a variant: its name, not lean
STORAGES = {"f32": vr.F32, "f64": vr.F64, "i16": pr.I16}
DEPTH = {"f32": 8, "f64": 4, "i16": 8}                               # rows in flight of the table forms
KNOBS = ("AFHIP_NO_CELL_MAP_HIST", "AFHIP_NO_END_BINS_HIST", "AFHIP_NO_PACKED_HIST")


@pytest.fixture(autouse=True)
def _no_knob(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _run(torch_cuda, r, seed=0, data=None):
    """(plan, got[K, P, cells], want, values in the cube's precision, stored integers or None) of recipe `r` on its own planted cube."""
    from aggfly_amd import hip
    if eb.is_packed(r.dtype):
        q = cm.stored_cube(r, seed) if data is None else data
        plan, got, want, values = _run_recipe(torch_cuda, r, q)
        return plan, got, want, values, q
    cube = cm.cube_for(r, seed) if data is None else data
    plan = hip.FusedPlan(r.T, r.n_cells, r.dtype, r.inner_bounds, r.outer_bounds, r.columns, exact_order=r.exact_order)
    got = plan.run_temporal(torch_cuda.from_numpy(cube).cuda()).cpu().numpy()
    want = _oracle_two_level(cube.astype(np.float64).reshape(r.T, 1, r.n_cells), r.inner_bounds, r.outer_bounds, r.columns)
    return plan, got, want, cube, None


def _cmap_name(storage, n_cells, sl, stat=0):
    vec = 2 if (storage == "i16" and n_cells % 2 == 0 and sl) else 1
    return f"{storage}_p0_v{vec}_s{stat}_t16_k16_d{DEPTH[storage]}_nt_ibins{'_sl' if sl else ''}_hist_ends_cmap"


def _every_bin_is_met(bins, values):
    for t0, t1 in bins:
        assert ((values > t0) & (values < t1)).sum() > 5, (t0, t1)


# ---- 1. every kernel of the table ----
@pytest.mark.parametrize("name", [v.name for v in MENU])
def test_cell_map_variant_against_the_oracle(torch_cuda, name):
    v = BY_NAME[name]
    r = cm.recipe(v)
    plan, got, want, values, q = _run(torch_cuda, r, seed=zlib.crc32(name.encode()))
    assert vr.plan_name(plan) == name, plan.describe()
    assert f" cells={cm.cells_of(eb.bins_of(r.columns))[1]} " in plan.describe(), plan.describe()
    if v.has(vr.SL):
        assert "packed-counts" in plan.describe() if v.stat == 0 else "packed-counts" not in plan.describe(), plan.describe()
    have = cm.planted(r, values, q)
    assert all(have.values()), {k: ok for k, ok in have.items() if not ok}
    _assert_cells(v, r.columns, got, want)
    _assert_counts(r, got, want, values, name)
    _every_bin_is_met(eb.bins_of(r.columns), values)


def test_the_cases_cover_the_loaded_builds_cell_map_menu(torch_cuda):
    from aggfly_amd import hip
    assert hip.menu_size("cell_map") == len(LOADED) == len(BY_NAME)
    if vr.loaded_menu_kind() != "dev":
        assert {(v.dtype, v.vec) for v in MENU} == {(vr.F32, 1), (vr.F64, 1), (pr.I16, 1), (pr.I16, 2)}


# ---- 2. partition shapes ----
def _lim(x, dtype):
    """An outer limit: on packed cubes the value of a stored integer, so that the cube holds values on it."""
    return pr._snap(x) if eb.is_packed(dtype) else float(x)


def _shape_bins(shape, dtype):
    lim = lambda x: _lim(x, dtype)      # noqa: E731
    eight = [t0 for t0, _ in cm.EIGHT[1:]]                              # -10, 0, 10, 20, 25, 30, 35
    if shape == "closed_six":
        return cm.partition([-10.0, 0.0, 7.5, 10.0, 30.0], lim(-20.0), lim(50.0))
    if shape == "closed_sixteen":
        return cm.partition(cm.edges_from(-25.0, cm.WIDTHS), lim(-40.0), lim(58.0))
    if shape == "open_below":
        return cm.partition(eight, -INF, lim(45.0))
    if shape == "open_above":
        return cm.partition(eight, lim(-30.0), INF)
    if shape == "open_both":
        return list(cm.EIGHT)
    if shape == "finite_wide_ends":
        return cm.partition(eight, lim(-40.0), lim(55.0))
    if shape == "ends_narrower_than_the_smallest_interior_bin":
        return cm.partition(eight, lim(-11.0), lim(36.0))
    if shape == "all_interior_widths_different":
        return cm.partition(cm.edges_from(-12.0, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]), -INF, lim(50.0))
    if shape == "widths_1_to_60":
        return cm.partition(cm.edges_from(-20.0, [30.0, 0.5, 10.0, 5.0, 14.5]), lim(-30.0), INF)          # 240 cells
    if shape == "edges_of_tenths":
        return cm.partition([0.1 * k for k in (0, 3, 5, 10, 12, 20, 50, 70)], -INF, INF)
    if shape == "edges_off_250.15":
        base = 45.15 if eb.is_packed(dtype) else 250.15                 # (a packed cube's values end at 63.8)
        return cm.partition([base + x for x in (0.0, 1.0, 2.0, 4.0, 5.0, 7.0, 10.0)], lim(base - 20.0), INF)
    raise KeyError(shape)


SHAPES = ["closed_six", "closed_sixteen", "open_below", "open_above", "open_both", "finite_wide_ends",
          "ends_narrower_than_the_smallest_interior_bin", "all_interior_widths_different", "widths_1_to_60", "edges_of_tenths", "edges_off_250.15"]


@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("shape", SHAPES)
def test_partition_shapes(torch_cuda, shape, storage):
    dtype = STORAGES[storage]
    bins = _shape_bins(shape, dtype)
    sl = SHAPES.index(shape) % 2 == 0
    odd = SHAPES.index(shape) % 3 == 0
    n_cells = (1101 if odd else 1102) if eb.is_packed(dtype) else (60 if odd else 64)
    seed = zlib.crc32(f"{shape} {storage}".encode())
    r = cm.make_recipe("", dtype, n_cells, bins, sl, False, seed=seed)          # (columns in an order shuffled per case)
    assert [c["inner_args"][:2] for c in r.columns] != sorted(c["inner_args"][:2] for c in r.columns)
    plan, got, want, values, q = _run(torch_cuda, r, seed)
    assert vr.plan_name(plan) == _cmap_name(storage, n_cells, sl), plan.describe()
    have = cm.planted(r, values, q)
    assert all(have.values()), {k: ok for k, ok in have.items() if not ok}
    _every_bin_is_met(bins, values)
    _assert_counts(r, got, want, values, f"{shape} {storage}")


# ---- 3. what must not move ----
@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("ends", ["closed", "open"])
def test_equal_width_plans_keep_their_kernels(torch_cuda, ends, storage):
    dtype = STORAGES[storage]
    lat = eb.lattice(dtype, 13)
    bins = eb.with_ends(lat) if ends == "closed" else eb.with_ends(lat, -INF, INF)
    r = eb.make_recipe("", dtype, 1101 if eb.is_packed(dtype) else 60, bins, True, False)
    plan, got, want, values, _ = _run(torch_cuda, r, 3)
    depth = {"f32": 8, "f64": 4, "i16": 16}[storage]
    assert vr.plan_name(plan) == f"{storage}_p0_v1_s0_t16_k16_d{depth}_nt_ibins_sl_hist_arith" + ("_ends" if ends == "open" else ""), plan.describe()
    _assert_counts(r, got, want, values, f"{ends} {storage}")


def _off_route_cases():
    cols = lambda bins: [dict(inner="bins", inner_args=(t0, t1, 0.0), outer="sum") for t0, t1 in bins]      # noqa: E731
    w = 2.0 ** -14
    narrow = [300.0 + 2.0 ** -15 + w * k for k in (0, 1, 3, 4, 6, 7, 9)]      # interior bins of two and four float32 ulps at 300
    return {
        "five_bins": cols([(-20.0, 0.0), (0.0, 7.5), (7.5, 10.0), (10.0, 30.0), (30.0, 99.0)]),
        "a_gap": cols([b for i, b in enumerate(cm.EIGHT) if i != 3]),
        "a_degree_day_slot_beside_the_bins": cols(cm.EIGHT) + [dict(inner="dd", inner_args=(-10.0, 20.0, 0.0), outer="sum")],
        "ratio_over_127": cols(cm.partition(cm.edges_from(-25.0, [0.25, 40.0, 10.0, 5.0, 9.75]), -INF, INF)),          # 260 cells
        "widths_of_a_few_ulps": cols(cm.partition(narrow, -INF, INF)),
    }


@pytest.mark.parametrize("storage", ["f32", "i16"])
@pytest.mark.parametrize("case", list(_off_route_cases()))
def test_other_plans_stay_off_the_cell_map_route(torch_cuda, case, storage):
    dtype = STORAGES[storage]
    cols = _off_route_cases()[case]
    ib, ob = ph.groups(False)
    es = sorted({float(x) for c in cols for x in c["inner_args"][:2] if np.isfinite(x)})
    seed = zlib.crc32(case.encode())
    if eb.is_packed(dtype) and case == "widths_of_a_few_ulps":
        # values 300 + q / 16384, exact in float32: a stored integer or two per narrow bin (as in test_gpu_end_bins)
        r = vr.Recipe("", dtype, int(ib[-1]), 1102, ib, ob, cols, True, 0, edges=[12.0])
        q = ph.stored_cube(r, seed)
        q[::5, ::9] = np.random.default_rng(1).integers(-2, 12, q[::5, ::9].shape).astype(np.int16)
        plan, got, want, values = _run_recipe(torch_cuda, r, q, pairs=[(2.0 ** -14, 300.0)])
    else:
        r = vr.Recipe("", dtype, int(ib[-1]), 1102 if eb.is_packed(dtype) else 64, ib, ob, cols, True, 0, edges=es)
        plan, got, want, values, _ = _run(torch_cuda, r, seed)
    name = vr.plan_name(plan)
    assert "_hist" not in name and "_ends" not in name and "_cmap" not in name and " cells=" not in plan.describe().split(" | ")[0], plan.describe()
    if storage == "i16":
        assert name.startswith("i16_p0_v2_") and name.endswith("_nt") and "_ibins" not in name, plan.describe()
    elif case != "a_degree_day_slot_beside_the_bins":
        assert "_ibins" in name, plan.describe()
    for k in range(len(cols)):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{case} column {k}")


@pytest.mark.parametrize("storage", list(STORAGES))
@pytest.mark.parametrize("single_level,mean", [(True, False), (False, True)], ids=["sl", "two_level_mean"])
def test_knob_sends_the_plan_down_the_earlier_route_with_the_same_counts(torch_cuda, monkeypatch, single_level, mean, storage):
    dtype = STORAGES[storage]
    n_cells = 1102 if eb.is_packed(dtype) else 64
    r = cm.make_recipe("", dtype, n_cells, list(cm.EIGHT), single_level, mean)
    data = cm.stored_cube(r, 9) if eb.is_packed(dtype) else cm.cube_for(r, 9)
    plan, got, want, values, _ = _run(torch_cuda, r, data=data)
    assert vr.plan_name(plan) == _cmap_name(storage, n_cells, single_level, int(mean)), plan.describe()
    monkeypatch.setenv("AFHIP_NO_CELL_MAP_HIST", "1")
    earlier, got_e, _, _, _ = _run(torch_cuda, r, data=data)
    monkeypatch.delenv("AFHIP_NO_CELL_MAP_HIST")
    name = vr.plan_name(earlier)
    assert "_hist" not in name and "_ends" not in name and "_cmap" not in name, earlier.describe()
    if storage == "i16":
        assert name.startswith(f"i16_p0_v2_s{int(mean)}_") and name.endswith("_nt") and "packed-counts" not in earlier.describe(), earlier.describe()
    else:
        assert name.startswith(f"{storage}_p0_") and f"_s{int(mean)}_" in name and "_ibins" in name and ("_sl" in name) == single_level, earlier.describe()
    np.testing.assert_array_equal(got[:8], got_e[:8])                 # the counts, bit for bit (NaN where the other has NaN)
    _assert_cells(ANY, r.columns, got_e, want)
    _assert_counts(r, got, want, values, f"knob {storage}")


# ---- 4. packed specifics ----
UNEQUAL5 = cm.partition([-19.85, -10.05, -5.15, -0.25, 9.55, 14.45, 19.35, 29.15, 34.05, 43.85], -INF, 60.0)      # widths 9.8 and 4.9


@pytest.mark.parametrize("single_level", [False, True], ids=["two_level", "sl"])
@pytest.mark.parametrize("n_cells", [1102, 1101])
def test_rule_changes_wherever_they_can_fall(torch_cuda, n_cells, single_level):
    """The cube, the rules and the places of the rule changes of test_gpu_end_bins.py::test_rule_changes_wherever_they_can_fall."""
    from aggfly_amd import hip
    cube, values64, bits = hist_mod._case5(n_cells)
    T5, IB5 = hist_mod.T5, hist_mod.IB5
    assert cube.n_rules == len(hist_mod.BOUNDS5) - 1 >= 3
    ob = np.arange(len(IB5), dtype=np.int64) if single_level else np.arange(0, 41, 8, dtype=np.int64)
    cols = eb.bin_columns(UNEQUAL5, "identity" if single_level else "sum", mean=not single_level)
    plan = hip.FusedPlan(T5, n_cells, hip.I16, IB5, ob, cols, exact_order=True)
    plan.bind_packing(cube)
    assert vr.plan_name(plan) == _cmap_name("i16", n_cells, single_level, 0 if single_level else 1), plan.describe()
    got = plan.run_temporal(cube).cpu().numpy()
    want = _oracle_two_level(values64, IB5, ob, cols)
    _assert_cells(ANY, cols, got, want)
    r = vr.Recipe("", pr.I16, T5, n_cells, IB5, ob, cols, True, 0)
    _assert_counts(r, got, want, values64, "rules")
    for t0, t1 in UNEQUAL5:                                            # every bin is met, under several rules
        assert ((values64 > t0) & (values64 < t1)).sum() > 100, (t0, t1)


def test_uint16_storage_takes_the_same_kernels(torch_cuda):
    from aggfly_amd import hip
    pairs, fill = uns.PAIRS, 65535                        # value(q) = q * 0.001 + 252.4 - 273.15: -20.75 ... 44.79 C
    near = lambda x: uns.stored_near(x, pairs)            # noqa: E731
    val = lambda x: float(uns.np_unpack([near(x)], pairs, None)[0])      # noqa: E731
    bins = cm.partition([-14.85, -7.45, -3.75, -0.05, 7.35, 11.05, 22.15, 25.85, 33.25], val(-19.0), val(43.0))      # widths 3.7, 7.4, 11.1
    ib, ob = ph.groups(True)
    cols = eb.bin_columns(bins, "identity")
    T, C = int(ib[-1]), 1102
    rng = np.random.default_rng(6)
    q = rng.integers(0, 65536, (T, C)).astype(np.uint16)
    every = sorted({x for b in bins for x in b} | set(cm.cells_of(bins)[2]))
    plant = [0, 1, 32767, 32768, 65534] + [s + d for x in every for s in [near(x)] for d in (-3, -2, -1, 0, 1, 2, 3)]
    q.reshape(-1)[rng.choice(q.size, 20 * len(plant), replace=False)] = np.array(plant * 20, dtype=np.uint16)
    ne = np.flatnonzero(np.diff(ib) > 0)
    q[ib[ne[::5]], 40:60] = fill                                   # the fill in first rows of groups
    for g in ne[2::7]:
        q[ib[g]:ib[g + 1], 100:104] = fill                        # in whole groups
    q[:, [3, C - 1]] = fill                                        # in whole cells, the last one included
    cube = uns._cuda_cube(torch_cuda, q.reshape(T, 1, C), scale_factor=pairs[0][0], add_offset=pairs[0][1], fill_value=fill) - 273.15
    plans = {}
    for code, c in ((hip.U16, cube), (hip.I16, af.PackedCube(cube.q, fill_value=-1, unsigned=False, _pairs=cube.pairs))):
        plan = hip.FusedPlan(T, C, code, ib, ob, cols, exact_order=True)
        plan.bind_packing(c)
        plans[code] = plan
    pu = plans[hip.U16]
    assert vr.plan_name(pu) == vr.plan_name(plans[hip.I16]) == _cmap_name("i16", C, True), pu.describe()
    assert "storage=uint16" in pu.describe() and "storage=int16" in plans[hip.I16].describe()
    values = uns.np_unpack(q, pairs, fill)
    assert (q > 32767).mean() > 0.4 and np.isnan(values).sum() == (q == fill).sum() > 2 * T
    assert (values == np.float32(bins[0][0])).any() and (values < np.float32(bins[0][0])).any() and (values > np.float32(bins[-1][1])).any()
    got = pu.run_temporal(cube).cpu().numpy()
    want = _oracle_two_level(values.astype(np.float64).reshape(T, 1, C), ib, ob, cols)
    r = vr.Recipe("", pr.I16, T, C, ib, ob, cols, True, 0)
    _assert_counts(r, got, want, values, "uint16")


# ---- 5. the whole pass ----
@pytest.mark.parametrize("storage", list(STORAGES))
def test_whole_pass_direct_gather_and_cell_major_panel_agree(torch_cuda, storage):
    from aggfly_amd import hip
    dtype = STORAGES[storage]
    n_cells = 1102 if eb.is_packed(dtype) else 64
    r = cm.make_recipe("", dtype, n_cells, list(cm.EIGHT), True, False)
    if eb.is_packed(dtype):
        q = cm.stored_cube(r, 4)
        values = pr.np_unpack(q)
        d = af.PackedCube(torch_cuda.from_numpy(q.reshape(r.T, 1, r.n_cells)).cuda(), scale_factor=pr.PAIRS[0][0], add_offset=pr.PAIRS[0][1],
                          fill_value=pr.FILL) + pr.PAIRS[1][1]
    else:
        values = cm.cube_for(r, 4)
        d = torch_cuda.from_numpy(values).cuda()
    plan = hip.FusedPlan(r.T, r.n_cells, hip.I16 if eb.is_packed(dtype) else dtype, r.inner_bounds, r.outer_bounds, r.columns, exact_order=True)
    if eb.is_packed(dtype):
        plan.bind_packing(d)
    assert vr.plan_name(plan) == _cmap_name(storage, n_cells, True) and "packed-counts" in plan.describe(), plan.describe()
    tab = _csr_table(r.n_cells, seed=5)
    csr = hip.CSR(tab["index_right"].to_numpy(), tab["cell_id"].to_numpy(), tab["weight"].to_numpy(), int(tab["index_right"].max()) + 1, r.n_cells)
    direct = plan.run(d, csr, want_cells=False)
    via_panel = plan.run(d, csr, want_cells=True)
    for key in ("num", "den", "res"):
        np.testing.assert_array_equal(direct[key].cpu().numpy(), via_panel[key].cpu().numpy(), err_msg=key)
    want = _oracle_two_level(values.astype(np.float64).reshape(r.T, 1, r.n_cells), r.inner_bounds, r.outer_bounds, r.columns)
    np.testing.assert_array_equal(via_panel["cells"].cpu().numpy(), want)


def test_eight_bin_spec_through_the_public_api(torch_cuda, tmp_path):
    from aggfly_amd import engine as eng
    from aggfly_amd import io as afio
    from oracle import ref_aggregate as ra
    T, ny, nx = 24 * 20, 25, 44                                        # 1,100 cells, twenty days over a new year: two yearly periods
    rng = np.random.default_rng(12)
    per_deg = 1.0 / 0.0017
    stored = np.clip(np.rint(pr.stored_near(12.0) + rng.normal(0.0, 14.0, (T, ny, nx)) * per_deg), -32766, 32766).astype(np.int16)
    stored[rng.random((T, ny, nx)) < 0.01] = -32767
    stored[:, 2, 3] = -32767                                            # an ocean cell
    edges = [t0 for t0, _ in cm.EIGHT[1:]]
    for x in edges + cm.cells_of(cm.EIGHT)[2]:                          # the stored integers around every edge and every cell boundary
        s = pr.stored_near(x)
        stored.reshape(-1)[rng.choice(stored.size, 30, replace=False)] = np.array([s - 1, s, s + 1] * 10, dtype=np.int16)
    attrs = {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}
    time = pd.date_range("2003-12-22", periods=T, freq="h")
    lat, lon = 35 + 0.25 * np.arange(ny), 250 + 0.25 * np.arange(nx)
    tv, tattrs = afio._encode_time(time)
    store = str(tmp_path / "bins.zarr")
    os.makedirs(store)
    json.dump({"zarr_format": 2}, open(os.path.join(store, ".zgroup"), "w"))
    afio._write_array(store, "t2m", stored, ("time", "latitude", "longitude"), (48, ny, nx), attrs, None)
    afio._write_array(store, "time", np.asarray(tv, dtype=np.float64), ("time",), (T,), tattrs, None)
    afio._write_array(store, "latitude", lat, ("latitude",), (ny,), {}, None)
    afio._write_array(store, "longitude", lon, ("longitude",), (nx,), {}, None)
    celsius = lambda x: x - 273.15                                      # noqa: E731
    packed = af.dataset_from_path(store, "t2m", device="cuda", keep_packed=True, preprocess=celsius)
    plain = af.dataset_from_path(store, "t2m", device="cuda", preprocess=celsius)
    assert packed.is_packed and not plain.is_packed
    tab = synth.weights_table(ny, nx, 20, seed=3, secondary=True)
    regions = pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]})
    gr = af.GeoRegions(regions, regionid="geoid")
    ddargs = [[t0, t1, 0] for t0, t1 in cm.EIGHT]
    spec = dict(bins=[("aggregate", {"calc": "bins", "groupby": "year", "ddargs": ddargs})])
    frames, descs = {}, {}
    for key, ds in (("packed", packed), ("plain", plain)):
        eng._PLAN_CACHE.clear()
        frames[key] = af.aggregate_dataset(dataset=ds, weights=af.weights_from_objects(ds, gr, table=tab), **spec)
        plans = list(eng._PLAN_CACHE.values())
        assert len(plans) == 1
        descs[key] = plans[0].describe()
    dp, df = descs["packed"], descs["plain"]
    assert "variant=i16_p0_v2_s0_t16_k16_d8_nt_ibins_sl_hist_ends_cmap " in dp and " cells=18 " in dp and "packed-counts" in dp and "storage=int16" in dp, dp
    assert "variant=f32_p0_v1_s0_t16_k16_d8_nt_ibins_sl_hist_ends_cmap " in df and " cells=18 " in df and "packed-counts" in df, df
    last = lambda d: [w for w in d.split() if w.startswith("last-run=")]      # noqa: E731
    assert last(dp) == last(df) and last(dp), (dp, df)                  # the same spatial route: the frames must agree in every bit
    cols = [c for c in frames["packed"].columns if c not in ("geoid", "time")]
    assert len(cols) == 8 and frames["packed"]["time"].nunique() == 2
    pd.testing.assert_frame_equal(frames["packed"], frames["plain"], check_exact=True)
    # ... and the oracle's frame, on the host-unpacked float32 values
    values = pr.np_unpack(stored.reshape(T, -1)).reshape(T, ny, nx)
    ow = ra.OWeights(tab, np.arange(ny * nx), regions["geoid"], "geoid", "nan")
    want = ra.aggregate_dataset(ow, ra.ODataset(values.astype(np.float64), time, lat, lon, True), engine="numba", **spec)
    assert list(frames["plain"].columns) == list(want.columns) and len(want) == len(frames["plain"])
    np.testing.assert_allclose(frames["plain"][cols].values, want[cols].values, rtol=1e-10, atol=0, equal_nan=True)      # the suite's bar for a frame against the oracle's
    assert (np.nansum(frames["plain"][cols].values, axis=0) > 0).all()         # every bin, the open ones included, holds values
