"""Packed cubes' bins plans on the LDS-histogram kernels (gen_variants.py: packed_hist_menu; afhip_planner.cpp:
choose_hist_variant): every kernel of the menu against the oracle, the edge-table form, the plans that must stay on the general
packed kernels, the A/B knob, rule changes wherever they can fall, uint16 storage, and the public route.

Bin counts are integers far below 2^53 and the compares are the contract's (a float32 value against the float32
neighbours of a double edge), so every count column is held with ZERO tolerance — to the oracle on the host-unpacked values, to the
general packed kernel, and to the float32 route.  The mean column of the stat-1 kernels is held as `_assert_cells` holds it (bit for
bit under exact_order).
"""
import functools
import json
import os
import re
import zlib

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import synth

import packed_hist_recipes as ph
import packed_recipes as pr
import variant_recipes as vr
import test_gpu_packed_rules as rules_mod
import test_gpu_unsigned as uns
from test_gpu_packed import _run_recipe
from test_gpu_variant_menu import _assert_cells, _oracle_two_level

pytestmark = pytest.mark.gpu


LOADED = vr.menu_of("packed_hist", vr.loaded_menu_kind())
MENU = [vr.variant(t) for t in LOADED if t[8]]          # the production kernels: what the planner picks by its own rule
BY_NAME = {v.name: v for v in MENU}
ANY = vr.Variant("packed bins plan", pr.I16, 0, 1, 1, 16, 16, 8, 0)          # what _assert_cells reads of a variant: its name, not lean


def _vec(n_cells, single_level, arith):
    """Cells per lane the planner takes: the widest that divides the rows and that the production menu holds for the form."""
    return max(v.vec for v in MENU if n_cells % v.vec == 0 and v.has(vr.SL) == single_level and v.has(vr.HA) == arith)


# ---- 1. every kernel of the menu ----
@pytest.mark.parametrize("name", [v.name for v in MENU])
def test_packed_hist_variant_against_the_oracle(torch_cuda, name):
    v = BY_NAME[name]
    r = ph.recipe(v)
    q = ph.stored_cube(r, seed=zlib.crc32(name.encode()))
    plan, got, want, values = _run_recipe(torch_cuda, r, q)
    assert vr.plan_name(plan) == name and "storage=int16" in plan.describe(), plan.describe()
    if v.has(vr.SL):
        assert "packed-counts" in plan.describe() if v.stat == 0 else "packed-counts" not in plan.describe(), plan.describe()
    # the data: stored integers on an edge (arithmetic plans), next to every edge, in both guard bins, the extremes, whole groups of fills
    e = np.array(r.edges)
    on = ph.stored_on_edges(r.edges)
    assert bool(on) == v.has(vr.HA) and all((values == np.float32(x)).any() for x in on)
    assert (values < e[0]).any() and (values > e[-1]).any() and {32767, -32768} <= set(np.unique(q).tolist())
    ib = r.inner_bounds
    assert any(np.isnan(values[ib[g]:ib[g + 1]]).all(axis=0).any() for g in range(len(ib) - 1) if ib[g + 1] > ib[g])
    _assert_cells(v, r.columns, got, want)
    for k, c in enumerate(r.columns):
        if c["inner"] == "bins":
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{name} column {k}")       # zero tolerance, said once more


def test_the_cases_cover_the_loaded_builds_packed_hist_menu(torch_cuda):
    from aggfly_amd import hip
    assert hip.build_info()["packed_hist_variants"] == len(LOADED) and len(MENU) == len(BY_NAME) == sum(t[8] for t in LOADED)
    assert {v.vec for v in MENU} == {1, 2}                  # one cell per lane and two are both exercised above


# ---- 2. the edge table: edges float32 cannot hold ----
def _plan_case(n_cells, edges, single_level=False, mean=False, extra=(), seed=5):
    ib, ob = ph.groups(single_level)
    cols = ph.bin_columns(edges, "identity" if single_level else "sum", mean=mean) + list(extra)
    es = sorted({float(x) for c in cols if c["inner"] in ("bins", "dd") for x in c["inner_args"][:2]})
    r = vr.Recipe("", pr.I16, int(ib[-1]), n_cells, ib, ob, cols, True, 0, edges=es)
    return r, ph.stored_cube(r, seed)


@pytest.mark.parametrize("n_cells,single_level", [(1102, True), (1102, False), (1101, False)])
def test_inexact_edges_take_the_table_form(torch_cuda, n_cells, single_level):
    edges = 0.05 + 0.1 * np.arange(15)                      # width 0.1 from 0.05: fourteen bins between 0.05 and 1.45 C
    r, q = _plan_case(n_cells, edges, single_level)
    vec = _vec(n_cells, single_level, False)
    assert vec == (2 if (n_cells, single_level) == (1102, True) else 1)          # (profiles/packed_cube.txt, section 6)
    lo, hi = pr.stored_near(-0.1), pr.stored_near(1.6)       # a tenth of the cube inside and around the fourteen bins
    q[::3, 7::11] = np.random.default_rng(n_cells).integers(lo, hi, q[::3, 7::11].shape).astype(np.int16)
    plan, got, want, values = _run_recipe(torch_cuda, r, q)
    name = vr.plan_name(plan)
    assert name.startswith(f"i16_p0_v{vec}_s0_") and "_hist" in name and "_arith" not in name and ("_sl_" in name) == single_level, plan.describe()
    assert all(((values > np.float32(a)) & (values < np.float32(b))).sum() > 50 for a, b in zip(edges[:-1], edges[1:]))   # every bin is met
    for k in range(len(r.columns)):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"column {k}")


# ---- 3. what stays on the general packed kernels ----
def _fallback_cases():
    a = ph.arith_edges(13)
    e0 = float(a[0])
    gap = [dict(inner="bins", inner_args=(float(a[i]), float(a[i + 1]), 0.0), outer="sum") for i in (0, 1, 2, 4, 5, 6)]      # bin 3 is missing
    poison = ph.bin_columns(a[:6], "sum")
    poison[2] = dict(inner="dd", inner_args=poison[2]["inner_args"], outer="sum")           # a degree-day slot poisons on NaN
    # six bins of two float32 ulps at 300 (emax * eps * 16 = 5.8e-4 >= w = 6.1e-5), their edges half way between the stored values
    w = 2.0 ** -14
    narrow = 300.0 + 2.0 ** -15 + w * np.arange(7)
    return {
        "three_bins": ph.bin_columns(a[:4], "sum"),
        "bins_beside_degree_days": ph.bin_columns(a, "sum") + [dict(inner="dd", inner_args=(e0, e0 + 30.0, 0.0), outer="sum")],
        "not_contiguous": gap,
        "nan_poisoning_slot": poison,
        "too_narrow_for_the_guess": ph.bin_columns(narrow, "sum"),
    }


@pytest.mark.parametrize("case", list(_fallback_cases()))
def test_other_plans_stay_on_the_general_kernels(torch_cuda, case):
    cols = _fallback_cases()[case]
    ib, ob = ph.groups(False)
    es = sorted({float(x) for c in cols for x in c["inner_args"][:2]})
    r = vr.Recipe("", pr.I16, int(ib[-1]), 1102, ib, ob, cols, True, 0, edges=[x for x in es if x < 100.0])
    q = ph.stored_cube(r, seed=zlib.crc32(case.encode()))
    pairs = pr.PAIRS
    if case == "too_narrow_for_the_guess":
        pairs = [(2.0 ** -14, 300.0)]                      # values 300 + q / 16384, exact in float32: one stored integer per bin
        q[::5, ::9] = np.random.default_rng(1).integers(-2, 9, q[::5, ::9].shape).astype(np.int16)
    plan, got, want, values = _run_recipe(torch_cuda, r, q, pairs=pairs)
    name = vr.plan_name(plan)
    assert name.startswith("i16_p0_v2_") and name.endswith("_nt") and "_hist" not in name and "_ibins" not in name, plan.describe()
    if case == "too_narrow_for_the_guess":
        assert sum(np.nansum(want[k]) for k in range(len(cols))) > 100
    for k in range(len(cols)):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{case} column {k}")


# ---- 4. the knob ----
@pytest.mark.parametrize("single_level,mean", [(True, False), (False, True)], ids=["sl", "two_level_mean"])
def test_knob_sends_the_plan_to_the_general_kernel_with_the_same_bits(torch_cuda, monkeypatch, single_level, mean):
    from aggfly_amd import hip
    r, q = _plan_case(1102, ph.arith_edges(13), single_level, mean)
    plan, got, want, _ = _run_recipe(torch_cuda, r, q)
    assert "_hist_arith" in vr.plan_name(plan) and ("_sl_" in vr.plan_name(plan)) == single_level, plan.describe()
    monkeypatch.setenv("AFHIP_NO_PACKED_HIST", "1")
    general, got_g, _, _ = _run_recipe(torch_cuda, r, q)
    monkeypatch.delenv("AFHIP_NO_PACKED_HIST")
    tier = f"i16_p0_v2_s{int(mean)}_t16_k16_d16_nt"
    assert vr.plan_name(general) == tier and "packed-counts" not in general.describe(), general.describe()
    assert got.dtype == got_g.dtype == np.float64
    np.testing.assert_array_equal(got, got_g)              # bit for bit (counts and means; NaN where the other has NaN)
    _assert_cells(ANY, r.columns, got, want)
    # ... and so does the float32 route on the unpacked values (the single-level LDS-histogram kernel of the float menu)
    f32 = hip.FusedPlan(r.T, r.n_cells, hip.F32, r.inner_bounds, r.outer_bounds, r.columns, exact_order=True)
    assert "_hist" in vr.plan_name(f32), f32.describe()
    vals = torch_cuda.from_numpy(pr.np_unpack(q).reshape(r.T, 1, r.n_cells)).cuda()
    np.testing.assert_array_equal(f32.run_temporal(vals).cpu().numpy(), got)


# ---- 5. several rules ----
T5 = 24 * 40
# rule changes: inside a burst (1, 2, 3, 5; 55 = day 2 + 7), at group ends (24, 192, 240), one-row rules (80-81, 81-82), mid-group
# (503 = day 20 + 23), the last row; 192 and 240 start chunks (two-level: periods of eight days, one chunk each; sl: chunks of two days)
CHANGES5 = [1, 2, 3, 5, 24, 24 * 2 + 7, 24 * 3 + 8, 24 * 3 + 9, 24 * 3 + 10, 192, 240, 24 * 20 + 23, T5 - 1]
BOUNDS5 = [0] + CHANGES5 + [T5]
IB5 = np.arange(0, T5 + 1, 24, dtype=np.int64)
EDGES5 = -20.0 + 5.0 * np.arange(14)                      # thirteen bins of 5 C; integers: arithmetic edges
TABLE5 = -19.85 + 4.9 * np.arange(14)


def _rules5():
    shapes = rules_mod._rule_shapes(False)[:4]            # different scale / offset / fill, two and three pairs: one stored integer, different bins
    return [shapes[i % len(shapes)] for i in range(len(BOUNDS5) - 1)]


@functools.lru_cache(maxsize=None)
def _case5(n_cells):
    import torch
    rules = _rules5()
    bits = rules_mod._stored(T5, n_cells, BOUNDS5, rules, seed=n_cells)
    cube = rules_mod._cube(torch, bits.reshape(T5, 1, n_cells), rules, BOUNDS5, False)
    values = rules_mod._np_values(bits, rules, BOUNDS5, False)             # per-rule numpy float32 chains: the oracle's input
    return cube, values.astype(np.float64).reshape(T5, 1, n_cells), bits


def test_one_stored_integer_falls_into_different_bins_under_different_rules():
    sh = rules_mod._rule_shapes(False)[:4]
    q = np.array([2000], dtype=np.int16)
    bins = {int(np.searchsorted(EDGES5, float(rules_mod._np_unpack(q, p, f, False)[0]))) for p, f in sh}
    assert len(bins) >= 2, bins


@pytest.mark.parametrize("single_level", [False, True], ids=["two_level", "sl"])
@pytest.mark.parametrize("form", ["arith", "table"])
@pytest.mark.parametrize("n_cells", [1102, 1101])
def test_rule_changes_wherever_they_can_fall(torch_cuda, n_cells, form, single_level):
    from aggfly_amd import hip
    cube, values64, bits = _case5(n_cells)
    assert cube.n_rules == len(BOUNDS5) - 1 >= 3
    ob = np.arange(len(IB5), dtype=np.int64) if single_level else np.arange(0, 41, 8, dtype=np.int64)
    cols = ph.bin_columns(EDGES5 if form == "arith" else TABLE5, "identity" if single_level else "sum", mean=not single_level)
    plan = hip.FusedPlan(T5, n_cells, hip.I16, IB5, ob, cols, exact_order=True)
    plan.bind_packing(cube)
    d = plan.describe()
    want_name = f"i16_p0_v{_vec(n_cells, single_level, form == 'arith')}_s{0 if single_level else 1}_t16_k16_"
    assert vr.plan_name(plan).startswith(want_name) and "_hist" in d and ("_arith" in d) == (form == "arith") and ("_sl_" in d) == single_level, d
    # three chunks and more, all of one length that divides 192 and 240: rules change at chunk starts, and chunks start inside rules
    n_chunks, lo, hi = (int(x) for x in re.search(r"chunks=(\d+) \(steps (\d+)\.\.(\d+)\)", d).groups())
    assert n_chunks >= 3 and lo == hi == T5 // n_chunks and 192 % lo == 0 and (240 % lo == 0 or not single_level), d
    got = plan.run_temporal(cube).cpu().numpy()
    want = _oracle_two_level(values64, IB5, ob, cols)
    _assert_cells(ANY, cols, got, want)
    assert np.nansum(want[:13]) > 0.4 * np.isfinite(values64).sum()            # the thirteen bins hold a good part of the values


# ---- 6. uint16 storage ----
@pytest.mark.parametrize("form", ["arith", "table"])
def test_uint16_storage_takes_the_same_kernels(torch_cuda, form):
    from aggfly_amd import hip
    pairs, fill = uns.PAIRS, 65535                        # value(q) = q * 0.001 + 252.4 - 273.15: -20.75 ... 44.79 C
    near = lambda x: uns.stored_near(x, pairs)            # noqa: E731
    if form == "arith":
        e0 = float(uns.np_unpack([near(-15.0)], pairs, None)[0])
        edges = e0 + 4.0 * np.arange(15)
    else:
        edges = -14.85 + 3.7 * np.arange(15)
    ib, ob = ph.groups(True)
    cols = ph.bin_columns(edges, "identity")
    T, C = int(ib[-1]), 1102
    rng = np.random.default_rng(6)
    q = rng.integers(0, 65536, (T, C)).astype(np.uint16)
    plant = [0, 1, 32767, 32768, 65534] + [s + d for x in edges for s in [near(x)] for d in (-1, 0, 1)]
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
    name = vr.plan_name(pu)
    assert name == vr.plan_name(plans[hip.I16]) and "_sl_hist" in name and ("_arith" in name) == (form == "arith"), pu.describe()
    assert "storage=uint16" in pu.describe() and "storage=int16" in plans[hip.I16].describe()
    values = uns.np_unpack(q, pairs, fill)
    assert (q > 32767).mean() > 0.4 and np.isnan(values).sum() == (q == fill).sum() > 2 * T
    assert form == "table" or (values == np.float32(edges[0])).any()
    got = pu.run_temporal(cube).cpu().numpy()
    want = _oracle_two_level(values.astype(np.float64).reshape(T, 1, C), ib, ob, cols)
    for k in range(len(cols)):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"column {k}")
    assert sum(np.nansum(want[k]) for k in range(len(cols))) > 0.7 * np.isfinite(values).sum()


# ---- 7. the public route ----
def test_keep_packed_bins_spec_through_the_public_api(torch_cuda, tmp_path):
    from aggfly_amd import engine as eng
    from aggfly_amd import io as afio
    T, ny, nx = 24 * 20, 25, 44                                        # 1,100 cells, twenty days over a new year: two yearly periods
    rng = np.random.default_rng(12)
    per_deg = 1.0 / 0.0017
    stored = np.clip(np.rint(pr.stored_near(12.0) + rng.normal(0.0, 14.0, (T, ny, nx)) * per_deg), -32766, 32766).astype(np.int16)
    stored[rng.random((T, ny, nx)) < 0.01] = -32767
    stored[:, 2, 3] = -32767                                            # an ocean cell
    edges = [float(x) for x in -20.0 + 5.0 * np.arange(14)]
    for x in edges:                                                     # the stored integers around every edge
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
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}), regionid="geoid")
    spec = dict(bins=[("aggregate", {"calc": "bins", "groupby": "year", "ddargs": [[a, b, 0] for a, b in zip(edges[:-1], edges[1:])]})])
    frames, descs = {}, {}
    for key, ds in (("packed", packed), ("plain", plain)):
        eng._PLAN_CACHE.clear()
        frames[key] = af.aggregate_dataset(dataset=ds, weights=af.weights_from_objects(ds, gr, table=tab), **spec)
        plans = list(eng._PLAN_CACHE.values())
        assert len(plans) == 1
        descs[key] = plans[0].describe()
    dp, df = descs["packed"], descs["plain"]
    assert f"variant=i16_p0_v{_vec(ny * nx, True, True)}_s0_t16_k16_" in dp and "_sl_hist_arith" in dp and "packed-counts" in dp and "last-run=count-gather" in dp and "storage=int16" in dp, dp
    assert "variant=f32_" in df and "_sl_hist" in df and "packed-counts" in df, df
    last = lambda d: [w for w in d.split() if w.startswith("last-run=")]      # noqa: E731
    assert last(dp) == last(df) and last(dp), (dp, df)                  # the same spatial route: the frames must agree in every bit
    cols = [c for c in frames["packed"].columns if c not in ("geoid", "time")]
    assert len(cols) == 13 and frames["packed"]["time"].nunique() == 2
    pd.testing.assert_frame_equal(frames["packed"], frames["plain"], check_exact=True)
    assert np.isfinite(frames["packed"][cols].values).any() and (frames["packed"][cols].values > 0).any()
