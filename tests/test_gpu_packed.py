"""int16-packed cubes on the GPU: the unpack rule over every stored value, every kernel of the packed menu against the oracle,
the planner's choice of cells per lane by row length, what the library refuses, and the public route (`keep_packed`) against
the default float32 route and the oracle.

The oracle of a packed plan is `cport` on the cube unpacked on the host in numpy float32, one rounded operation at a time
(`packed_recipes.np_unpack`): the kernels must reproduce that chain bit for bit, so the bars are those of the float32 kernels
(test_gpu_variant_menu.py: bit-exact statistics / dd / bins under exact_order, 4e-16 for integer powers, 1e-10 for sine_dd).
"""
import json
import os
import zlib

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import synth
from oracle import ref_aggregate as ra

import packed_recipes as pr
import variant_recipes as vr
from test_gpu_variant_menu import _assert_cells, _oracle_two_level

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdf5")


MENU = [vr.variant(v) for v in vr.menu_of("packed", vr.loaded_menu_kind())]
BY_NAME = {v.name: v for v in MENU}


def _same_bits(got, want):
    """float32 arrays equal bit for bit, NaN exactly where `want` has it."""
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- the unpack rule, exhaustively ----
PACKINGS = {
    "era5": dict(scale_factor=0.0017, add_offset=281.3, fill_value=-32767),
    "fill_min": dict(scale_factor=0.0017, add_offset=281.3, fill_value=-32768),
    "no_fill": dict(scale_factor=0.0017, add_offset=281.3),
    "scale_only_celsius": dict(scale_factor=0.01, fill_value=-32767),
}


@pytest.mark.parametrize("name", list(PACKINGS))
def test_unpack_every_int16_value(torch_cuda, name):
    kw = PACKINGS[name]
    q = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    q = np.concatenate([q, q[[0, 1, 40000]]])               # a length that is no multiple of the four elements a lane takes
    cube = af.PackedCube(torch_cuda.from_numpy(q).cuda(), **kw)
    pairs = [(kw.get("scale_factor"), kw.get("add_offset"))]
    if name == "scale_only_celsius":
        cube = cube - 273.15
        assert cube.pairs == [(np.float32(0.01), np.float32(-273.15))]
        pairs = [(0.01, -273.15)]
    want = pr.np_unpack(q, pairs, kw.get("fill_value"))
    assert np.isnan(want).sum() == (0 if "fill_value" not in kw else np.sum(q == kw["fill_value"]))
    _same_bits(cube.materialize().cpu().numpy(), want)
    # three pairs, and a view that starts inside a lane's eight bytes
    f = ((cube * 1.8) + 32)[3:]
    if isinstance(f, af.PackedCube):
        assert f.n_pairs == len(pairs) + 1
        _same_bits(f.materialize().cpu().numpy(), pr.np_unpack(q, pairs + [(1.8, 32)], kw.get("fill_value"))[3:])


# ---- every kernel of the packed menu ----
def _run_recipe(torch_cuda, r, q, pairs=pr.PAIRS, fill=pr.FILL):
    from aggfly_amd import hip
    cube = af.PackedCube(torch_cuda.from_numpy(q.reshape(r.T, 1, r.n_cells)).cuda(), scale_factor=pairs[0][0], add_offset=pairs[0][1], fill_value=fill)
    for m, a in pairs[1:]:
        cube = cube * m if m is not None else cube
        cube = cube + a if a is not None else cube
    assert isinstance(cube, af.PackedCube) and cube.n_pairs == len(pairs)
    plan = hip.FusedPlan(r.T, r.n_cells, hip.I16, r.inner_bounds, r.outer_bounds, r.columns, exact_order=r.exact_order)
    plan.bind_packing(cube.packing())
    values = pr.np_unpack(q, pairs, fill)
    want = _oracle_two_level(values.astype(np.float64).reshape(r.T, 1, r.n_cells), r.inner_bounds, r.outer_bounds, r.columns)
    return plan, plan.run_temporal(cube).cpu().numpy(), want, values


@pytest.mark.parametrize("name", [v.name for v in MENU])
def test_packed_variant_against_the_oracle(torch_cuda, name):
    v = BY_NAME[name]
    r = pr.recipe(v)
    q = pr.stored_cube_for(r, seed=zlib.crc32(name.encode()))
    plan, got, want, values = _run_recipe(torch_cuda, r, q)
    assert plan.describe().split()[0] == f"variant={name}", plan.describe()
    # the data meet the thresholds exactly, hold the extreme stored values, and a whole group of fills somewhere
    assert all((values == np.float32(e)).any() for e in r.edges) and {32767, -32768} <= set(np.unique(q).tolist())
    ib = r.inner_bounds
    assert any(np.isnan(values[ib[g]:ib[g + 1]]).all(axis=0).any() for g in range(len(ib) - 1) if ib[g + 1] > ib[g])
    _assert_cells(v, r.columns, got, want)


def test_the_cases_cover_the_loaded_builds_packed_menu(torch_cuda):
    from aggfly_amd import hip
    assert hip.build_info()["packed_variants"] == len(MENU) == len(BY_NAME)


# ---- cells per lane by row length ----
@pytest.mark.parametrize("n_cells,vec", [(1100, 4), (1101, 1), (1102, 2), (1103, 1)])
def test_row_length_decides_the_cells_per_lane(torch_cuda, n_cells, vec):
    """A light plan (mean and a degree-day column): four cells per lane on rows that are multiples of four, two on the other even
    rows, one on odd rows — and the same values whichever kernel reads them.  Three pairs (to Fahrenheit), no fill value."""
    pairs = [(0.0017, 281.3), (None, -273.15), (1.8, 32.0)]
    lens = vr._inner_lengths("", 0)
    ib = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    edge = float(pr.np_unpack([pr.stored_near(12.0)], pairs, None)[0])
    cols = [dict(inner="mean", outer="sum"), dict(inner="dd", inner_args=(edge, edge + 20.0, 0.0), outer="sum")]
    r = vr.Recipe("", pr.I16, int(ib[-1]), n_cells, ib, vr._outer_bounds(len(lens), 8), cols, True, 0)
    rng = np.random.default_rng(n_cells)
    q = rng.integers(-32768, 32768, (r.T, n_cells)).astype(np.int16)
    q[::7, ::5] = pr.stored_near(12.0)
    plan, got, want, _ = _run_recipe(torch_cuda, r, q, pairs, None)
    assert f"_v{vec}_" in plan.describe().split()[0] and plan.describe().startswith("variant=i16_p0_"), plan.describe()
    _assert_cells(vr.Variant("", pr.I16, 0, vec, 1, 1, 2, 0, 0), cols, got, want)


# ---- refusals ----
def test_the_library_refuses_what_it_cannot_read(torch_cuda):
    from aggfly_amd import hip
    T, C = 20, 300
    ib, ob = np.array([0, 8, 20]), np.array([0, 2])
    cols = [dict(inner="mean", outer="sum")]
    q = torch_cuda.zeros((T, 1, C), dtype=torch_cuda.int16, device="cuda")
    cube = af.PackedCube(q, 0.0017, 281.3, -32767)
    plan = hip.FusedPlan(T, C, hip.I16, ib, ob, cols)
    with pytest.raises(ValueError, match="bind_packing"):                 # an unbound packing
        plan.run_temporal(cube)
    with pytest.raises(ValueError, match="does not match the plan"):      # float values to a packed plan
        plan.run_temporal(torch_cuda.zeros((T, 1, C), dtype=torch_cuda.float32, device="cuda"))
    plan.bind_packing(cube.packing())
    assert plan.run_temporal(cube).shape == (1, 1, C)
    f32 = hip.FusedPlan(T, C, hip.F32, ib, ob, cols)
    with pytest.raises(ValueError, match="does not match the plan"):      # ... and the reverse
        f32.run_temporal(cube)
    with pytest.raises(ValueError, match="AFHIP_I16"):
        f32.bind_packing(cube.packing())
    with pytest.raises(TypeError):                                        # the bare integers are no cube
        plan.run_temporal(q)
    bad = cube.packing()
    bad.n_pairs = 4
    with pytest.raises(ValueError, match="n_pairs"):
        plan.bind_packing(bad)
    # the grouped reducers keep to float32 / float64
    lib, bounds = hip.load(), np.array([0, 8, 20], dtype=np.int64)
    out = torch_cuda.zeros((2, C), dtype=torch_cuda.float32, device="cuda")
    dd = np.array([10.0, 30.0, 0.0])
    assert lib.afhip_group_stat(q.data_ptr(), hip.I16, T, C, bounds.ctypes.data, 2, hip.MEAN, out.data_ptr(), None) == hip.E_INVALID
    for fn in (lib.afhip_group_dd, lib.afhip_group_bins, lib.afhip_group_sine_dd):
        assert fn(q.data_ptr(), hip.I16, T, C, bounds.ctypes.data, 2, dd.ctypes.data, 1, out.data_ptr(), None) == hip.E_INVALID
    with pytest.raises(TypeError):
        hip.group_stat(cube, bounds, "mean")


# ---- the public route ----
def _spec(outer):
    return dict(
        dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": outer})],
        tavg=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 4)}),
              ("aggregate", {"calc": "sum", "groupby": outer})],
        bins=[("aggregate", {"calc": "bins", "groupby": "date", "ddargs": [[0, 10, 0], [10, 20, 0]]}), ("aggregate", {"calc": "sum", "groupby": outer})],
    )


def _celsius(x):
    return x - 273.15


def _check_public_route(torch_cuda, path, var, T, ny, nx):
    from aggfly_amd import engine as eng
    host = af.dataset_from_path(path, var, preprocess=_celsius)
    plain = af.dataset_from_path(path, var, device="cuda", preprocess=_celsius)
    packed = af.dataset_from_path(path, var, device="cuda", keep_packed=True, preprocess=_celsius)
    assert packed.is_packed and not plain.is_packed and not host.is_packed
    q = packed.packed_cube().q
    assert q.dtype == torch_cuda.int16 and q.is_cuda and q.numel() * q.element_size() == T * ny * nx * 2
    assert packed.da.data.n_pairs == 2 and packed.da.dtype == torch_cuda.float32
    cube = packed.cube()
    assert cube.dtype == torch_cuda.float32 and cube.is_cuda
    _same_bits(cube.cpu().numpy(), plain.cube().cpu().numpy())
    np.testing.assert_array_equal(plain.cube().cpu().numpy(), host.cube())
    tab = synth.weights_table(ny, nx, 5, seed=3, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}), regionid="geoid")
    ods = ra.ODataset(host.cube().astype(np.float64), host.time, host.latitude, host.longitude, True)
    ow = ra.OWeights(tab, np.arange(ny * nx), gr.shp["geoid"], "geoid", "nan")
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
                for k in tp:
                    a, b = tp[k].cube().cpu().numpy(), tf[k].cube().cpu().numpy()
                    if exact:
                        np.testing.assert_array_equal(a, b)
                    else:
                        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)
    finally:
        eng.config.exact_order = old
    return packed, plain


LZ4 = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}


@pytest.mark.parametrize("comp,chunks", [(LZ4, (48, 8, 12)), (None, (48, 8, 12)), (LZ4, (100, 4, 5))], ids=["blosc_rows", "raw_rows", "blosc_tiles"])
def test_keep_packed_zarr_store_against_the_float32_route(torch_cuda, tmp_path, comp, chunks):
    from aggfly_amd import io as afio
    T, ny, nx = 24 * 40, 8, 12
    rng = np.random.default_rng(8)
    stored = rng.integers(-30000, 30000, (T, ny, nx)).astype(np.int16)
    stored[rng.random((T, ny, nx)) < 0.02] = -32767
    stored[:, 2, 3] = -32767                                            # an ocean cell
    attrs = {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}
    time = pd.date_range("2004-03-01", periods=T, freq="h")
    lat, lon = 35 + 0.25 * np.arange(ny), 250 + 0.25 * np.arange(nx)
    tv, tattrs = afio._encode_time(time)
    store = str(tmp_path / "p.zarr")
    os.makedirs(store)
    json.dump({"zarr_format": 2}, open(os.path.join(store, ".zgroup"), "w"))
    afio._write_array(store, "t2m", stored, ("time", "latitude", "longitude"), chunks, attrs, comp)
    afio._write_array(store, "time", np.asarray(tv, dtype=np.float64), ("time",), (T,), tattrs, None)
    afio._write_array(store, "latitude", lat, ("latitude",), (ny,), {}, None)
    afio._write_array(store, "longitude", lon, ("longitude",), (nx,), {}, None)
    os.remove(afio.ZarrArray(os.path.join(store, "t2m")).chunk_path((1, 0, 0)))       # an absent chunk = fill value
    packed, plain = _check_public_route(torch_cuda, store, "t2m", T, ny, nx)
    # what does not fold falls back to the values and continues as the float32 route does
    _same_bits(packed.power(2).cube().cpu().numpy(), plain.power(2).cube().cpu().numpy())
    other = plain.power(1)
    _same_bits(packed.interact(other).cube().cpu().numpy(), plain.interact(other).cube().cpu().numpy())
    assert not packed.power(2).is_packed and packed.is_packed


def test_keep_packed_netcdf4_variable_and_the_environment_switch(torch_cuda, monkeypatch):
    path = os.path.join(FIX, "nc4_like.nc")
    _check_public_route(torch_cuda, path, "t2m_packed", 37, 9, 14)
    assert not af.dataset_from_path(path, "t2m", device="cuda", keep_packed=True).is_packed         # float storage: nothing to keep
    monkeypatch.setenv("AGGFLY_HIP_KEEP_PACKED", "1")
    assert af.dataset_from_path(path, "t2m_packed", device="cuda").is_packed
    assert not af.dataset_from_path(path, "t2m_packed").is_packed                                   # no device: the host route
