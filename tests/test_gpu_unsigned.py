"""uint16-packed cubes on the GPU (AFHIP_U16): the unpack rule over every stored value, the temporal kernel at each row piece against
the oracle, what the library refuses, and the public routes (host, device, `keep_packed`) on uint16 stores and on int16 stores
under ``_Unsigned = "true"``.

A U16 plan runs the kernels of the int16-packed menu with the signedness in the unpack record, so the oracle and the bars are those
of test_gpu_packed.py: `cport` on the cube unpacked in numpy float32 one rounded operation at a time, bit-exact statistics / dd /
bins under exact_order, 4e-16 for integer powers, 1e-12 for the device pow(), 1e-10 for sine_dd (`_assert_cells`).  The stored
values span 0...65535 with thresholds among the values of the upper half: a kernel that reads the bits as signed changes every column.
"""
import json
import os

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import synth
from oracle import ref_aggregate as ra

import packed_recipes as pr
import variant_recipes as vr
from test_gpu_packed import LZ4, _celsius, _same_bits, _spec
from test_gpu_variant_menu import _assert_cells, _oracle_two_level

pytestmark = pytest.mark.gpu

U16 = 3                                           # include/aggfly_hip.h: AFHIP_U16
# value(q) = q * 0.001 + 252.4 - 273.15: -20.75 C at 0, 12.02 C at 32768, 44.79 C at 65535 — strictly increasing in float32 (the step
# is 30 ulp of the sum), so the recipes' thresholds (-12 ... 40 C) fall on both halves of the stored range
PAIRS = [(0.001, 252.4), (None, -273.15)]
FILL = 32767


def np_unpack(q, pairs=PAIRS, fill=FILL):
    """The unpack rule of uint16 storage in numpy float32, one rounded operation at a time; NaN at the fill."""
    q = np.asarray(q, dtype=np.uint16)
    f = q.astype(np.float32)
    for m, a in pairs:
        if m is not None:
            f = f * np.float32(m)
        if a is not None:
            f = f + np.float32(a)
    if fill is not None:
        f = np.where(q == np.uint16(fill), np.float32(np.nan), f)
    return f


def stored_near(value, pairs=PAIRS):
    """The stored integer whose value is the largest not above `value` (the rule is monotone: bisection over uint16)."""
    lo, hi = 1, 65534
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if float(np_unpack([mid], pairs, None)[0]) <= value:
            lo = mid
        else:
            hi = mid
    return lo if lo != FILL else lo + 1


def _snap(e):
    return float(np_unpack([stored_near(e)], PAIRS, None)[0])


def _snap_columns(cols):
    """`packed_recipes._snap_columns` on the unsigned cube's values."""
    out = []
    for c in cols:
        c = dict(c)
        for key in ("inner_args", "outer_args"):
            if key in c:
                c[key] = (_snap(c[key][0]), _snap(c[key][1]), c[key][2])
        if c.get("transform") == "hinge":
            c["transform_arg"] = _snap(c["transform_arg"])
        out.append(c)
    return out


def _edges(cols):
    e = set()
    for c in cols:
        if c["inner"] in ("dd", "bins"):
            e.update(c["inner_args"][:2])
        if c.get("transform") == "hinge":
            e.add(c["transform_arg"])
    return sorted(e)


def _cuda_cube(torch_cuda, q, **kw):
    """uint16 numpy -> PackedCube in HBM (through the int16 of the same bits: what the loaders hand over)."""
    cube = af.PackedCube(torch_cuda.from_numpy(np.ascontiguousarray(q).view(np.int16)).cuda(), unsigned=True, **kw)
    assert cube.unsigned and cube.q.dtype == torch_cuda.int16
    return cube


# ---- 1. the rule, exhaustively ----
PACKINGS = {
    "gridmet": dict(scale_factor=0.1, add_offset=220.0, fill_value=32767),
    "fill_max": dict(scale_factor=0.1, add_offset=220.0, fill_value=65535),
    "fill_zero": dict(scale_factor=0.1, add_offset=220.0, fill_value=0),
    "no_fill": dict(scale_factor=0.1, add_offset=220.0),
}


@pytest.mark.parametrize("name", list(PACKINGS))
def test_unpack_every_uint16_value(torch_cuda, name):
    kw = PACKINGS[name]
    q = np.arange(0, 65536, dtype=np.int64).astype(np.uint16)
    q = np.concatenate([q, q[[0, 32768, 65535]]])           # a length that is no multiple of the four elements a lane takes
    cube = _cuda_cube(torch_cuda, q, **kw)
    pairs = [(kw["scale_factor"], kw["add_offset"])]
    fill = kw.get("fill_value")
    want = np_unpack(q, pairs, fill)
    assert np.isnan(want).sum() == (0 if fill is None else np.sum(q == fill)) and np.nanmax(want) > 6773.0          # 65534 or 65535 read as unsigned
    _same_bits(cube.materialize().cpu().numpy(), want)
    # three pairs, and a view that starts inside a lane's eight bytes
    f = ((cube * 1.8) + 32)[3:]
    assert isinstance(f, af.PackedCube) and f.unsigned and f.n_pairs == 2
    _same_bits(f.materialize().cpu().numpy(), np_unpack(q, pairs + [(1.8, 32)], fill)[3:])
    g = ((cube - 273.15) * 1.8 + 32)[3:]
    assert isinstance(g, af.PackedCube) and g.n_pairs == 3
    _same_bits(g.materialize().cpu().numpy(), np_unpack(q, pairs + [(None, -273.15), (1.8, 32)], fill)[3:])


# ---- 2. the temporal kernel at each row piece ----
def _bounds():
    lens = vr._inner_lengths("", 0)
    ib = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return ib, vr._outer_bounds(len(lens), 8)


def _stored_cube(T, C, ib, edges, seed, hi=65536):
    """uint16 [T, C] uniform over 0 ... hi - 1: the extreme and the middle values planted, every edge with its two neighbours, the
    fill in first rows of groups, whole groups and ocean cells (the last cell included)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, hi, (T, C)).astype(np.uint16)
    flat = q.reshape(-1)
    plant = [0, 32766, 32768, 65535, 1, 65534] if hi == 65536 else [0, 32766, 1, hi - 1]
    for e in edges:
        s = stored_near(e)
        plant += [s, s, s + 1, s - 1]
    plant = np.array([p for p in plant if p != FILL and p < hi] * 20, dtype=np.uint16)
    flat[rng.choice(flat.size, plant.size, replace=False)] = plant
    ne = np.flatnonzero(np.diff(ib) > 0)
    for g in ne[::5]:
        q[ib[g], rng.choice(C, 25, replace=False)] = FILL
    for g in ne[2::7]:
        q[ib[g]:ib[g + 1], rng.choice(C, 4, replace=False)] = FILL
    q[:, [3, C // 2, C - 1]] = FILL
    return q


def _run(torch_cuda, q, ib, ob, cols, code=U16):
    from aggfly_amd import hip
    T, C = q.shape
    cube = _cuda_cube(torch_cuda, q.reshape(T, 1, C), scale_factor=PAIRS[0][0], add_offset=PAIRS[0][1], fill_value=FILL) - 273.15
    if code != U16:
        cube = af.PackedCube(cube.q, fill_value=FILL, unsigned=False, _pairs=cube.pairs)
    assert isinstance(cube, af.PackedCube) and cube.n_pairs == 2 and hip._dtype_code(cube) == code
    plan = hip.FusedPlan(T, C, code, ib, ob, cols, exact_order=True)
    plan.bind_packing(cube)
    return plan, plan.run_temporal(cube).cpu().numpy()


def _check_against_oracle(torch_cuda, n_cells, cols, vec, tiers, seed):
    ib, ob = _bounds()
    T = int(ib[-1])
    edges = _edges(cols)
    q = _stored_cube(T, n_cells, ib, edges, seed)
    values = np_unpack(q)
    # a kernel that reads the bits as signed changes every column: a quarter of every row (and far more) is stored from 32768 up,
    # and thresholds lie among the values of that half
    assert ((q >= 32768).mean(axis=1) >= 0.25).all()
    upper = float(np_unpack([32768], PAIRS, None)[0])
    assert any(e > upper for e in edges) and all((values == np.float32(e)).any() for e in edges)
    assert {0, 32766, 32767, 32768, 65535} <= set(np.unique(q).tolist()) and np.isnan(values[:, -1]).all()
    assert any(np.isnan(values[ib[g]:ib[g + 1]]).all(axis=0).any() for g in range(len(ib) - 1) if ib[g + 1] > ib[g])
    plan, got = _run(torch_cuda, q, ib, ob, cols)
    name = plan.describe().split()[0]
    assert name.startswith("variant=i16_p0_") and f"_v{vec}_" in name and tiers in name, plan.describe()
    assert "storage=uint16" in plan.describe()
    want = _oracle_two_level(values.astype(np.float64).reshape(T, 1, n_cells), ib, ob, cols)
    stat, nthr, kmax = (int(t[1:]) for t in tiers.strip("_").split("_"))
    _assert_cells(vr.Variant(name, pr.I16, 0, vec, stat, nthr, kmax, 0, 0), cols, got, want)
    return plan


@pytest.mark.parametrize("n_cells,vec", [(1100, 4), (1102, 2), (1101, 1)])
def test_light_plan_at_each_row_piece(torch_cuda, n_cells, vec):
    """Mean and one degree-day column: four, two and one cell per lane by the row length, as for int16 storage."""
    from aggfly_amd import hip
    cols = _snap_columns([dict(inner="mean", outer="sum"), dict(inner="dd", inner_args=(14.0, 34.0, 0.0), outer="sum")])
    plan = _check_against_oracle(torch_cuda, n_cells, cols, vec, "_s1_t1_k2_", seed=n_cells)
    ib, ob = _bounds()
    signed_plan = hip.FusedPlan(int(ib[-1]), n_cells, hip.I16, ib, ob, cols, exact_order=True)
    assert signed_plan.describe().split()[0] == plan.describe().split()[0]           # the planner treats the two storages alike
    assert "storage=int16" in signed_plan.describe()


def _heavy_vec(n_cells):
    """Cells per lane of the stat-3, sixteen-slot, sixteen-column kernel the loaded menu holds for a row length (the widest that
    divides it: the packed menu leaves the two-cell form of this shape out, so even rows take one cell per lane too)."""
    from aggfly_amd import hip
    menu = [vr.variant(v) for v in vr.menu_of("packed", hip.build_info()["menu"])]
    return max(v.vec for v in menu if (v.stat, v.nthr, v.kmax) == (3, 16, 16) and n_cells % v.vec == 0)


@pytest.mark.parametrize("n_cells", [1102, 1101])
def test_heavy_plan_on_even_and_odd_rows(torch_cuda, n_cells):
    """Statistic tier 3 with sixteen threshold slots and sixteen columns: the recipe of i16_p0_v1_s3_t16_k16, its thresholds moved
    onto values of the unsigned cube."""
    v = vr.Variant("i16_p0_v1_s3_t16_k16", pr.I16, 0, 1, 3, 16, 16, 8, vr.NT)
    nslots, K = vr._shape(v)
    assert (nslots, K) == (16, 16)
    cols = _snap_columns(vr._columns(v, nslots, K, False))
    assert len({c["inner_args"] for c in cols}) == 16
    _check_against_oracle(torch_cuda, n_cells, cols, _heavy_vec(n_cells), "_s3_t16_k16_", seed=7 * n_cells)


@pytest.mark.parametrize("n_cells", [1100, 1102, 1101])
def test_lower_half_values_read_alike_as_uint16_and_int16(torch_cuda, n_cells):
    """Stored values below 32768 are the same integers under both storages: the same bits run as U16 and as I16 give bit-identical
    cells."""
    ib, ob = _bounds()
    cols = _snap_columns([dict(inner="mean", outer="sum"), dict(inner="dd", inner_args=(-6.0, 4.0, 0.0), outer="sum"),
                          dict(inner="max", outer="mean"), dict(inner="bins", inner_args=(0.0, 9.0, 0.0), outer="sum")])
    q = _stored_cube(int(ib[-1]), n_cells, ib, _edges(cols), seed=n_cells, hi=32768)
    assert q.max() == 32767 and (q == FILL).any()
    pu, got_u = _run(torch_cuda, q, ib, ob, cols, U16)
    from aggfly_amd import hip
    ps, got_s = _run(torch_cuda, q, ib, ob, cols, hip.I16)
    assert pu.describe().split()[0] == ps.describe().split()[0]
    assert np.array_equal(np.isnan(got_u), np.isnan(got_s)) and np.isnan(got_u).any() and not np.isnan(got_u).all()
    np.testing.assert_array_equal(got_u.view(np.uint64), got_s.view(np.uint64))


# ---- 3. refusals ----
def test_the_library_refuses_what_it_cannot_read(torch_cuda):
    from aggfly_amd import hip
    assert hip.U16 == U16
    T, C = 20, 300
    ib, ob = np.array([0, 8, 20]), np.array([0, 2])
    cols = [dict(inner="mean", outer="sum")]
    q = torch_cuda.zeros((T, 1, C), dtype=torch_cuda.int16, device="cuda")
    ucube = af.PackedCube(q, 0.1, 220.0, 32767, unsigned=True)
    scube = af.PackedCube(q, 0.1, 220.0, 32767)
    plan = hip.FusedPlan(T, C, hip.U16, ib, ob, cols)
    with pytest.raises(ValueError, match="bind_packing"):                 # an unbound U16 plan
        plan.run_temporal(ucube)
    with pytest.raises(ValueError, match="does not match the plan"):      # an int16 cube's rule, and the cube itself, on a U16 plan
        plan.bind_packing(scube)
    plan.bind_packing(ucube)
    with pytest.raises(ValueError, match="does not match the plan"):
        plan.run_temporal(scube)
    assert plan.run_temporal(ucube).shape == (1, 1, C)
    splan = hip.FusedPlan(T, C, hip.I16, ib, ob, cols)                    # ... and the reverse
    with pytest.raises(ValueError, match="does not match the plan"):
        splan.bind_packing(ucube)
    splan.bind_packing(scube)
    with pytest.raises(ValueError, match="does not match the plan"):
        splan.run_temporal(ucube)
    # a fill outside the storage's range: 40000 is a uint16 and no int16, -1 is neither's on a U16 plan
    p = ucube.packing()
    p.fill = 40000
    plan.bind_packing(p)
    with pytest.raises(ValueError, match="no int16"):
        splan.bind_packing(p)
    for bad in (-1, 65536):
        p.fill = bad
        with pytest.raises(ValueError, match="no uint16"):
            plan.bind_packing(p)
    out = torch_cuda.zeros(8, dtype=torch_cuda.float32, device="cuda")
    lib = hip.load()
    import ctypes
    assert lib.afhip_unpack_u16(q.data_ptr(), 8, ctypes.byref(p), out.data_ptr(), None) == hip.E_INVALID
    p.fill = -1
    assert lib.afhip_unpack_i16(q.data_ptr(), 8, ctypes.byref(p), out.data_ptr(), None) == 0
    # the signedness is the library's: whatever the caller writes into `pad` is not read
    p = ucube.packing()
    p.pad = 1
    splan.bind_packing(p)
    neg = torch_cuda.full((T, 1, C), -2, dtype=torch_cuda.int16, device="cuda")
    got = splan.run_temporal(af.PackedCube(neg, 0.1, 220.0, 32767)).cpu().numpy()
    assert np.all(got == 2 * float(np.float32(-2) * np.float32(0.1) + np.float32(220.0)))
    # float plans still say which dtype takes a packing
    f32 = hip.FusedPlan(T, C, hip.F32, ib, ob, cols)
    with pytest.raises(ValueError, match="AFHIP_I16"):
        f32.bind_packing(ucube.packing())
    # the grouped reducers keep to float32 / float64
    bounds = np.array([0, 8, 20], dtype=np.int64)
    out = torch_cuda.zeros((2, C), dtype=torch_cuda.float32, device="cuda")
    dd = np.array([10.0, 30.0, 0.0])
    assert lib.afhip_group_stat(q.data_ptr(), hip.U16, T, C, bounds.ctypes.data, 2, hip.MEAN, out.data_ptr(), None) == hip.E_INVALID
    for fn in (lib.afhip_group_dd, lib.afhip_group_bins, lib.afhip_group_sine_dd):
        assert fn(q.data_ptr(), hip.U16, T, C, bounds.ctypes.data, 2, dd.ctypes.data, 1, out.data_ptr(), None) == hip.E_INVALID
    with pytest.raises(TypeError):
        hip.group_stat(ucube, bounds, "mean")


# ---- 4. the public route ----
T_PUB, NY, NX = 24 * 40, 8, 12


def _stored_public(fill):
    rng = np.random.default_rng(8)
    stored = rng.integers(0, 65536, (T_PUB, NY, NX)).astype(np.uint16)
    stored[stored == fill] = fill ^ 1
    stored.reshape(-1)[:4] = [0, 32768, 65535 if fill != 65535 else 65534, 32766]
    stored[rng.random((T_PUB, NY, NX)) < 0.02] = fill
    stored[:, 2, 3] = fill                                              # an ocean cell
    return stored


def _write_store(tmp_path, name, stored, attrs, comp, chunks):
    from aggfly_amd import io as afio
    time = pd.date_range("2004-03-01", periods=T_PUB, freq="h")
    lat, lon = 35 + 0.25 * np.arange(NY), 250 + 0.25 * np.arange(NX)
    tv, tattrs = afio._encode_time(time)
    store = str(tmp_path / name)
    os.makedirs(store)
    json.dump({"zarr_format": 2}, open(os.path.join(store, ".zgroup"), "w"))
    afio._write_array(store, "tmmx", stored, ("time", "latitude", "longitude"), chunks, attrs, comp)
    afio._write_array(store, "time", np.asarray(tv, dtype=np.float64), ("time",), (T_PUB,), tattrs, None)
    afio._write_array(store, "latitude", lat, ("latitude",), (NY,), {}, None)
    afio._write_array(store, "longitude", lon, ("longitude",), (NX,), {}, None)
    os.remove(afio.ZarrArray(os.path.join(store, "tmmx")).chunk_path((1, 0, 0)))      # an absent chunk = the array's fill value (0)
    return store


def _as_read(stored, chunks):
    """The stored integers a reader sees: zeros where the chunk file (1, 0, 0) was removed."""
    tc, yc, xc = chunks
    seen = stored.copy()
    seen[tc:2 * tc, :yc, :xc] = 0
    return seen


def _celsius_chain(seen, scale, offset, fill):
    """float32, one rounded operation at a time, as the host route and `_celsius` compute it; NaN at the fill."""
    f = seen.astype(np.float32) * np.float32(scale)
    f = f + np.float32(offset)
    f = f - np.float32(273.15)
    return np.where(seen == fill, np.float32(np.nan), f)


def _three_routes(torch_cuda, store):
    host = af.dataset_from_path(store, "tmmx", preprocess=_celsius)
    plain = af.dataset_from_path(store, "tmmx", device="cuda", preprocess=_celsius)
    packed = af.dataset_from_path(store, "tmmx", device="cuda", keep_packed=True, preprocess=_celsius)
    assert packed.is_packed and not plain.is_packed and not host.is_packed
    pc = packed.packed_cube()
    assert pc.unsigned and pc.q.dtype == torch_cuda.int16 and pc.q.is_cuda and pc.q.numel() * pc.q.element_size() == T_PUB * NY * NX * 2
    assert packed.da.data.n_pairs == 2 and packed.da.dtype == torch_cuda.float32
    assert plain.cube().dtype == torch_cuda.float32
    h = np.asarray(host.cube())
    _same_bits(plain.cube().cpu().numpy(), h)
    _same_bits(packed.cube().cpu().numpy(), h)
    return host, plain, packed


def _check_aggregates(host, plain, packed):
    from aggfly_amd import engine as eng
    tab = synth.weights_table(NY, NX, 5, seed=3, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}), regionid="geoid")
    ods = ra.ODataset(np.asarray(host.cube()).astype(np.float64), host.time, host.latitude, host.longitude, True)
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
                for k in tp:
                    a, b = tp[k].cube().cpu().numpy(), tf[k].cube().cpu().numpy()
                    if exact:
                        np.testing.assert_array_equal(a, b)
                    else:
                        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, equal_nan=True)
    finally:
        eng.config.exact_order = old


# stored 0...65535 at scale 0.001 from 252.4 K: -20.75 ... 44.79 C, so `_spec`'s thresholds (0, 10, 20, 30 C) fall on both halves
ATTRS = {"scale_factor": 0.001, "add_offset": 252.4, "_FillValue": 32767}
LAYOUTS = [(LZ4, (48, 8, 12)), (None, (48, 8, 12)), (LZ4, (100, 4, 5))]
LAYOUT_IDS = ["blosc_rows", "raw_rows", "blosc_tiles"]


@pytest.mark.parametrize("comp,chunks", LAYOUTS, ids=LAYOUT_IDS)
def test_uint16_zarr_store_on_the_three_routes(torch_cuda, tmp_path, comp, chunks):
    store = _write_store(tmp_path, "u.zarr", _stored_public(32767), ATTRS, comp, chunks)
    host, plain, packed = _three_routes(torch_cuda, store)
    seen = _as_read(_stored_public(32767), chunks)
    h = np.asarray(host.cube())
    _same_bits(h, _celsius_chain(seen, 0.001, 252.4, 32767))                                # the host route is the float32 chain on the unsigned integers
    assert (h[~np.isnan(h)] > 12.1).mean() > 0.25 and np.isnan(h[-1, 2, 3]) and np.isnan(h).sum() == (seen == 32767).sum()
    _check_aggregates(host, plain, packed)
    # what does not fold falls back to the values and continues as the float32 route does
    _same_bits(packed.power(2).cube().cpu().numpy(), plain.power(2).cube().cpu().numpy())
    assert not packed.power(2).is_packed and packed.is_packed


def test_uint16_blosc_store_decoded_in_hbm(torch_cuda, tmp_path, monkeypatch):
    """Once more with the chunks crossing PCIe compressed (the opt-in switch test_gpu_decode.py forces the route with)."""
    store = _write_store(tmp_path, "u.zarr", _stored_public(32767), ATTRS, LZ4, (48, 8, 12))
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "1")
    host, plain, packed = _three_routes(torch_cuda, store)
    _check_aggregates(host, plain, packed)


@pytest.mark.parametrize("comp,chunks", LAYOUTS, ids=LAYOUT_IDS)
def test_int16_store_under_the_unsigned_attribute_reads_as_the_uint16_store(torch_cuda, tmp_path, comp, chunks):
    stored = _stored_public(65535)
    attrs = {"scale_factor": 0.001, "add_offset": 252.4}
    u = _write_store(tmp_path, "u.zarr", stored, dict(attrs, _FillValue=65535), comp, chunks)
    s = _write_store(tmp_path, "s.zarr", stored.view(np.int16), dict(attrs, _FillValue=-1, _Unsigned="true"), comp, chunks)
    routes_u, routes_s = _three_routes(torch_cuda, u), _three_routes(torch_cuda, s)
    _same_bits(np.asarray(routes_u[0].cube()), _celsius_chain(_as_read(stored, chunks), 0.001, 252.4, 65535))
    assert np.isnan(np.asarray(routes_u[0].cube())).sum() > T_PUB // 2
    for a, b in zip(routes_u, routes_s):
        ca, cb = a.cube(), b.cube()
        _same_bits(np.asarray(ca.cpu() if hasattr(ca, "cpu") else ca), np.asarray(cb.cpu() if hasattr(cb, "cpu") else cb))
    assert routes_s[2].packed_cube().fill_value == 65535 == routes_u[2].packed_cube().fill_value
    assert torch_cuda.equal(routes_s[2].packed_cube().q, routes_u[2].packed_cube().q)


def test_the_environment_switch_keeps_uint16_packed(torch_cuda, tmp_path, monkeypatch):
    store = _write_store(tmp_path, "u.zarr", _stored_public(32767), ATTRS, None, (48, 8, 12))
    monkeypatch.setenv("AGGFLY_HIP_KEEP_PACKED", "1")
    ds = af.dataset_from_path(store, "tmmx", device="cuda")
    assert ds.is_packed and ds.packed_cube().unsigned
    assert not af.dataset_from_path(store, "tmmx").is_packed                                        # no device: the host route
