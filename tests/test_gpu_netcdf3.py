"""NetCDF classic files on the device route: the byte-swapping placement kernel (`hip.place_box_swapped`) against numpy, and
`dataset_from_path(device="cuda")` on the catalogue of tests/netcdf3_cases.py against the arrays written — bit for bit, NaN
positions included —, with time / space windows, packed cubes, several files and the store routes."""
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netcdf3_cases as C  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import distributed as D, engine as eng, hip, io as afio, synth  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = C.build_cases()
BY = {c.name: c for c in CASES}
SENTINEL = {2: 0x5A5A, 4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("classic")
    return {c.name: c.write(d) for c in CASES}


@pytest.fixture
def no_host_route(monkeypatch):
    """The host route is not an answer here: a fall-back to scipy fails the test."""
    def refuse(path, var):
        raise AssertionError(f"{path}: the host route was taken")
    monkeypatch.setattr(afio, "_open_netcdf3", refuse)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype.newbyteorder("=") == b.dtype.newbyteorder("="), (a.shape, a.dtype, b.shape, b.dtype)
    a, b = np.ascontiguousarray(a.astype(a.dtype.newbyteorder("="))), np.ascontiguousarray(b.astype(b.dtype.newbyteorder("=")))
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


def _values(case):
    """What the file's variable means: `_cf_mask_scale` of the stored array under the attributes written."""
    return np.asarray(afio._cf_mask_scale(case.stored[case.var], case.attrs[case.var]))


# ---------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------
def _ints(rng, shape, es):
    return rng.integers(np.iinfo(f"i{es}").min, np.iinfo(f"i{es}").max, size=shape, dtype=f"i{es}", endpoint=True)


@pytest.mark.parametrize("es", [2, 4, 8])
def test_place_box_swapped_against_numpy(torch_cuda, es):
    torch = torch_cuda
    rng = np.random.default_rng(es)
    block = _ints(rng, (3, 5, 7), es)
    cube0 = np.full((4, 6, 9), SENTINEL[es], dtype=f"i{es}")
    cube = torch.from_numpy(cube0.copy()).cuda()
    hip.place_box_swapped(torch.from_numpy(block).cuda(), cube, (1, 1, 2, 2, 3, 4), (1, 2, 3))
    want = cube0.copy()
    want[1:3, 2:5, 3:7] = block.byteswap()[1:3, 1:4, 2:6]
    got = cube.cpu().numpy()
    np.testing.assert_array_equal(got, want)
    outside = np.ones(cube0.shape, bool)
    outside[1:3, 2:5, 3:7] = False
    assert (got[outside] == SENTINEL[es]).all() and (want[~outside] != SENTINEL[es]).any()
    # several workgroups, nx no multiple of 64: the (3, 33, 130) block placed whole
    wide = _ints(rng, (3, 33, 130), es)
    out = torch.from_numpy(np.full(wide.shape, SENTINEL[es], dtype=wide.dtype)).cuda()
    hip.place_box_swapped(torch.from_numpy(wide).cuda(), out, (0, 0, 0, 3, 33, 130), (0, 0, 0))
    np.testing.assert_array_equal(out.cpu().numpy(), wide.byteswap())


@pytest.mark.parametrize("box,at", [
    ((0, 0, 4, 1, 1, 4), (0, 0, 0)),      # beyond the block in x
    ((0, 3, 0, 1, 3, 1), (0, 0, 0)),      # ... in y
    ((2, 0, 0, 2, 1, 1), (0, 0, 0)),      # ... in t
    ((0, 0, 0, 1, 1, 4), (0, 0, 6)),      # beyond the cube in x
    ((0, 0, 0, 1, 3, 1), (0, 4, 0)),      # ... in y
    ((0, 0, 0, 2, 1, 1), (3, 0, 0)),      # ... in t
    ((0, 0, -1, 1, 1, 1), (0, 0, 0)),     # negative
    ((0, 0, 0, 1, 1, 1), (0, -1, 0)),
])
def test_place_box_swapped_refuses_a_box_outside(torch_cuda, box, at):
    torch = torch_cuda
    block = torch.from_numpy(_ints(np.random.default_rng(1), (3, 5, 7), 2)).cuda()
    cube = torch.full((4, 6, 9), SENTINEL[2], dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):
        hip.place_box_swapped(block, cube, box, at)
    torch.cuda.synchronize()
    assert bool((cube == SENTINEL[2]).all())                        # nothing was written
    with pytest.raises(ValueError):
        hip.place_box_swapped(block, cube.to(torch.int32), (0, 0, 0, 1, 1, 1), (0, 0, 0))      # one element size


# ---------------------------------------------------------------------------------------
# the route
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_streams_into_hbm(torch_cuda, case, files, no_host_route, monkeypatch):
    ds = af.dataset_from_path(files[case.name], case.var, device="cuda")
    cube = ds.cube()
    assert cube.is_cuda and not ds.is_packed
    want = _values(case)
    if want.dtype.kind in "iu":                                      # (every integer case of the catalogue carries a CF attribute)
        raise AssertionError("an integer case without CF attributes")
    _same_bits(cube.cpu().numpy(), want)
    assert np.isnan(want).any() == (("_FillValue" in case.attrs[case.var]) and want.size > 0)
    lat, lon = C._grid(*want.shape[1:])
    np.testing.assert_array_equal(ds.latitude, lat)
    np.testing.assert_array_equal(ds.longitude, lon)
    if "time" in case.stored:
        assert ds.time.equals(pd.DatetimeIndex(pd.Timestamp("1900-01-01") + pd.to_timedelta(case.stored["time"].astype(np.int64), unit="h")))
    try:
        import scipy.io  # noqa: F401
    except ImportError:
        return
    monkeypatch.undo()                                               # the host route, for comparison
    host = af.dataset_from_path(files[case.name], case.var)
    _same_bits(cube.cpu().numpy(), host.cube())


@pytest.mark.parametrize("name,keep", [("short_cdf1", False), ("short_cdf1", True), ("int_cdf2", False), ("double_cdf2", False), ("one_record_var", False)])
def test_both_staging_buffers_are_reused(torch_cuda, name, keep, files, no_host_route, monkeypatch):
    """Slabs of one or two steps: the 7 steps go through at least three slabs, so each page-locked buffer is filled again
    while the upload of the other is in flight."""
    case = BY[name]
    step = case.stored[case.var][0].nbytes
    monkeypatch.setenv("AGGFLY_HIP_SLAB_MB", repr(2.5 * step / (1 << 20)))
    calls = []
    real = hip.place_box_swapped
    monkeypatch.setattr(hip, "place_box_swapped", lambda blk, cube, box, at: calls.append(box[3]) or real(blk, cube, box, at))
    ds = af.dataset_from_path(files[name], case.var, device="cuda", keep_packed=keep)
    assert len(calls) >= 3 and sum(calls) == 7 and max(calls) <= 2, calls
    if keep:
        assert ds.is_packed
        _same_bits(ds.packed_cube().q.cpu().numpy(), case.stored[case.var])
    _same_bits(ds.cube().cpu().numpy(), _values(case))


def _regions():
    # half a cell (0.125 degrees) around rows 1..2 (49.75, 49.5) and columns 1..3 (230.25 .. 230.75) of the 3 x 5 grid
    return af.GeoRegions(pd.DataFrame({"geoid": ["a"], "minx": [-129.70], "miny": [49.55], "maxx": [-129.30], "maxy": [49.70]}))


TIME_WINDOWS = {"all": ({}, slice(0, 7)), "window": ({"time_window": (2, 5)}, slice(2, 5)), "none": ({"time_window": (0, 0)}, slice(0, 0)),
                "sel": ({"time_sel": slice("2000-01-01 01:00", "2000-01-01 04:00")}, slice(1, 5))}
SPACE_WINDOWS = {"grid": (lambda: {}, slice(0, 3), slice(0, 5)), "regions": (lambda: {"georegions": _regions()}, slice(1, 3), slice(1, 4)),
                 "band": (lambda: {"lat_window": (1, 3)}, slice(1, 3), slice(0, 5))}


@pytest.mark.parametrize("space", list(SPACE_WINDOWS))
@pytest.mark.parametrize("time", list(TIME_WINDOWS))
@pytest.mark.parametrize("name", ["short_cdf1", "short_cdf2_two", "fixed_time", "float_cdf1"])
def test_windows_read_the_same_box_as_the_host_cube(torch_cuda, name, time, space, files, no_host_route):
    case = BY[name]
    assert case.stored["time"][0] == 876576                          # 2000-01-01 00:00 in hours since 1900
    tkw, ts = TIME_WINDOWS[time]
    skw, ys, xs = SPACE_WINDOWS[space]
    ds = af.dataset_from_path(files[name], case.var, device="cuda", **tkw, **skw())
    cube = ds.cube()
    assert cube.is_cuda
    _same_bits(cube.cpu().numpy(), _values(case)[ts, ys, xs])
    lat, lon = C._grid(3, 5)
    np.testing.assert_array_equal(ds.latitude, lat[ys])
    np.testing.assert_array_equal(ds.longitude, lon[xs])
    assert len(ds.time) == ts.stop - ts.start


def test_the_wide_case_clipped_in_x(torch_cuda, files, no_host_route):
    """The x clip is the kernel's: the rows of the box are read whole, columns 40..89 of 130 reach the cube."""
    case = BY["short_wide"]
    lat, lon = C._grid(33, 130)
    gr = af.GeoRegions(pd.DataFrame({"geoid": ["a"], "minx": [float(lon[40]) - 360], "miny": [float(lat[20])], "maxx": [float(lon[89]) - 360],
                                     "maxy": [float(lat[4])]}))
    ds = af.dataset_from_path(files["short_wide"], "t2m", device="cuda", georegions=gr)
    _same_bits(ds.cube().cpu().numpy(), _values(case)[:, 4:21, 40:90])


# ---------------------------------------------------------------------------------------
# packed cubes
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in CASES if c.stored[c.var].dtype == np.int16])
def test_short_cases_stay_packed(torch_cuda, name, files, no_host_route):
    case = BY[name]
    packed = af.dataset_from_path(files[name], case.var, device="cuda", keep_packed=True)
    plain = af.dataset_from_path(files[name], case.var, device="cuda")
    assert packed.is_packed and not plain.is_packed
    q = packed.packed_cube().q
    assert q.is_cuda and q.dtype == torch_cuda.int16
    _same_bits(q.cpu().numpy(), case.stored[case.var])
    _same_bits(packed.cube().cpu().numpy(), plain.cube().cpu().numpy())
    for nm in [c.name for c in CASES if c.stored[c.var].dtype != np.int16][:1]:
        other = af.dataset_from_path(files[nm], BY[nm].var, device="cuda", keep_packed=True)
        assert not other.is_packed                                   # other storage: nothing to keep packed


NY2, NX2 = 6, 8


def _pair(tmp_path, second="short"):
    """Two files of 24 hourly steps, 2000-01-01 and -02, each with its own scale_factor / add_offset (the second, on request, float32)."""
    rng = np.random.default_rng(77)
    out = []
    for i, at in enumerate([{"scale_factor": 0.0011, "add_offset": 280.5, "_FillValue": np.int16(-32767)},
                            {"scale_factor": 0.0016, "add_offset": 268.25, "_FillValue": np.int16(-32767)}]):
        if i == 1 and second == "float":
            data, at = rng.normal(275, 8, size=(24, NY2, NX2)).astype(np.float32), {}
        else:
            data = C._ints(rng, (24, NY2, NX2), np.int16, -32767, n_fill=6)
            data[:, 2, 3] = -32767                                   # an ocean cell
        c = C._case(f"pair{i}_{second}", 2 - i, data, at, "t2m", T=24, ny=NY2, nx=NX2, start_hour=876576 + 24 * i)
        out.append((c, c.write(tmp_path)))
    return out


def test_two_files_of_different_packings_stay_packed(torch_cuda, tmp_path, no_host_route):
    pair = _pair(tmp_path)
    paths = [p for _, p in pair]
    pre = lambda x: x - 273.15
    packed = af.dataset_from_path(paths, "t2m", device="cuda", keep_packed=True, preprocess=pre)
    plain = af.dataset_from_path(paths, "t2m", device="cuda", preprocess=pre)
    assert packed.is_packed and not plain.is_packed
    data = packed.da.data
    assert data.n_rules == 2 and data.rule_bounds == [0, 24, 48] and len(packed.time) == 48
    _same_bits(packed.packed_cube().q.cpu().numpy(), np.concatenate([c.stored["t2m"] for c, _ in pair]))
    want = np.concatenate([_values(c) for c, _ in pair]) - np.float32(273.15)
    _same_bits(plain.cube().cpu().numpy(), want)
    _same_bits(packed.cube().cpu().numpy(), plain.cube().cpu().numpy())
    # a glob gives the same dataset
    globbed = af.dataset_from_path(os.path.join(str(tmp_path), "pair*_short.nc"), "t2m", device="cuda", keep_packed=True, preprocess=pre)
    assert globbed.is_packed and globbed.da.data.rule_bounds == [0, 24, 48]
    tab = synth.weights_table(NY2, NX2, 4, seed=3, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}), regionid="geoid")
    spec = dict(tavg=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 3)}),
                      ("aggregate", {"calc": "sum", "groupby": "year"})])
    old = eng.config.exact_order
    try:
        eng.config.exact_order = True
        got_p = af.aggregate_dataset(dataset=packed, weights=af.weights_from_objects(packed, gr, table=tab), **spec)
        got_f = af.aggregate_dataset(dataset=plain, weights=af.weights_from_objects(plain, gr, table=tab), **spec)
    finally:
        eng.config.exact_order = old
    cols = [c for c in got_f.columns if c not in ("geoid", "time")]
    assert list(got_p.columns) == list(got_f.columns) and len(got_p) == len(got_f) > 0 and len(cols) == 2
    np.testing.assert_array_equal(got_p[cols].values, got_f[cols].values)
    assert np.isfinite(got_f[cols].values).any()


def test_a_short_file_beside_a_float_file_takes_the_float32_route(torch_cuda, tmp_path, no_host_route):
    pair = _pair(tmp_path, second="float")
    ds = af.dataset_from_path([p for _, p in pair], "t2m", device="cuda", keep_packed=True)
    assert not ds.is_packed and ds.cube().is_cuda and ds.cube().dtype == torch_cuda.float32
    _same_bits(ds.cube().cpu().numpy(), np.concatenate([_values(c) for c, _ in pair]))


# ---------------------------------------------------------------------------------------
# the store routes
# ---------------------------------------------------------------------------------------
def test_store_sharded_streams_a_classic_file_in_windows(torch_cuda, tmp_path, no_host_route, monkeypatch):
    """`aggregate_store_sharded` on one classic file (January 30th to February 4th, monthly output) under a budget of two days
    per window: each month is a window that streams its own steps
    from the file, and the frame equals `aggregate_dataset` on the whole dataset exactly (the comparison of
    tests/test_gpu_sharded.py::test_store_sharded_streams_each_ranks_window, table-order sums)."""
    T, ny, nx = 24 * 6, 10, 12
    cube = synth.temperature_cube(T, ny, nx, dtype=np.float32, seed=61, ocean_frac=0.1, scattered_nan=30) + np.float32(273.15)
    stored = np.where(np.isnan(cube), -32767, np.round((cube - 280.0) / 0.002)).astype(np.int16)
    case = C._case("era", 2, stored, {"scale_factor": 0.002, "add_offset": 280.0, "_FillValue": np.int16(-32767)}, "t2m", T=T, ny=ny, nx=nx,
                   start_hour=876576 + 29 * 24)
    path = case.write(tmp_path)
    tab = synth.weights_table(ny, nx, 6, seed=62, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}))
    spec = dict(dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": "month"})],
                t=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 3)}),
                   ("aggregate", {"calc": "sum", "groupby": "month"})])
    weights_of = lambda ds: af.weights_from_objects(ds, gr, table=tab)
    pre = lambda x: x - 273.15
    opened = []
    real_open = afio.dataset_from_path
    monkeypatch.setattr(afio, "dataset_from_path", lambda *a, **k: opened.append(k.get("time_window")) or real_open(*a, **k))
    old = eng.config.exact_order
    try:
        eng.config.exact_order = True
        for keep in (False, True):
            opened.clear()
            got = D.aggregate_store_sharded(weights_of, path, "t2m", spec, lon_is_360=True, preprocess=pre, keep_packed=keep,
                                            max_window_bytes=2 * 24 * ny * nx * (2 if keep else 4))
            assert len(opened) >= 2 and opened[0][0] == 0 and opened[-1][1] == T, opened
            assert all(a[1] == b[0] for a, b in zip(opened, opened[1:])), opened
            whole = real_open(path, "t2m", lon_is_360=True, preprocess=pre, device="cuda", keep_packed=keep)
            assert whole.is_packed == keep
            want = af.aggregate_dataset(dataset=whole, weights=weights_of(whole), aggregator_dict=spec)
            assert len(got) == len(want) > 0
            pd.testing.assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True), check_exact=True)
    finally:
        eng.config.exact_order = old
