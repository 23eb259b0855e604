"""The host side every store-to-HBM route shares (`io._StreamedSource`): the request resolver and the coordinate cut, the one probe
(`io._streamed_source`) on a fixture of each container, what the probe declines, and the time concatenation of multi-file datasets.
No GPU: nothing is streamed here."""
import os

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import distributed as D, io as afio
from aggfly_amd.cfcalendar import CFTimeIndex, decode_cf_time

import grib_cases as G
import netcdf3_cases as N

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdf5")
XY = ("longitude", "latitude")

# ---------------------------------------------------------------------------------------
# the resolver: 7 daily steps on a 6 x 9 grid of 1 degree, latitudes 40..45, longitudes 230..238
# ---------------------------------------------------------------------------------------
TIME = pd.date_range("2001-01-01", periods=7, freq="D")
LAT, LON = 40.0 + np.arange(6), 230.0 + np.arange(9)


def _regions(minx, miny, maxx, maxy):
    return af.GeoRegions(pd.DataFrame({"geoid": ["a", "b"], "minx": [minx, minx + 1.0], "miny": [miny, miny], "maxx": [maxx - 1.0, maxx],
                                       "maxy": [maxy, maxy]}))


# centroids within half a cell (0.5) of the extent: longitudes 231.8 - 0.5 .. 235.1 + 0.5 -> 232..235, cells 2..5; latitudes
# 41.2 - 0.5 .. 43.9 + 0.5 -> 41..44, rows 1..4
CLIP = _regions(-128.2, 41.2, -124.9, 43.9)

# (request, window, latitude rows, longitude cells) — None: all of the axis
CASES = [
    ({}, None, None, None),
    ({"time_window": (2, 5)}, (2, 5), None, None),
    ({"time_window": (0, 0)}, (0, 0), None, None),
    ({"time_sel": slice("2001-01-03", "2001-01-05")}, (2, 5), None, None),
    ({"time_sel": "2001-01-04"}, (3, 4), None, None),
    ({"time_sel": slice("2001-01-03", "2001-01-05"), "time_window": (1, 7)}, (1, 7), None, None),      # the window wins
    ({"georegions": CLIP}, None, (1, 5), (2, 6)),
    ({"georegions": CLIP, "lat_window": (1, 3)}, None, (2, 4), (2, 6)),                               # rows 1..2 of the clip's four
    ({"lat_window": (1, 3)}, None, (1, 3), (0, 9)),
    ({"georegions": CLIP, "time_window": (2, 5), "lat_window": (0, 4)}, (2, 5), (1, 5), (2, 6)),
]


@pytest.mark.parametrize("order", ["lat_lon", "lon_lat"])
@pytest.mark.parametrize("request_, window, rows, cells", CASES)
def test_resolver_and_coordinate_cut(order, request_, window, rows, cells):
    lat_first = order == "lat_lon"
    dims = ("time", "latitude", "longitude") if lat_first else ("time", "longitude", "latitude")
    shape = (7, 6, 9) if lat_first else (7, 9, 6)
    coords = {"time": TIME, "latitude": LAT, "longitude": LON}
    box = None if rows is None else ((rows + cells) if lat_first else (cells + rows))
    got = afio._resolve_request(dims, shape, coords, XY, "time", lon_is_360=True, **request_)
    assert got == (window, box)
    cut = afio._cut_coords(dims, coords, *got)
    assert set(cut) == set(coords) and len(coords["time"]) == 7                   # (the source's coordinates are left as they were)
    assert cut["time"].equals(TIME if window is None else TIME[window[0]:window[1]])
    np.testing.assert_array_equal(cut["latitude"], LAT if rows is None else LAT[rows[0]:rows[1]])
    np.testing.assert_array_equal(cut["longitude"], LON if cells is None else LON[cells[0]:cells[1]])


def test_resolver_leaves_to_the_dataset_what_it_cannot_cut():
    dims, shape = ("time", "latitude", "longitude"), (7, 6, 9)
    coords = {"time": TIME, "latitude": LAT, "longitude": LON}
    # no decoded time coordinate: `Dataset` applies the selection afterwards
    assert afio._resolve_request(dims, shape, {"latitude": LAT, "longitude": LON}, XY, "time", time_sel=slice("2001-01-03", None)) == (None, None)
    # a selection `_time_window` cannot turn into one run (a descending index)
    assert afio._resolve_request(dims, shape, dict(coords, time=TIME[::-1]), XY, "time", time_sel=slice("2001-01-03", "2001-01-05")) == (None, None)
    # a clip that is no contiguous run of rows (latitudes out of order: row 2 lies outside, rows 1 and 3..5 inside): no box
    scattered = dict(coords, latitude=np.array([40.0, 41.0, 45.0, 42.0, 43.0, 44.0]))
    assert afio._resolve_request(dims, shape, scattered, XY, "time", georegions=CLIP) == (None, None)


def test_resolver_errors_keep_their_messages():
    dims, shape = ("time", "latitude", "longitude"), (7, 6, 9)
    coords = {"time": TIME, "latitude": LAT, "longitude": LON}
    scattered = dict(coords, latitude=np.array([40.0, 41.0, 45.0, 42.0, 43.0, 44.0]))
    with pytest.raises(ValueError, match="lat_window on a non-contiguous clip goes through the host route"):
        afio._resolve_request(dims, shape, scattered, XY, "time", georegions=CLIP, lat_window=(0, 2))
    with pytest.raises(ValueError, match=r"lat_window \(2, 6\) outside the 4 latitude rows of the grid"):
        afio._resolve_request(dims, shape, coords, XY, "time", georegions=CLIP, lat_window=(2, 6))
    with pytest.raises(ValueError, match="time_window needs a time-leading or a time-last array"):
        afio._resolve_request(("latitude", "longitude", "time"), (6, 9, 7), coords, XY, "time", time_window=(2, 5))


def test_file_sources_refuse_a_window_outside_their_steps(tmp_path):
    """The chunked routes clamp such a window (`_ScatterJob`); a file has no step outside its own.  The check needs no GPU: it comes
    before anything is staged."""
    case = {c.name: c for c in N.build_cases()}["short_cdf1"]
    src = afio._netcdf3_source(case.write(tmp_path), "t2m")
    with pytest.raises(ValueError, match=r"time_window \(5, 8\) outside the 7 steps of 't2m'"):
        src.to_device("cuda", (5, 8), None, False)
    gcase = {c.name: c for c in G.build_cases()}["e1_n12"]
    gsrc = afio._grib_source(gcase.write(tmp_path), "t2m")
    with pytest.raises(ValueError, match=r"time_window \(-1, 3\) outside the 7 steps of 't2m'"):
        gsrc.to_device("cuda", (-1, 3), None)


# ---------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------
def _zarr_dataset(T=7, ny=4, nx=5):
    cube = np.arange(T * ny * nx, dtype=np.float32).reshape(T, ny, nx)
    time = pd.date_range("2003-01-01", periods=T, freq="h")
    ds = af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                 {"time": time, "latitude": 30 + 0.5 * np.arange(ny), "longitude": 10 + 0.5 * np.arange(nx)}), lon_is_360=True)
    return ds, time


def _check(src, shape, dtype, packing, time, step_bytes, path, var):
    assert isinstance(src, afio._StreamedSource)
    assert tuple(src.dims) == ("time", "latitude", "longitude") and tuple(src.shape) == shape
    assert np.dtype(src.dtype) == np.dtype(dtype) and np.dtype(src.dtype).isnative and src.name == var
    assert src.packing == packing
    assert not any(isinstance(v, np.generic) for v in src.attrs.values())
    got = src.coords()["time"]
    assert isinstance(got, pd.DatetimeIndex) and got.equals(pd.DatetimeIndex(time))
    assert src.step_bytes() == step_bytes == D._step_bytes(path, var)


@pytest.mark.parametrize("layout", ["time-major", "time-last"])
def test_probe_takes_a_zarr_store(tmp_path, layout, monkeypatch):
    monkeypatch.delenv("AGGFLY_HIP_KEEP_PACKED", raising=False)
    ds, time = _zarr_dataset()
    path = str(tmp_path / "s.zarr")
    af.dataset_to_zarr(ds, path, var="t2m", chunks={"time": 4, "latitude": 2, "longitude": 5}, layout=layout)
    stored = afio.ZarrArray(os.path.join(path, "t2m"))
    assert stored.shape == ((7, 4, 5) if layout == "time-major" else (4, 5, 7))
    src = afio._streamed_source(path, "t2m", XY, "time")
    assert type(src) is afio._ZarrSource and src.tlast == (layout == "time-last")
    _check(src, (7, 4, 5), np.float32, None, time, 4 * 5 * 4, path, "t2m")      # time-major either way, as the tensor lies in HBM
    assert src.step_bytes(keep_packed=True) == 4 * 5 * 4                        # float storage is not packed, whatever is asked for


@pytest.mark.parametrize("fn", ["nc4_like.nc", "unlimited_time.nc"])
def test_probe_takes_a_chunked_netcdf4_variable(fn, monkeypatch):
    monkeypatch.delenv("AGGFLY_HIP_KEEP_PACKED", raising=False)
    path = os.path.join(FIX, fn)
    src = afio._streamed_source(path, "t2m", XY, "time")
    assert type(src) is afio._H5Source
    time = pd.Timestamp("2000-01-01") + pd.to_timedelta(6 * np.arange(37), unit="h")      # (tests/golden/make_hdf5_fixtures.py)
    _check(src, (37, 9, 14), np.float32, None, time, 9 * 14 * 4, path, "t2m")
    np.testing.assert_array_equal(src.coords()["latitude"], (50 - 0.25 * np.arange(9)).astype(np.float32))
    assert src.takes(1, (0, 5), None) and not src.takes(1, None, (0, 2)) and not src.takes(2, None, None)


def test_probe_takes_classic_files(tmp_path, monkeypatch):
    monkeypatch.delenv("AGGFLY_HIP_KEEP_PACKED", raising=False)
    by = {c.name: c for c in N.build_cases()}
    time = pd.Timestamp("1900-01-01") + pd.to_timedelta(876576 + np.arange(7), unit="h")
    path = by["short_cdf1"].write(tmp_path)
    src = afio._streamed_source(path, "t2m", XY, "time")
    assert type(src) is afio._Nc3Source
    _check(src, (7, 3, 5), np.int16, (0.0018311105046321, 273.6425033329, -32767, False), time, 3 * 5 * 4, path, "t2m")
    assert src.step_bytes(keep_packed=True) == 3 * 5 * 2 == D._step_bytes(path, "t2m", keep_packed=True)
    path = by["float_cdf1"].write(tmp_path)
    src = afio._streamed_source(path, "ws", XY, "time")
    _check(src, (7, 3, 5), np.float32, None, time, 3 * 5 * 4, path, "ws")
    assert src.takes(1, (0, 3), (0, 2)) and src.takes(3, None, (0, 2)) and not src.takes(3, (0, 3), None)
    assert afio._streamed_source(path, "ws", XY, "time", engine="netcdf4") is None       # another reader was asked for


def test_probe_takes_a_grib_file(tmp_path):
    case = {c.name: c for c in G.build_cases()}["e1_n12"]
    path = case.write(tmp_path)
    src = afio._streamed_source(path, "t2m", XY, "time")
    assert type(src) is afio._GribSource and not src.host_route
    _check(src, (7, G.NJ, G.NI), np.float32, None, case.times, G.NJ * G.NI * 4, path, "t2m")
    assert (G.NJ, G.NI) == (5, 9) and src.step_bytes(keep_packed=True) == 5 * 9 * 4      # keep_packed is ignored
    with pytest.raises(KeyError, match="msl"):                                           # what grib.py refuses raises: no other route
        afio._streamed_source(path, "msl", XY, "time")


def test_probe_declines_what_no_route_streams(tmp_path):
    lat, lon = N._grid(3, 5)
    dims = [("time", None), ("latitude", 3), ("longitude", 5), ("level", 2)]
    variables = [("longitude", ("longitude",), {}, lon), ("latitude", ("latitude",), {}, lat),
                 ("time", ("time",), {"units": N.HOURS}, np.arange(7, dtype=np.int32)),
                 ("c", ("time", "latitude", "longitude"), {}, np.full((7, 3, 5), b"x", "S1")),
                 ("four", ("time", "level", "latitude", "longitude"), {}, np.zeros((7, 2, 3, 5), np.float32))]
    classic = str(tmp_path / "mixed.nc")
    N.write_classic(classic, 1, dims, variables, 7)
    assert afio._streamed_source(classic, "c", XY, "time") is None                        # a char variable
    assert afio._streamed_source(classic, "four", XY, "time") is None                     # a 4-D variable
    assert afio._streamed_source(os.path.join(FIX, "nc4_like.nc"), "t2m_packed", XY, "time") is None      # a contiguous HDF5 variable
    other = tmp_path / "notes.txt"
    other.write_text("none of the formats\n")
    assert afio._streamed_source(str(other), "t2m", XY, "time") is None
    assert D._step_bytes(str(other), "t2m") is None


# ---------------------------------------------------------------------------------------
# the time axis of a multi-file dataset
# ---------------------------------------------------------------------------------------
def test_time_concatenation_on_both_kinds_of_index():
    a, b = pd.date_range("2001-01-30", periods=3, freq="D"), pd.date_range("2001-02-02", periods=2, freq="D")
    got = afio._concat_time([a, b])
    assert isinstance(got, pd.DatetimeIndex) and got.equals(pd.date_range("2001-01-30", periods=5, freq="D"))
    # noleap: 2001-02-27 + 4 days crosses into March without a leap day in any year
    units = "days since 2000-02-27"
    ca, cb = decode_cf_time(np.arange(0, 2), units, "noleap"), decode_cf_time(np.arange(2, 5), units, "noleap")
    assert isinstance(ca, CFTimeIndex)
    got = afio._concat_time([ca, cb])
    want = decode_cf_time(np.arange(0, 5), units, "noleap")
    assert isinstance(got, CFTimeIndex) and got.calendar == want.calendar == "noleap" and len(got) == 5
    np.testing.assert_array_equal(got.seconds, want.seconds)
    np.testing.assert_array_equal(got.seconds, np.concatenate([ca.seconds, cb.seconds]))
