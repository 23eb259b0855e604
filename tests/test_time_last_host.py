"""Time-last Zarr stores — (latitude, longitude, time), what the reference's converter writes — on the host: the writer's
``layout=``, the host read back, the bytes of one time step as the window planner counts them, and the library entry's declaration."""
import json
import os

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import distributed as D, hip, io as afio, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ds(T, ny, nx, dtype=np.float32, seed=3):
    cube = synth.temperature_cube(T, ny, nx, dtype=dtype, seed=seed, scattered_nan=5)
    time = pd.date_range("2003-01-01", periods=T, freq="h")
    return af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                   {"time": time, "latitude": 30 + 0.5 * np.arange(ny), "longitude": 10 + 0.5 * np.arange(nx)}),
                      lon_is_360=True), cube


def _tree(path):
    out = {}
    for d, _, files in os.walk(path):
        for f in files:
            with open(os.path.join(d, f), "rb") as h:
                out[os.path.relpath(os.path.join(d, f), path)] = h.read()
    return out


@pytest.mark.parametrize("fmt", [2, 3])
@pytest.mark.parametrize("compress", [True, "zstd", False])
def test_time_last_layout_is_written_reordered_and_reads_back(tmp_path, fmt, compress):
    T, ny, nx = 50, 9, 13
    ds, cube = _ds(T, ny, nx)
    chunks = {"time": 20, "latitude": 4, "longitude": 5}
    path = str(tmp_path / "tl.zarr")
    af.dataset_to_zarr(ds, path, var="t2m", chunks=chunks, compress=compress, zarr_format=fmt, layout="time-last")
    za = afio.ZarrArray(os.path.join(path, "t2m"))
    assert za.dims == ("latitude", "longitude", "time")
    assert za.shape == (ny, nx, T) and za.chunks == (4, 5, 20)
    np.testing.assert_array_equal(za.read(), cube.transpose(1, 2, 0))
    back = af.dataset_from_path(path, "t2m")
    np.testing.assert_array_equal(back.cube(), cube)
    assert back.time.equals(ds.time)
    np.testing.assert_array_equal(back.latitude, ds.latitude)
    np.testing.assert_array_equal(back.longitude, ds.longitude)


@pytest.mark.parametrize("fmt", [2, 3])
def test_default_chunks_are_the_auto_chunks_reordered(tmp_path, fmt):
    T, ny, nx = 50, 40, 45
    ds, cube = _ds(T, ny, nx)
    path = str(tmp_path / "auto.zarr")
    af.dataset_to_zarr(ds, path, var="t2m", zarr_format=fmt, layout="time-last")
    auto = afio._auto_chunks({"time": T, "latitude": ny, "longitude": nx}, 4)
    want = tuple({"time": T, "latitude": ny, "longitude": nx}[d] if auto[d] == -1 else min(auto[d], {"time": T, "latitude": ny, "longitude": nx}[d])
                 for d in ("latitude", "longitude", "time"))
    za = afio.ZarrArray(os.path.join(path, "t2m"))
    assert za.chunks == want and za.chunks[2] == T           # the whole series in square tiles, time last
    major = str(tmp_path / "auto_major.zarr")
    af.dataset_to_zarr(ds, major, var="t2m", zarr_format=fmt)
    zm = afio.ZarrArray(os.path.join(major, "t2m"))
    assert za.chunks == (zm.chunks[1], zm.chunks[2], zm.chunks[0])
    np.testing.assert_array_equal(af.dataset_from_path(path, "t2m").cube(), cube)


def test_shards_are_reordered_too(tmp_path):
    T, ny, nx = 48, 12, 16
    ds, cube = _ds(T, ny, nx)
    path = str(tmp_path / "sh.zarr")
    af.dataset_to_zarr(ds, path, var="t2m", chunks={"time": 12, "latitude": 6, "longitude": 16}, shards={"time": 24, "latitude": 12, "longitude": 16},
                       compress="zstd", zarr_format=3, layout="time-last")
    za = afio.ZarrArray(os.path.join(path, "t2m"))
    assert za.chunks == (6, 16, 12) and za.shard_shape == (12, 16, 24) and za.dims == ("latitude", "longitude", "time")
    np.testing.assert_array_equal(af.dataset_from_path(path, "t2m").cube(), cube)


@pytest.mark.parametrize("fmt", [2, 3])
def test_time_major_keyword_writes_the_same_bytes_as_no_keyword(tmp_path, fmt):
    ds, _ = _ds(50, 9, 13)
    chunks = {"time": 20, "latitude": 4, "longitude": 5}
    a, b = str(tmp_path / "a.zarr"), str(tmp_path / "b.zarr")
    af.dataset_to_zarr(ds, a, var="t2m", chunks=chunks, zarr_format=fmt)
    af.dataset_to_zarr(ds, b, var="t2m", chunks=chunks, zarr_format=fmt, layout="time-major")
    ta, tb = _tree(a), _tree(b)
    assert ta.keys() == tb.keys() and len(ta) > 4
    assert all(ta[k] == tb[k] for k in ta)
    assert afio.ZarrArray(os.path.join(b, "t2m")).dims == ("time", "latitude", "longitude")


def test_gpu_encode_refuses_the_time_last_layout(tmp_path):
    ds, _ = _ds(24, 4, 5)
    with pytest.raises(ValueError, match="time-last"):
        af.dataset_to_zarr(ds, str(tmp_path / "g.zarr"), var="t2m", encode="gpu", layout="time-last")
    with pytest.raises(ValueError, match="layout"):
        af.dataset_to_zarr(ds, str(tmp_path / "h.zarr"), var="t2m", layout="time-first")
    assert not os.path.exists(str(tmp_path / "g.zarr"))       # refused before anything is written


def test_zarr_from_path_passes_the_layout_on(tmp_path):
    ds, cube = _ds(30, 6, 7)
    src, dst = str(tmp_path / "src.zarr"), str(tmp_path / "dst.zarr")
    af.dataset_to_zarr(ds, src, var="t2m")
    afio.zarr_from_path(src, dst, "t2m", layout="time-last", zarr_format=3, compress="zstd")
    assert afio.ZarrArray(os.path.join(dst, "t2m")).dims == ("latitude", "longitude", "time")
    np.testing.assert_array_equal(af.dataset_from_path(dst, "t2m").cube(), cube)


def test_step_bytes_of_a_time_last_store_counts_the_two_spatial_extents(tmp_path):
    ny, nx, T = 9, 13, 50
    ds, _ = _ds(T, ny, nx)
    path = str(tmp_path / "sb.zarr")
    af.dataset_to_zarr(ds, path, var="t2m", chunks={"time": 20, "latitude": 4, "longitude": 5}, layout="time-last")
    assert afio.ZarrArray(os.path.join(path, "t2m")).shape == (9, 13, 50)
    assert D._step_bytes(path, "t2m") == 9 * 13 * 4            # (the product of shape[1:] would be 2600)
    major = str(tmp_path / "sb_major.zarr")
    af.dataset_to_zarr(ds, major, var="t2m")
    assert D._step_bytes(major, "t2m") == 9 * 13 * 4
    # an int16-packed time-last store: 4 bytes per cell unpacked to float32, 2 when it stays packed
    rng = np.random.default_rng(4)
    stored = rng.integers(-30000, 30000, (ny, nx, T)).astype(np.int16)
    attrs = {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}
    tv, tattrs = afio._encode_time(pd.date_range("2004-03-01", periods=T, freq="h"))
    packed = str(tmp_path / "sb_packed.zarr")
    os.makedirs(packed)
    with open(os.path.join(packed, ".zgroup"), "w") as f:
        json.dump({"zarr_format": 2}, f)
    afio._write_array(packed, "t2m", stored, ("latitude", "longitude", "time"), (4, 5, 20), attrs, None)
    afio._write_array(packed, "time", np.asarray(tv, dtype=np.float64), ("time",), (T,), tattrs, None)
    assert D._step_bytes(packed, "t2m") == 9 * 13 * 4
    assert D._step_bytes(packed, "t2m", keep_packed=True) == 9 * 13 * 2
    # another name for the time coordinate: the last dimension is then no time axis
    assert D._step_bytes(path, "t2m", timecoord="valid_time") == 13 * 50 * 4


def test_the_entry_is_exported_and_declared():
    assert "afhip_place_box_tlast" in hip.EXPORTS
    with open(os.path.join(ROOT, "include", "aggfly_hip.h")) as f:
        header = f.read()
    assert "int afhip_place_box_tlast(const void* chunk_dev, void* cube_dev, int elem_size," in header
    assert hasattr(hip, "place_box_tlast")
