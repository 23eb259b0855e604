"""Time-last Zarr stores — (latitude, longitude, time), what the reference's converter writes — streamed into HBM: the transposing
placement kernel (`afhip_place_box_tlast`) against numpy, its refusals, and every device route of `dataset_from_path` on such
stores against the cube they were written from.  All comparisons are bit-exact: this is a copy."""
import json
import os

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import distributed as D, engine as eng, hip, io as afio, synth

pytestmark = pytest.mark.gpu

NP_OF = {2: np.int16, 4: np.int32, 8: np.int64}
SENTINEL = -7


def _chunk(shape, es, seed=0):
    rng = np.random.default_rng(seed)
    info = np.iinfo(NP_OF[es])
    return rng.integers(info.min // 2, info.max // 2, shape).astype(NP_OF[es])


def _place(torch, chunk, cube_shape, box, at):
    """-> (the cube after `hip.place_box_tlast`, the cube numpy makes of the same arguments)."""
    (sy, sx, st, ny, nx, nt), (t0, y0, x0) = box, at
    want = np.full(cube_shape, SENTINEL, dtype=chunk.dtype)
    want[t0:t0 + nt, y0:y0 + ny, x0:x0 + nx] = chunk[sy:sy + ny, sx:sx + nx, st:st + nt].transpose(2, 0, 1)
    cube = torch.full(cube_shape, SENTINEL, dtype=getattr(torch, chunk.dtype.name), device="cuda")
    hip.place_box_tlast(torch.from_numpy(chunk).cuda(), cube, box, at)
    torch.cuda.synchronize()
    return cube.cpu().numpy(), want


KERNEL_CASES = {
    # chunk [by][bx][bt], cube [T][NY][NX], (sy, sx, st, ny, nx, nt), (t0, y0, x0)
    "ragged": ((3, 70, 133), (130, 4, 71), (1, 3, 5, 2, 65, 127), (2, 1, 5)),          # no extent a multiple of a tile
    "aligned": ((1, 128, 128), (128, 1, 128), (0, 0, 0, 1, 128, 128), (0, 0, 0)),
    "one_step": ((3, 70, 133), (130, 4, 71), (1, 3, 5, 2, 65, 1), (129, 1, 5)),
    "one_column": ((3, 70, 133), (130, 4, 71), (1, 3, 5, 2, 1, 127), (2, 1, 70)),
    "last_element": ((3, 70, 133), (130, 4, 71), (2, 69, 132, 1, 1, 1), (129, 3, 70)),
}


@pytest.mark.parametrize("es", [2, 4, 8])
@pytest.mark.parametrize("case", list(KERNEL_CASES))
def test_kernel_against_numpy(torch_cuda, es, case):
    chunk_shape, cube_shape, box, at = KERNEL_CASES[case]
    got, want = _place(torch_cuda, _chunk(chunk_shape, es, seed=es), cube_shape, box, at)
    np.testing.assert_array_equal(got, want)                  # the whole cube: one stray write fails


@pytest.mark.parametrize("es", [2, 4, 8])
@pytest.mark.parametrize("box", [(1, 3, 5, 0, 65, 127), (1, 3, 5, 2, 0, 127), (1, 3, 5, 2, 65, 0)])
def test_an_empty_box_leaves_the_cube_untouched(torch_cuda, es, box):
    got, want = _place(torch_cuda, _chunk((3, 70, 133), es), (130, 4, 71), box, (2, 1, 5))
    assert (want == SENTINEL).all()
    np.testing.assert_array_equal(got, want)


REFUSED = {
    # one element outside the chunk [3][70][133] ...
    "chunk_y": ((1, 3, 5, 3, 65, 127), (2, 0, 5)),
    "chunk_x": ((1, 3, 5, 2, 68, 127), (2, 1, 2)),
    "chunk_t": ((1, 3, 5, 2, 65, 129), (0, 1, 5)),
    # ... or the cube [130][4][71]
    "cube_y": ((1, 3, 5, 2, 65, 127), (2, 3, 5)),
    "cube_x": ((1, 3, 5, 2, 65, 127), (2, 1, 7)),
    "cube_t": ((1, 3, 5, 2, 65, 127), (4, 1, 5)),
    "negative": ((1, -1, 5, 2, 65, 127), (2, 1, 5)),
}


@pytest.mark.parametrize("es", [2, 4, 8])
@pytest.mark.parametrize("case", list(REFUSED))
def test_a_box_outside_the_chunk_or_the_cube_is_refused(torch_cuda, es, case):
    torch = torch_cuda
    box, at = REFUSED[case]
    chunk = torch.from_numpy(_chunk((3, 70, 133), es)).cuda()
    cube = torch.full((130, 4, 71), SENTINEL, dtype=chunk.dtype, device="cuda")
    with pytest.raises(ValueError, match="place_box_tlast"):
        hip.place_box_tlast(chunk, cube, box, at)
    torch.cuda.synchronize()
    assert bool((cube == SENTINEL).all())


def test_other_element_sizes_and_strided_tensors_are_refused(torch_cuda):
    torch = torch_cuda
    box, at = (0, 0, 0, 2, 8, 8), (0, 0, 0)
    chunk = torch.from_numpy(_chunk((3, 70, 133), 4)).cuda()
    for cube in (torch.full((130, 4, 71), SENTINEL, dtype=torch.int16, device="cuda"),                     # another element size
                 torch.full((130, 4, 142), SENTINEL, dtype=torch.int32, device="cuda")[:, :, ::2],          # a strided cube
                 torch.full((130, 4 * 71), SENTINEL, dtype=torch.int32, device="cuda")):                    # not 3-D
        with pytest.raises(ValueError, match="place_box_tlast"):
            hip.place_box_tlast(chunk, cube, box, at)
        torch.cuda.synchronize()
        assert bool((cube == SENTINEL).all())
    cube = torch.full((130, 4, 71), SENTINEL, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="place_box_tlast"):
        hip.place_box_tlast(chunk.permute(0, 2, 1), cube, box, at)                                         # a strided chunk
    one = torch.full((130, 4, 71), SENTINEL, dtype=torch.int8, device="cuda")
    with pytest.raises(ValueError, match="place_box_tlast"):                                               # 1-byte elements: no kernel
        hip.place_box_tlast(torch.zeros((3, 70, 133), dtype=torch.int8, device="cuda"), one, box, at)
    torch.cuda.synchronize()
    assert bool((cube == SENTINEL).all()) and bool((one == SENTINEL).all())


# ---- stores ----
T, NY, NX = 480, 12, 16
TIME = pd.date_range("2003-01-01", periods=T, freq="h")
LAT, LON = 30 + 0.5 * np.arange(NY), 10 + 0.5 * np.arange(NX)
SEL = slice("2003-01-03 05:00", "2003-01-11 17:00")                # steps 53 .. 258
K0, K1 = 53, 258
# an interior box: with half a cell of slack the clip keeps latitude rows 3..8 and longitude columns 4..9
REGIONS = pd.DataFrame({"geoid": ["a", "b"], "minx": [12.0, 13.0], "miny": [31.6, 32.0], "maxx": [13.5, 14.4], "maxy": [33.0, 33.9]})
BOX = (3, 9, 4, 10)
_CUBES = {}


def _cube(dtype):
    """One reference cube per dtype, computed once, shared by every test and never written to."""
    key = np.dtype(dtype).name
    if key not in _CUBES:
        _CUBES[key] = synth.temperature_cube(T, NY, NX, dtype=dtype, seed=5, scattered_nan=7)
    return _CUBES[key]


def _dataset(cube, time=TIME):
    return af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"], {"time": time, "latitude": LAT, "longitude": LON}), lon_is_360=True)


def _spy_chunks(monkeypatch, var="t2m"):
    """The chunk indices of the data variable that any read route asks `ZarrArray.chunk_locator` for."""
    seen = set()
    real = afio.ZarrArray.chunk_locator

    def chunk_locator(self, idx, *a, **k):
        if os.path.basename(self.path) == var:
            seen.add(tuple(int(i) for i in idx))
        return real(self, idx, *a, **k)

    monkeypatch.setattr(afio.ZarrArray, "chunk_locator", chunk_locator)
    return seen


def _touching(chunks, box, k0=0, k1=T):
    """Chunk indices (iy, ix, it) of a time-last array of ``chunks`` = (yc, xc, tc) that touch rows / columns ``box`` and steps [k0, k1)."""
    yc, xc, tc = chunks
    return {(iy, ix, it) for iy in range(box[0] // yc, -(-box[1] // yc)) for ix in range(box[2] // xc, -(-box[3] // xc))
            for it in range(k0 // tc, -(-k1 // tc))}


def _check_store(torch, path, cube, chunks, monkeypatch, absent=None):
    want = cube
    if absent is not None:
        want = cube.copy()
        want[absent] = np.nan
    seen = _spy_chunks(monkeypatch)
    for mode in ("1", "0"):
        monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
        d = af.dataset_from_path(path, "t2m", device="cuda")
        data = d.da.transpose("time", "latitude", "longitude").data
        assert data.is_cuda and data.is_contiguous() and d.cube().data_ptr() == data.data_ptr()      # time-major in HBM: cube() is free
        assert d.da.dims == ("latitude", "longitude", "time") and d.time.equals(TIME)
        np.testing.assert_array_equal(d.cube().cpu().numpy(), want)
        np.testing.assert_array_equal(d.latitude, LAT)
        np.testing.assert_array_equal(d.longitude, LON)
        seen.clear()
        d = af.dataset_from_path(path, "t2m", device="cuda", time_sel=SEL)
        assert seen == _touching(chunks, (0, NY, 0, NX), K0, K1)
        assert d.time.equals(TIME[K0:K1]) and d.cube().data_ptr() == d.da.transpose("time", "latitude", "longitude").data.data_ptr()
        np.testing.assert_array_equal(d.cube().cpu().numpy(), want[K0:K1])
        d = af.dataset_from_path(path, "t2m", device="cuda", time_window=(K0, K1))
        assert d.cube().is_cuda and d.cube().shape == (205, NY, NX) and d.time.equals(TIME[K0:K1])
        np.testing.assert_array_equal(d.cube().cpu().numpy(), want[K0:K1])
        d = af.dataset_from_path(path, "t2m", device="cuda", time_window=(0, 0))
        assert d.cube().is_cuda and d.cube().shape == (0, NY, NX) and len(d.time) == 0
        np.testing.assert_array_equal(d.latitude, LAT)
        seen.clear()
        d = af.dataset_from_path(path, "t2m", device="cuda", georegions=af.GeoRegions(REGIONS))
        assert seen == _touching(chunks, BOX)
        np.testing.assert_array_equal(d.cube().cpu().numpy(), want[:, BOX[0]:BOX[1], BOX[2]:BOX[3]])
        np.testing.assert_array_equal(d.latitude, LAT[BOX[0]:BOX[1]])
        np.testing.assert_array_equal(d.longitude, LON[BOX[2]:BOX[3]])
        seen.clear()
        d = af.dataset_from_path(path, "t2m", device="cuda", lat_window=(3, 9))
        assert seen == _touching(chunks, (3, 9, 0, NX))
        np.testing.assert_array_equal(d.cube().cpu().numpy(), want[:, 3:9])
        np.testing.assert_array_equal(d.latitude, LAT[3:9])


@pytest.mark.parametrize("chunks", [(6, 6, T), (5, 7, 96)], ids=["whole_series_tiles", "ragged"])
@pytest.mark.parametrize("compress", [False, True, "zstd"], ids=["raw", "blosc_lz4", "zstd"])
@pytest.mark.parametrize("fmt", [2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_time_last_stores_on_every_device_route(torch_cuda, tmp_path, monkeypatch, dtype, fmt, compress, chunks):
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE_HOST_TAIL_MIN_MB", "0")      # the decode-in-HBM route's host-decoded tail takes part
    cube = _cube(dtype)
    path = str(tmp_path / "tl.zarr")
    af.dataset_to_zarr(_dataset(cube), path, var="t2m", chunks={"latitude": chunks[0], "longitude": chunks[1], "time": chunks[2]},
                       compress=compress, zarr_format=fmt, layout="time-last")
    za = afio.ZarrArray(os.path.join(path, "t2m"))
    assert za.dims == ("latitude", "longitude", "time") and za.chunks == chunks
    _check_store(torch_cuda, path, cube, chunks, monkeypatch)


def test_a_sharded_time_last_store(torch_cuda, tmp_path, monkeypatch):
    cube = _cube(np.float32)
    path = str(tmp_path / "sh.zarr")
    af.dataset_to_zarr(_dataset(cube), path, var="t2m", chunks={"latitude": 6, "longitude": 8, "time": 96},
                       shards={"latitude": 12, "longitude": 16, "time": 192}, compress="zstd", zarr_format=3, layout="time-last")
    za = afio.ZarrArray(os.path.join(path, "t2m"))
    assert za.shard_shape == (12, 16, 192) and za.chunks == (6, 8, 96)
    _check_store(torch_cuda, path, cube, (6, 8, 96), monkeypatch)


@pytest.mark.parametrize("compress", [True, "zstd"], ids=["blosc_lz4", "zstd"])
def test_an_absent_chunk_is_the_fill_value(torch_cuda, tmp_path, monkeypatch, compress):
    cube = _cube(np.float32)
    path = str(tmp_path / "absent.zarr")
    af.dataset_to_zarr(_dataset(cube), path, var="t2m", chunks={"latitude": 5, "longitude": 7, "time": 96}, compress=compress, layout="time-last")
    os.remove(afio.ZarrArray(os.path.join(path, "t2m")).chunk_path((1, 0, 2)))         # rows 5..9, columns 0..6, steps 192..287
    _check_store(torch_cuda, path, cube, (5, 7, 96), monkeypatch, absent=(slice(192, 288), slice(5, 10), slice(0, 7)))


# ---- packed and joined stores ----
def _packed_store(path, stored, dims, chunks, attrs, time):
    tv, tattrs = afio._encode_time(time)
    os.makedirs(path)
    with open(os.path.join(path, ".zgroup"), "w") as f:
        json.dump({"zarr_format": 2}, f)
    afio._write_array(path, "t2m", stored, dims, chunks, attrs, {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0})
    afio._write_array(path, "time", np.asarray(tv, dtype=np.float64), ("time",), (len(time),), tattrs, None)
    afio._write_array(path, "latitude", LAT, ("latitude",), (NY,), {}, None)
    afio._write_array(path, "longitude", LON, ("longitude",), (NX,), {}, None)


@pytest.mark.parametrize("storage", ["int16", "uint16"])
def test_a_packed_time_last_store_stays_packed_like_the_time_major_one(torch_cuda, tmp_path, monkeypatch, storage):
    rng = np.random.default_rng(8)
    if storage == "int16":
        stored = rng.integers(-30000, 30000, (T, NY, NX)).astype(np.int16)
        attrs = {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}
    else:
        stored = rng.integers(0, 65000, (T, NY, NX)).astype(np.uint16)
        attrs = {"scale_factor": 0.1, "add_offset": -50.0, "_FillValue": 65535}
    stored[rng.random((T, NY, NX)) < 0.02] = attrs["_FillValue"]
    major, last = str(tmp_path / "major.zarr"), str(tmp_path / "last.zarr")
    _packed_store(major, stored, ("time", "latitude", "longitude"), (96, 5, 7), attrs, TIME)
    _packed_store(last, np.ascontiguousarray(stored.transpose(1, 2, 0)), ("latitude", "longitude", "time"), (5, 7, 96), attrs, TIME)
    for mode in ("1", "0"):
        monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
        a = af.dataset_from_path(major, "t2m", device="cuda", keep_packed=True)
        b = af.dataset_from_path(last, "t2m", device="cuda", keep_packed=True)
        assert a.is_packed and b.is_packed
        pa, pb = a.packed_cube(), b.packed_cube()
        assert pb.q.is_cuda and pb.q.dtype == pa.q.dtype and pa.rules == pb.rules and pa.unsigned == pb.unsigned
        np.testing.assert_array_equal(pb.q.cpu().numpy(), pa.q.cpu().numpy())
        np.testing.assert_array_equal(pb.q.cpu().numpy().view(stored.dtype), stored)
        # the float32 route of the same store (the casting fallback of the placement) gives the values the time-major store gives
        fa = af.dataset_from_path(major, "t2m", device="cuda", time_sel=SEL)
        fb = af.dataset_from_path(last, "t2m", device="cuda", time_sel=SEL)
        assert not fb.is_packed
        np.testing.assert_array_equal(fb.cube().cpu().numpy(), fa.cube().cpu().numpy())


def test_time_last_stores_join_along_time_also_beside_a_time_major_one(torch_cuda, tmp_path, monkeypatch):
    cube = _cube(np.float32)
    half = T // 2
    paths = {}
    for name, (k0, k1), layout in (("a_last", (0, half), "time-last"), ("b_last", (half, T), "time-last"), ("b_major", (half, T), "time-major")):
        paths[name] = str(tmp_path / f"{name}.zarr")
        af.dataset_to_zarr(_dataset(cube[k0:k1], TIME[k0:k1]), paths[name], var="t2m", chunks={"latitude": 5, "longitude": 7, "time": 96},
                           compress="zstd", zarr_format=3, layout=layout)
    for mode in ("1", "0"):
        monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
        for second in ("b_last", "b_major"):
            d = af.dataset_from_path([paths["a_last"], paths[second]], "t2m", device="cuda")
            assert d.cube().is_cuda and d.time.equals(TIME)
            np.testing.assert_array_equal(d.cube().cpu().numpy(), cube)
            d = af.dataset_from_path([paths["a_last"], paths[second]], "t2m", device="cuda", time_sel=SEL)
            assert d.time.equals(TIME[K0:K1])
            np.testing.assert_array_equal(d.cube().cpu().numpy(), cube[K0:K1])
        d = af.dataset_from_path(str(tmp_path / "*_last.zarr"), "t2m", device="cuda")
        np.testing.assert_array_equal(d.cube().cpu().numpy(), cube)


# ---- sharded aggregation ----
def test_store_sharded_and_cell_sharded_aggregation_of_a_time_last_store(torch_cuda, tmp_path, monkeypatch):
    cube = _cube(np.float64)
    ds = _dataset(cube)
    last, major = str(tmp_path / "agg_last.zarr"), str(tmp_path / "agg_major.zarr")
    chunks = {"latitude": 5, "longitude": 7, "time": 96}
    af.dataset_to_zarr(ds, last, var="t2m", chunks=chunks, compress="zstd", zarr_format=3, layout="time-last")
    af.dataset_to_zarr(ds, major, var="t2m", chunks=chunks, compress="zstd", zarr_format=3)
    tab = synth.weights_table(NY, NX, 6, seed=62, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}))
    spec = dict(dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": "date"})],
                t=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 3)}),
                   ("aggregate", {"calc": "sum", "groupby": "date"})])
    weights_of = lambda d: af.weights_from_objects(d, gr, table=tab)
    opened = []
    real_open = afio.dataset_from_path
    monkeypatch.setattr(afio, "dataset_from_path", lambda *a, **k: opened.append(k.get("time_window")) or real_open(*a, **k))
    old = eng.config.exact_order
    try:
        eng.config.exact_order = True                  # no period is split, so a period's sums do not depend on its window
        want = af.aggregate_dataset(dataset=ds.to_device(), weights=weights_of(ds), aggregator_dict=spec)
        # a budget of a week of steps per window: 20 days go through HBM in at least three windows
        got = D.aggregate_store_sharded(weights_of, last, "t2m", spec, lon_is_360=True, max_window_bytes=7 * 24 * D._step_bytes(last, "t2m"))
        assert D._step_bytes(last, "t2m") == NY * NX * 8
        assert len(opened) >= 3 and opened[0][0] == 0 and opened[-1][1] == T, opened
        assert all(a[1] == b[0] for a, b in zip(opened, opened[1:])), opened
        assert len(got) == len(want) > 0
        pd.testing.assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True))
        cells = D.aggregate_store_cells(weights_of, last, "t2m", spec, lon_is_360=True)
        pd.testing.assert_frame_equal(cells.reset_index(drop=True), want.reset_index(drop=True))
        a = real_open(last, "t2m", lon_is_360=True, device="cuda")
        b = real_open(major, "t2m", lon_is_360=True, device="cuda")
        pd.testing.assert_frame_equal(af.aggregate_dataset(dataset=a, weights=weights_of(a), aggregator_dict=spec),
                                      af.aggregate_dataset(dataset=b, weights=weights_of(b), aggregator_dict=spec))
    finally:
        eng.config.exact_order = old
