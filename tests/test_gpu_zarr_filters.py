"""numcodecs element filters undone in HBM: `hip.delta_decode` against a wrapping running sum at every element size around the
tile and workgroup edges, `hip.fso_decode` against the numpy restatement of tests/zarr_filter_cases.py bit for bit, both with guard
bytes around every buffer and with their refusals, and `dataset_from_path(device="cuda")` on filtered stores against the host route
on the three scatter routes, with windows, a time-last store, an absent chunk and several stores."""
import ctypes as C
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zarr_filter_cases as Z  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import hip, io as afio, synth  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                                           # bytes of 0xA5 on either side of every buffer (a multiple of 16: alignment is kept)
TILE_BYTES = 16384                                   # afhip_filter_kernels.h: DELTA_TILE_BYTES
WG = 256                                             # lanes of the second pass: a chunk of more tiles takes several steps


def _guarded(torch, nbytes, shift=0):
    """A uint8 HBM buffer of ``nbytes`` with guards around it -> (whole, view); ``shift`` moves the view off its 16-byte alignment."""
    whole = torch.full((GUARD + shift + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD + shift:GUARD + shift + nbytes]


def _guards_intact(whole, nbytes, shift=0):
    return bool((whole[:GUARD + shift] == 0xA5).all()) and bool((whole[GUARD + shift + nbytes:] == 0xA5).all())


# ---- delta ----
def _delta_lengths(es):
    tile = TILE_BYTES // es
    return [1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 17, (WG + 1) * tile + 5]


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_delta_decode_against_a_wrapping_running_sum(torch_cuda, es):
    torch = torch_cuda
    dt = np.dtype(f"i{es}")
    info = np.iinfo(dt)
    rng = np.random.default_rng(es)
    for n in _delta_lengths(es):
        for n_chunks in (1, 2, 7):
            # differences over the whole range of the type: every running sum wraps within a few elements
            enc = rng.integers(info.min, info.max, size=(n_chunks, n), endpoint=True, dtype=np.int64).astype(dt)
            want = np.stack([Z.delta_decode_fast(row, dt) for row in enc])
            nbytes = enc.nbytes
            whole, stage = _guarded(torch, nbytes)
            stage.copy_(torch.from_numpy(enc.reshape(-1).view(np.uint8)))
            sbytes = hip.delta_scratch_bytes(n_chunks, n, es)
            swhole, scratch = _guarded(torch, sbytes)
            hip.delta_decode(stage, n_chunks, n, es, scratch)
            torch.cuda.synchronize()
            got = stage.cpu().numpy().view(dt).reshape(n_chunks, n)
            assert np.array_equal(got, want), (es, n, n_chunks, int(np.argmax(got != want)))
            assert _guards_intact(whole, nbytes) and _guards_intact(swhole, sbytes), (es, n, n_chunks)
    assert np.array_equal(Z.delta_decode_fast(enc[0, :300], dt), Z.delta_decode(enc[0, :300], dt))       # the two restatements agree


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_delta_decode_from_a_start_that_is_not_16_byte_aligned(torch_cuda, es):
    torch = torch_cuda
    dt = np.dtype(f"u{es}")
    n = 2 * (TILE_BYTES // es) + 3
    enc = np.random.default_rng(9).integers(0, np.iinfo(dt).max, size=n, endpoint=True, dtype=np.uint64).astype(dt)
    whole, stage = _guarded(torch, enc.nbytes, shift=es)
    stage.copy_(torch.from_numpy(enc.view(np.uint8)))
    swhole, scratch = _guarded(torch, hip.delta_scratch_bytes(1, n, es))
    hip.delta_decode(stage, 1, n, es, scratch)
    torch.cuda.synchronize()
    assert np.array_equal(stage.cpu().numpy().view(dt), Z.delta_decode_fast(enc, dt))
    assert _guards_intact(whole, enc.nbytes, shift=es) and _guards_intact(swhole, scratch.numel())


def test_delta_decode_refusals_touch_nothing(torch_cuda):
    torch = torch_cuda
    lib = hip.load()
    whole, stage = _guarded(torch, 1 << 16)
    swhole, scratch = _guarded(torch, 1 << 12)
    stage.fill_(0x11)
    scratch.fill_(0x22)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tile = TILE_BYTES // 2
    for n_chunks, chunk_elems, es, sbytes, why in [
            (1, 0, 2, 1 << 12, "chunk_elems"), (1, -5, 2, 1 << 12, "chunk_elems"), (-1, 8, 2, 1 << 12, "n_chunks"),
            (1, 64, 3, 1 << 12, "elem_size must be 1, 2, 4 or 8"), (1, 64, 16, 1 << 12, "elem_size must be 1, 2, 4 or 8"),
            (1 << 40, 1 << 40, 2, 1 << 12, "overflows or is too large"),                   # the product overflows int64
            (1, (1 << 31) * tile, 2, 1 << 12, "overflows or is too large"),                # more tiles than a grid has workgroups
            (1, (1 << 63) - 1, 1, 1 << 12, "overflows or is too large"),                   # the largest int64: no sum on the way may overflow
            (1 << 31, 4, 2, 1 << 12, "overflows or is too large"),                         # more chunks than the second pass has workgroups
            (1, 3 * tile, 2, 16, "scratch")]:                                               # a scratch smaller than the call needs
        rc = lib.afhip_delta_decode(stage.data_ptr(), n_chunks, chunk_elems, es, scratch.data_ptr(), sbytes, stream)
        assert rc == hip.E_INVALID, (n_chunks, chunk_elems, es)
        assert why in lib.afhip_last_error().decode(), (why, lib.afhip_last_error().decode())
        assert lib.afhip_delta_scratch_bytes(n_chunks, chunk_elems, es) == -1 or why == "scratch"
    with pytest.raises(ValueError, match="do not fit the stage"):
        hip.delta_decode(stage, 2, 1 << 16, 1, scratch)                                     # the binding checks the tensor's size
    assert lib.afhip_delta_decode(stage.data_ptr(), 0, 8, 2, scratch.data_ptr(), 1 << 12, stream) == 0     # no chunks: nothing to do
    torch.cuda.synchronize()
    assert bool((stage == 0x11).all()) and bool((scratch == 0x22).all())
    assert _guards_intact(whole, 1 << 16) and _guards_intact(swhole, 1 << 12)


# ---- fixedscaleoffset ----
def _fso(torch, enc, out_np, scale, offset, shift_src=0, shift_dst=0):
    """`hip.fso_decode` on ``enc`` between guards -> the decoded array; the guards are checked."""
    out_np = np.dtype(out_np)
    swhole, src = _guarded(torch, enc.nbytes, shift=shift_src)
    src.copy_(torch.from_numpy(np.ascontiguousarray(enc).view(np.uint8)))
    dwhole, dst8 = _guarded(torch, enc.size * out_np.itemsize, shift=shift_dst)
    dst = dst8.view(torch.float32 if out_np == np.float32 else torch.float64)
    hip.fso_decode(src, dst, enc.size, enc.dtype.name, scale, offset)
    torch.cuda.synchronize()
    assert _guards_intact(swhole, enc.nbytes, shift_src) and _guards_intact(dwhole, dst8.numel(), shift_dst)
    return dst.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(f"u{a.dtype.itemsize}")


@pytest.mark.parametrize("out_np", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", Z.TYPE_NAMES)
def test_fso_decode_every_source_type(torch_cuda, name, out_np):
    rng = np.random.default_rng(11)
    for n in (1, 15, 16, 17, 4099):                         # around a lane's run, and an odd length beyond one workgroup
        enc = Z.type_code_arrays(rng, name, n)
        for scale, offset in ((10.0, 273.15), (128.0, -5.5), (1.0, 0.0)):       # a decimal scale, a power of two, the plain conversion
            got = _fso(torch_cuda, enc, out_np, scale, offset)
            want = Z.fso_decode(enc, scale, offset, out_np)
            assert got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want)), (name, n, scale)
            if scale == 1.0 and enc.dtype.kind in "iu":
                assert np.array_equal(_bits(got), _bits(enc.astype(out_np)))      # bit for bit the cast: how Quantize / AsType run


@pytest.mark.parametrize("out_np", [np.float32, np.float64], ids=["f32", "f64"])
def test_fso_decode_all_int16_values_in_float64_arithmetic(torch_cuda, out_np):
    """enc / 10.0 + 273.15 in float64, rounded once: float32 arithmetic gives other bits for a third of the int16 values."""
    enc = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    got = _fso(torch_cuda, enc, out_np, 10.0, 273.15)
    want = Z.fso_decode(enc, 10.0, 273.15, out_np)
    assert np.array_equal(_bits(got), _bits(want))
    if out_np == np.float32:
        shortcut = enc.astype(np.float32) / np.float32(10.0) + np.float32(273.15)
        assert (_bits(shortcut) != _bits(want)).mean() > 0.2                   # (the case does tell the two apart)


@pytest.mark.parametrize("name", ["int8", "int16", "uint16", "int32", "float32", "float64"])
def test_fso_decode_from_misaligned_starts(torch_cuda, name):
    enc = Z.type_code_arrays(np.random.default_rng(12), name, 1031)
    es = enc.dtype.itemsize
    for out_np in (np.float32, np.float64):
        for shift_src, shift_dst in ((es, 0), (0, np.dtype(out_np).itemsize), (es, np.dtype(out_np).itemsize)):
            got = _fso(torch_cuda, enc, out_np, 10.0, 273.15, shift_src, shift_dst)
            assert np.array_equal(_bits(got), _bits(Z.fso_decode(enc, 10.0, 273.15, out_np))), (name, shift_src, shift_dst)


def test_fso_decode_refusals_touch_nothing(torch_cuda):
    torch = torch_cuda
    lib = hip.load()
    swhole, src = _guarded(torch, 4096)
    dwhole, dst = _guarded(torch, 8192)
    src.fill_(0x11)
    dst.fill_(0x22)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = lambda s, d, n, st, dt_, scale=10.0: lib.afhip_fso_decode(C.c_void_p(s), C.c_void_p(d), n, st, dt_, scale, 1.0, stream)
    for args, why in [((src.data_ptr(), dst.data_ptr(), 16, 8, 6), "src_type"), ((src.data_ptr(), dst.data_ptr(), 16, -1, 6), "src_type"),
                      ((src.data_ptr(), dst.data_ptr(), 16, 2, 4), "dst_type"), ((src.data_ptr(), dst.data_ptr(), -1, 2, 6), "n < 0"),
                      ((src.data_ptr(), dst.data_ptr(), 16, 2, 6, 0.0), "scale"), ((src.data_ptr(), dst.data_ptr(), 16, 2, 6, float("nan")), "scale"),
                      ((src.data_ptr(), dst.data_ptr(), (1 << 31) * 256, 2, 6), "too many elements"),
                      ((src.data_ptr() + 1, dst.data_ptr(), 16, 2, 6), "element-aligned"), ((src.data_ptr(), dst.data_ptr() + 2, 16, 2, 6), "element-aligned"),
                      ((None, dst.data_ptr(), 16, 2, 6), "null"), ((dst.data_ptr(), dst.data_ptr() + 16, 16, 2, 6), "overlap")]:
        assert f(*args) == hip.E_INVALID, why
        assert why in lib.afhip_last_error().decode(), (why, lib.afhip_last_error().decode())
    with pytest.raises(ValueError, match="float32 or float64"):
        hip.fso_decode(src, dst, 16, "int16", 10.0, 0.0)                      # a uint8 destination
    with pytest.raises(ValueError, match="stored type"):
        hip.fso_decode(src, dst.view(torch.float32), 16, "int64", 10.0, 0.0)
    with pytest.raises(ValueError, match="do not fit"):
        hip.fso_decode(src, dst.view(torch.float32), 4096, "int16", 10.0, 0.0)
    torch.cuda.synchronize()
    assert bool((src == 0x11).all()) and bool((dst == 0x22).all())
    assert _guards_intact(swhole, 4096) and _guards_intact(dwhole, 8192)


# ---- stores ----
T, NY, NX = 72, 12, 16
CHUNKS = (10, 5, 7)                                  # edge chunks overhang the array on all three axes
BLOSC = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
ZLIB = {"id": "zlib", "level": 1}
ROUTES = [("0", BLOSC), ("1", BLOSC), ("1", ZLIB)]   # host-decoded scatter, Blosc-LZ4 decoded in HBM, zlib decoded in HBM
ROUTE_IDS = ["host-decode", "hbm-blosc-lz4", "hbm-zlib"]
# an interior box: with half a cell of slack the clip keeps latitude rows 3..8 and longitude columns 4..9
REGIONS = pd.DataFrame({"geoid": ["a", "b"], "minx": [12.0, 13.0], "miny": [31.6, 32.0], "maxx": [13.5, 14.4], "maxy": [33.0, 33.9]})
BOX = (3, 9, 4, 10)
FSO_I32 = {"id": "fixedscaleoffset", "scale": 1000.0, "offset": 273.15, "dtype": "<f8", "astype": "<i4"}
CHAINS = {
    "fso": (np.float32, [Z.FSO_I16]),
    "fso_delta": (np.float32, [Z.FSO_I16, Z.DELTA_I16]),
    "fso_u16": (np.float32, [{"id": "fixedscaleoffset", "scale": 8.0, "offset": -3000.0, "dtype": "<f4", "astype": "<u2"}]),
    "fso_i32_f64_delta": (np.float64, [FSO_I32, {"id": "delta", "dtype": "<i4", "astype": "<i4"}]),
    "fso_i8": (np.float32, [{"id": "fixedscaleoffset", "scale": 0.03125, "offset": 273.15, "dtype": "<f4", "astype": "<i1"}, {"id": "delta", "dtype": "<i1"}]),
    "fso_float_astype": (np.float64, [{"id": "fixedscaleoffset", "scale": 10.0, "offset": 273.15, "dtype": "<f8", "astype": "<f4"}]),
    "quantize": (np.float64, [{"id": "quantize", "digits": 1, "dtype": "<f8", "astype": "<f4"}]),
    "astype": (np.float32, [{"id": "astype", "encode_dtype": "<i2", "decode_dtype": "<f4"}]),
    "bitround": (np.float32, [{"id": "bitround", "keepbits": 9}]),
    # delta alone: running sums with no conversion behind them, placed straight into the cube (integers are read to float64 in HBM)
    "delta_i32": (np.int32, [{"id": "delta", "dtype": "<i4"}]),
    # ... and what the host undoes (`ZarrArray._chunk`), also with device=
    "fso_delta_shuffle": (np.float32, [Z.FSO_I16, Z.DELTA_I16, {"id": "shuffle", "elementsize": 2}]),
    "delta_narrowing": (np.int32, [{"id": "delta", "dtype": "<i4", "astype": "<i2"}]),
}
ON_HOST = ("fso_delta_shuffle", "delta_narrowing")
# `hip.fso_decode` calls of one read: the conversion of the whole cube; stored floats under Quantize are cast by torch (-0.0 stays -0.0)
FSO_CALLS = {"fso": 1, "fso_delta": 1, "fso_u16": 1, "fso_i32_f64_delta": 1, "fso_i8": 1, "fso_float_astype": 1, "quantize": 0, "astype": 1,
             "bitround": 0, "delta_i32": 0}
_FIELDS = {}


def _field(dtype):
    """One field per dtype, computed once and never written to: tenths around 273.15 K that cover the whole int16 range, so that
    the stored differences — and the running sums that undo them — wrap."""
    key = np.dtype(dtype).name
    if key not in _FIELDS:
        rng = np.random.default_rng(21)
        f = (273.15 + rng.uniform(-3276.0, 3276.0, size=(T, NY, NX))).astype(dtype)
        f[3, 2, 5] = -0.0 if key == "float64" else f[3, 2, 5]
        _FIELDS[key] = f
    return _FIELDS[key]


def _values(name):
    dtype, filters = CHAINS[name]
    if name == "astype":
        return np.round(_field(np.float64) - 273.15).astype(np.float32), filters
    if name == "delta_i32":                      # the whole range of int32: the stored differences and their running sums wrap
        return np.random.default_rng(22).integers(-2 ** 31, 2 ** 31, size=(T, NY, NX), dtype=np.int64).astype(np.int32), filters
    if name == "delta_narrowing":                # steps that fit the int16 they are stored as
        return np.cumsum(np.random.default_rng(23).integers(-9, 10, size=T * NY * NX)).reshape(T, NY, NX).astype(np.int32), filters
    return _field(dtype), filters


@pytest.fixture
def spies(monkeypatch):
    """Counts of the two kernels' calls and of the host's chunk decodes of the data variable."""
    seen = {"delta": 0, "fso": 0, "host_chunks": 0, "hbm_decodes": 0}
    real_delta, real_fso, real_chunk, real_route = hip.delta_decode, hip.fso_decode, afio.ZarrArray._chunk, afio._scatter_gpu_decode

    def route(*a, **k):
        seen["hbm_decodes"] += 1
        return real_route(*a, **k)

    def delta(*a, **k):
        seen["delta"] += 1
        return real_delta(*a, **k)

    def fso(*a, **k):
        seen["fso"] += 1
        return real_fso(*a, **k)

    def chunk(self, idx):
        if os.path.basename(self.path) == "t2m":
            seen["host_chunks"] += 1
        return real_chunk(self, idx)

    monkeypatch.setattr(hip, "delta_decode", delta)
    monkeypatch.setattr(hip, "fso_decode", fso)
    monkeypatch.setattr(afio.ZarrArray, "_chunk", chunk)
    monkeypatch.setattr(afio, "_scatter_gpu_decode", route)
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE_HOST_TAIL_MIN_MB", "0")      # the decode-in-HBM routes' host-decoded tail takes part
    return seen


def _same(t, want):
    got = t.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_device_read_equals_the_host_read(torch_cuda, tmp_path, monkeypatch, spies, name, route):
    mode, compressor = route
    values, filters = _values(name)
    path = str(tmp_path / "s.zarr")
    want, _ = Z.write_store(path, "t2m", values, CHUNKS, filters, compressor, absent={(1, 0, 1), (7, 2, 2)})
    host = af.dataset_from_path(path, "t2m").cube()
    np.testing.assert_array_equal(_bits(host), _bits(want))
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
    spies.update(delta=0, fso=0, host_chunks=0, hbm_decodes=0)
    ds = af.dataset_from_path(path, "t2m", device="cuda")
    assert ds.cube().is_cuda and not ds.is_packed
    # (integers become float64 in HBM, as on every streaming route: exact for int32; an absent chunk is the fill value 0)
    _same(ds.cube(), want.astype(np.float64) if want.dtype.kind == "i" else want)
    n_delta = sum(f["id"] == "delta" for f in filters)
    if name in ON_HOST:
        assert spies["host_chunks"] > 0 and spies["delta"] == spies["fso"] == 0
    else:
        assert spies["host_chunks"] == 0, "the host un-filtered the chunks"
        assert (spies["delta"] > 0) == (n_delta > 0)
        assert spies["fso"] == FSO_CALLS[name]
        assert spies["hbm_decodes"] == (1 if mode == "1" else 0)           # the chunks crossed PCIe compressed, as stored elements


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_cf_packed_int16_written_with_delta(torch_cuda, tmp_path, monkeypatch, spies, route):
    """An int16 CF-packed array under ``delta``: the running sums are the packed integers — unpacked to float32 in HBM like any packed
    store, or, with ``keep_packed``, the `PackedCube` itself."""
    mode, compressor = route
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
    rng = np.random.default_rng(24)
    stored = rng.integers(-32766, 32767, size=(T, NY, NX)).astype(np.int16)            # neighbours differ by more than int16 holds
    stored[rng.random((T, NY, NX)) < 0.02] = -32767
    attrs = {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}
    major, last = str(tmp_path / "major.zarr"), str(tmp_path / "last.zarr")
    absent = {(1, 0, 1), (7, 2, 2)}
    want, _ = Z.write_store(major, "t2m", stored, CHUNKS, [{"id": "delta", "dtype": "<i2"}], compressor, attrs=attrs, absent=absent)
    Z.write_store(last, "t2m", stored, CHUNKS, [{"id": "delta", "dtype": "<i2"}], compressor, attrs=attrs, absent=absent, time_last=True)
    assert want.dtype == np.int16 and (want[10:20, :5, 7:14] == 0).all()                # an absent chunk: the array's fill value, 0
    host = af.dataset_from_path(major, "t2m").cube()
    assert host.dtype == np.float32 and np.isnan(host).any()
    spies.update(delta=0, fso=0, host_chunks=0, hbm_decodes=0)
    for path in (major, last):
        d = af.dataset_from_path(path, "t2m", device="cuda")
        assert not d.is_packed
        _same(d.cube(), host)
        p = af.dataset_from_path(path, "t2m", device="cuda", keep_packed=True)
        assert p.is_packed and p.packed_cube().q.is_cuda
        np.testing.assert_array_equal(p.packed_cube().q.cpu().numpy().view(np.int16), want)
        w = af.dataset_from_path(path, "t2m", device="cuda", keep_packed=True, time_window=(13, 47))
        np.testing.assert_array_equal(w.packed_cube().q.cpu().numpy().view(np.int16), want[13:47])
    assert spies["delta"] > 0 and spies["fso"] == 0 and spies["host_chunks"] == 0
    assert spies["hbm_decodes"] == (6 if mode == "1" else 0)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_windows_time_last_and_keep_packed(torch_cuda, tmp_path, monkeypatch, spies, route):
    mode, compressor = route
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
    values, filters = _values("fso_delta")
    absent = {(1, 0, 1), (2, 1, 1)}
    major, last = str(tmp_path / "major.zarr"), str(tmp_path / "last.zarr")
    tdelta = [{"id": "delta", "dtype": "<i8", "astype": "<i8"}]            # the time coordinate as xarray writes it
    want, _ = Z.write_store(major, "t2m", values, CHUNKS, filters, compressor, absent=absent, time_filters=tdelta)
    want_last, _ = Z.write_store(last, "t2m", values, CHUNKS, filters, compressor, absent=absent, time_last=True, time_filters=tdelta)
    # (a time-last chunk is flattened in another order, so its stored differences differ; the wrapping sums give the same values back)
    np.testing.assert_array_equal(_bits(want), _bits(want_last))
    gr = af.GeoRegions(REGIONS)
    for path in (major, last):
        _same(af.dataset_from_path(path, "t2m", device="cuda").cube(), want)
        d = af.dataset_from_path(path, "t2m", device="cuda", time_window=(13, 47))
        assert len(d.time) == 34 and d.time[0] == pd.Timestamp("2001-01-01 13:00") and d.time[-1] == pd.Timestamp("2001-01-02 22:00")
        _same(d.cube(), want[13:47])
        d = af.dataset_from_path(path, "t2m", device="cuda", georegions=gr)
        _same(d.cube(), want[:, BOX[0]:BOX[1], BOX[2]:BOX[3]])
        d = af.dataset_from_path(path, "t2m", device="cuda", georegions=gr, time_window=(13, 47))
        _same(d.cube(), want[13:47, BOX[0]:BOX[1], BOX[2]:BOX[3]])
        d = af.dataset_from_path(path, "t2m", device="cuda", keep_packed=True)
        assert not d.is_packed and d.cube().dtype == torch_cuda.float32
        _same(d.cube(), want)
    assert spies["host_chunks"] == 0 and spies["delta"] > 0 and spies["fso"] == 10 and spies["hbm_decodes"] == (10 if mode == "1" else 0)


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_a_filtered_store_beside_a_plain_one(torch_cuda, tmp_path, monkeypatch, spies, route):
    mode, compressor = route
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
    values, filters = _values("fso_delta")
    a, b = str(tmp_path / "y2001a.zarr"), str(tmp_path / "y2001b.zarr")
    want_a, _ = Z.write_store(a, "t2m", values, CHUNKS, filters, compressor)
    want_b, _ = Z.write_store(b, "t2m", values[::-1].copy(), CHUNKS, None, compressor, start_hour=T)
    d = af.dataset_from_path([a, b], "t2m", device="cuda")
    assert len(d.time) == 2 * T
    _same(d.cube(), np.concatenate([want_a, want_b]))
    _same(af.dataset_from_path(str(tmp_path / "y2001*.zarr"), "t2m", device="cuda").cube(), np.concatenate([want_a, want_b]))
    np.testing.assert_array_equal(_bits(af.dataset_from_path([a, b], "t2m").cube()), _bits(np.concatenate([want_a, want_b])))


def test_cf_attributes_on_top_of_a_filter_in_hbm(torch_cuda, tmp_path, monkeypatch, spies):
    values, filters = _values("fso_delta")
    path = str(tmp_path / "cf.zarr")
    fill = float(Z.fso_decode(np.array([100], dtype=np.int16), 10.0, 273.15, np.float32)[0])
    Z.write_store(path, "t2m", values, CHUNKS, filters, ZLIB, attrs={"scale_factor": 0.5, "add_offset": 10.0, "_FillValue": fill})
    host = af.dataset_from_path(path, "t2m").cube()
    for mode in ("0", "1"):
        monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
        _same(af.dataset_from_path(path, "t2m", device="cuda").cube(), host)
    assert spies["fso"] == 2                                        # (one conversion per device read)


def test_aggregate_on_a_filtered_store_equals_the_float_store(torch_cuda, tmp_path, spies):
    values, filters = _values("fso_delta")
    filtered, plain = str(tmp_path / "f.zarr"), str(tmp_path / "p.zarr")
    want, _ = Z.write_store(filtered, "t2m", values, CHUNKS, filters, BLOSC)
    Z.write_store(plain, "t2m", want, CHUNKS, None, BLOSC)                # the decoded values, as float32
    tab = synth.weights_table(NY, NX, 6, seed=62, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}))
    spec = dict(dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": "date"})],
                t=[("aggregate", {"calc": "mean", "groupby": "date"}), ("aggregate", {"calc": "sum", "groupby": "date"})])
    frames = []
    for path in (filtered, plain):
        d = af.dataset_from_path(path, "t2m", lon_is_360=True, device="cuda")
        frames.append(af.aggregate_dataset(dataset=d, weights=af.weights_from_objects(d, gr, table=tab), aggregator_dict=spec))
    assert len(frames[0]) > 0 and spies["fso"] == 1
    pd.testing.assert_frame_equal(frames[0], frames[1], check_exact=True)


def test_store_sharded_and_cell_sharded_aggregation_of_a_filtered_store(torch_cuda, tmp_path, spies):
    from aggfly_amd import distributed as D, engine as eng
    values, filters = _values("fso_delta")
    path = str(tmp_path / "f.zarr")
    Z.write_store(path, "t2m", values, CHUNKS, filters, BLOSC)
    tab = synth.weights_table(NY, NX, 6, seed=62, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}))
    spec = dict(t=[("aggregate", {"calc": "mean", "groupby": "date"}), ("aggregate", {"calc": "sum", "groupby": "date"})])
    weights_of = lambda d: af.weights_from_objects(d, gr, table=tab)
    old = eng.config.exact_order
    try:
        eng.config.exact_order = True                  # no period is split, so a period's sums do not depend on its window
        whole = af.dataset_from_path(path, "t2m", lon_is_360=True, device="cuda")
        want = af.aggregate_dataset(dataset=whole, weights=weights_of(whole), aggregator_dict=spec)
        assert D._step_bytes(path, "t2m") == NY * NX * (4 + 2)
        got = D.aggregate_store_sharded(weights_of, path, "t2m", spec, lon_is_360=True, max_window_bytes=24 * D._step_bytes(path, "t2m"))
        pd.testing.assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True))
        cells = D.aggregate_store_cells(weights_of, path, "t2m", spec, lon_is_360=True)
        pd.testing.assert_frame_equal(cells.reset_index(drop=True), want.reset_index(drop=True))
    finally:
        eng.config.exact_order = old
    assert spies["fso"] >= 4 and spies["host_chunks"] == 0           # the whole read, three daily windows at least, the band
