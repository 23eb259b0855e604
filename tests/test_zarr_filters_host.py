"""Zarr format-2 stores written with numcodecs element filters (FixedScaleOffset, Delta, Quantize, BitRound, AsType), read on the
host: `ZarrArray`'s stored type and filter chain, `open_zarr` / `dataset_from_path` bit for bit against the restatement of
`tests/zarr_filter_cases.py`, the hand-built chunks of `tests/golden/zarr_filter_known_chunks.json`, every refusal with its reason,
and the writer's ``filters=``."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from zarr_filter_cases import DELTA_I16, FSO_I16, decode_stored, encode_chain, write_store  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import distributed as D, hip, io as afio  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "zarr_filter_known_chunks.json")) as _f:
    GOLDEN = json.load(_f)["chunks"]

T, NY, NX = 23, 9, 13
CHUNKS = (10, 4, 5)                                   # edge chunks overhang the array on all three axes
BLOSC = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}
ZLIB = {"id": "zlib", "level": 1}


def field(dtype=np.float32, seed=1, spread=3276.0):
    """Temperatures whose tenths cover the whole int16 range around 273.15 K: neighbours differ by more than int16 holds, so the
    differences ``delta`` stores wrap, and so do the running sums that undo them."""
    rng = np.random.default_rng(seed)
    return (273.15 + rng.uniform(-spread, spread, size=(T, NY, NX))).astype(dtype)


CHAINS = {
    "fso": (np.float32, [FSO_I16]),
    "fso_delta": (np.float32, [FSO_I16, DELTA_I16]),
    "fso_delta_shuffle": (np.float32, [FSO_I16, DELTA_I16, {"id": "shuffle", "elementsize": 2}]),
    "fso_u16": (np.float32, [{"id": "fixedscaleoffset", "scale": 8.0, "offset": -3000.0, "dtype": "<f4", "astype": "<u2"}]),
    "fso_i32_f64": (np.float64, [{"id": "fixedscaleoffset", "scale": 1000.0, "offset": 273.15, "dtype": "<f8", "astype": "<i4"},
                                 {"id": "delta", "dtype": "<i4", "astype": "<i4"}]),
    "fso_float_astype": (np.float64, [{"id": "fixedscaleoffset", "scale": 10.0, "offset": 273.15, "dtype": "<f8", "astype": "<f4"}]),
    "delta_i32": (np.int32, [{"id": "delta", "dtype": "<i4"}]),
    "delta_narrowing": (np.int32, [{"id": "delta", "dtype": "<i4", "astype": "<i2"}]),
    "quantize": (np.float64, [{"id": "quantize", "digits": 1, "dtype": "<f8", "astype": "<f4"}]),
    "astype": (np.float32, [{"id": "astype", "encode_dtype": "<i2", "decode_dtype": "<f4"}]),
    "bitround": (np.float32, [{"id": "bitround", "keepbits": 9}]),
}


def values_for(name):
    dtype, filters = CHAINS[name]
    if name == "astype":
        return np.round(field(np.float64) - 273.15).astype(np.float32), filters       # whole numbers inside int16
    if name in ("delta_narrowing", "delta_i32"):
        return np.cumsum(np.random.default_rng(4).integers(-9, 10, size=(T, NY, NX)), axis=None).reshape(T, NY, NX).astype(np.int32), filters
    return field(dtype), filters


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    return np.array_equal(a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}"))


@pytest.mark.parametrize("compressor", [None, ZLIB, BLOSC], ids=["raw", "zlib", "blosc"])
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_every_chain_reads_bit_for_bit(tmp_path, name, compressor):
    values, filters = values_for(name)
    path = str(tmp_path / "s.zarr")
    want, hours = write_store(path, "t2m", values, CHUNKS, filters, compressor, absent={(1, 0, 1)})
    za = afio.ZarrArray(os.path.join(path, "t2m"))
    stored = encode_chain(values[:1], [f for f in filters if f["id"] != "shuffle"])[1].dtype      # what the compressor was given
    assert za.dtype == values.dtype and za.stored_dtype == stored
    assert za.chunk_nbytes == int(np.prod(CHUNKS)) * stored.itemsize
    # the compressor alone decides the kind; a byte shuffle in the chain keeps the host route, as before
    assert za.native_kind == (None if name == "fso_delta_shuffle" else "raw" if compressor is None else compressor["id"])
    assert same_bits(za.read(), want)
    da = afio.open_zarr(path, "t2m")
    assert same_bits(da.values, want)
    ds = af.dataset_from_path(path, "t2m")
    assert same_bits(ds.cube(), want)
    assert len(ds.time) == T and ds.time[0] == np.datetime64("2001-01-01")
    if name == "fso_delta":
        assert len(np.unique(encode_chain(values[:10, :4, :5], filters)[1])) > 100          # (the stored differences do span int16)


def test_int16_running_sums_wrap(tmp_path):
    values, filters = values_for("fso_delta")
    _, stored = encode_chain(values[:10, :4, :5], filters)
    wide = np.cumsum(stored.astype(np.int64))
    assert (np.abs(wide) > 32767).any()                      # a sum in wider arithmetic leaves int16: the int16 sum wraps
    assert np.array_equal(decode_stored(stored, filters[1:]), wide.astype(np.int16))


def test_absent_chunk_is_the_fill_value_in_the_decoded_type(tmp_path):
    values, filters = values_for("fso_delta")
    path = str(tmp_path / "s.zarr")
    want, _ = write_store(path, "t2m", values, CHUNKS, filters, ZLIB, absent={(0, 1, 1)}, fill_value=-1.5)
    got = afio.ZarrArray(os.path.join(path, "t2m")).read()
    assert (got[:10, 4:8, 5:10] == np.float32(-1.5)).all() and same_bits(got, want)


def test_delta_time_coordinate_loads(tmp_path):
    values, filters = values_for("fso")
    path = str(tmp_path / "s.zarr")
    write_store(path, "t2m", values, CHUNKS, filters, ZLIB, time_filters=[{"id": "delta", "dtype": "<i8", "astype": "<i8"}], start_hour=17)
    want = np.datetime64("2001-01-01T17") + np.arange(T) * np.timedelta64(1, "h")
    assert np.array_equal(afio.read_time_coordinate(path, "t2m").values, want.astype("datetime64[ns]"))
    assert np.array_equal(af.dataset_from_path(path, "t2m").time.values, want.astype("datetime64[ns]"))


def test_cf_attributes_apply_on_top_of_a_filter(tmp_path):
    values, filters = values_for("fso")
    path = str(tmp_path / "s.zarr")
    attrs = {"scale_factor": 0.5, "add_offset": 10.0, "_FillValue": float(np.float32(273.15))}
    want, _ = write_store(path, "t2m", values, CHUNKS, filters, ZLIB, attrs=attrs)
    want[0, 0, 0] = np.float32(273.15)                     # a value that is the CF fill
    za = afio.ZarrArray(os.path.join(path, "t2m"))
    raw = za.read()
    hit = raw == np.float32(273.15)
    cf = raw.copy()
    cf[hit] = np.nan
    cf *= 0.5
    cf += 10.0
    assert same_bits(afio.open_zarr(path, "t2m").values, cf)


def test_step_bytes_count_the_stored_elements_beside_the_cube(tmp_path):
    values, filters = values_for("fso_delta")
    path = str(tmp_path / "s.zarr")
    write_store(path, "t2m", values, CHUNKS, filters, None)
    assert D._step_bytes(path, "t2m") == NY * NX * (4 + 2)
    plain = str(tmp_path / "p.zarr")
    write_store(plain, "t2m", values, CHUNKS, None, None)
    assert D._step_bytes(plain, "t2m") == NY * NX * 4


@pytest.mark.parametrize("rec", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden_chunks_decode_to_their_recorded_bits(tmp_path, rec):
    d = tmp_path / "g.zarr" / "v"
    os.makedirs(d)
    with open(d / ".zarray", "w") as f:
        json.dump({"zarr_format": 2, "shape": rec["shape"], "chunks": rec["shape"], "dtype": rec["dtype"], "compressor": None,
                   "fill_value": 0, "order": "C", "filters": rec["filters"]}, f)
    with open(d / ".".join("0" for _ in rec["shape"]), "wb") as f:
        f.write(bytes.fromhex(rec["stored"]))
    got = afio.ZarrArray(str(d)).read()
    assert got.dtype == np.dtype(rec["dtype"]) and list(got.shape) == rec["shape"]
    assert got.tobytes().hex() == rec["decoded"]
    # ... and the restatement agrees with the hand-built bits
    za = afio.ZarrArray(str(d))
    stored = np.frombuffer(bytes.fromhex(rec["stored"]), dtype=za.stored_dtype)
    assert decode_stored(stored, rec["filters"]).astype(rec["dtype"]).tobytes().hex() == rec["decoded"]


def _zarray(tmp_path, dtype, filters, shape=(8,)):
    d = tmp_path / "r.zarr" / "v"
    os.makedirs(d, exist_ok=True)
    with open(d / ".zarray", "w") as f:
        json.dump({"zarr_format": 2, "shape": list(shape), "chunks": list(shape), "dtype": dtype, "compressor": None, "fill_value": 0,
                   "order": "C", "filters": filters}, f)
    return str(d)


@pytest.mark.parametrize("dtype,filters,reason", [
    ("<f4", [{"id": "packbits"}], r"'packbits' is not supported"),
    ("<f8", [FSO_I16], r"decodes to <f4, but the array's dtype is <f8.*do not connect"),
    ("<f4", [FSO_I16, {"id": "delta", "dtype": "<i4", "astype": "<i4"}], r"decodes to <i4, but astype of filter 0 \('fixedscaleoffset'\) is <i2.*do not connect"),
    ("<f4", [{"id": "fixedscaleoffset", "scale": 10.0, "offset": 0.0, "dtype": "<f4", "astype": ">i2"}], r"big-endian type >i2"),
    (">f4", [{"id": "fixedscaleoffset", "scale": 10.0, "offset": 0.0, "dtype": ">f4", "astype": "<i2"}], r"big-endian type >f4"),
    ("<c16", [{"id": "astype", "encode_dtype": "<c8", "decode_dtype": "<c16"}], r"type <c16 is not supported \(integers and floats of 1, 2, 4 or 8 bytes"),
    ("<f4", [{"id": "shuffle", "elementsize": 2}, FSO_I16], r"follows a byte shuffle"),
    ("<i4", [{"id": "bitround", "keepbits": 3}], r"'bitround' on int32 data"),
    ("<f4", [{"id": "delta", "dtype": "<f4", "astype": "<f4"}], r"'delta' on floating-point data \(<f4\) is not supported"),
    ("<f8", [{"id": "delta", "dtype": "<f8"}], r"'delta' on floating-point data \(<f8\) is not supported"),
])
def test_refusals_name_their_reason(tmp_path, dtype, filters, reason):
    with pytest.raises(ValueError, match=reason):
        afio.ZarrArray(_zarray(tmp_path, dtype, filters))


def test_format_3_is_left_as_it_is(tmp_path):
    d = tmp_path / "v3" / "v"
    os.makedirs(d)
    with open(d / "zarr.json", "w") as f:
        json.dump({"zarr_format": 3, "node_type": "array", "shape": [4], "data_type": "float32",
                   "chunk_grid": {"name": "regular", "configuration": {"chunk_shape": [4]}}, "fill_value": 0,
                   "codecs": [{"name": "bytes", "configuration": {"endian": "little"}}, {"name": "delta"}]}, f)
    with pytest.raises(ValueError, match="unsupported Zarr v3 codec 'delta'"):
        afio.ZarrArray(str(d))


# ---- the chains that are undone in HBM, and those the host keeps ----
def test_which_chains_the_device_takes(tmp_path):
    taken = {"fso": (0, ("fso", 10.0, 273.15)), "fso_delta": (1, ("fso", 10.0, 273.15)), "fso_u16": (0, ("fso", 8.0, -3000.0)),
             "fso_i32_f64": (1, ("fso", 1000.0, 273.15)), "fso_float_astype": (0, ("fso", 10.0, 273.15)), "quantize": (0, ("cast",)),
             "astype": (0, ("cast",)), "bitround": None, "delta_i32": (1, None)}
    for name in sorted(CHAINS):
        values, filters = values_for(name)
        path = str(tmp_path / f"{name}.zarr")
        write_store(path, "t2m", values, CHUNKS, filters, ZLIB)
        za = afio.ZarrArray(os.path.join(path, "t2m"))
        plan = afio._hbm_filter_plan(za)
        if name in taken:
            assert plan == taken[name], name
            assert za.native_kind == za.scatter_kind == "zlib"
        else:                                                # a narrowing delta, a chain with the byte shuffle
            assert plan is None and za.scatter_kind is None, name
    assert afio.packing_of(afio.ZarrArray(os.path.join(str(tmp_path / "fso.zarr"), "t2m"))) is None      # float in HBM: never a PackedCube


def test_library_declares_the_filter_entries():
    assert {"afhip_delta_scratch_bytes", "afhip_delta_decode", "afhip_fso_decode"} <= set(hip.EXPORTS)
    with open(os.path.join(ROOT, "include", "aggfly_hip.h")) as f:
        header = f.read()
    for name in ("afhip_delta_scratch_bytes", "afhip_delta_decode", "afhip_fso_decode"):
        assert f" {name}(" in header
    codes = dict(I8=0, U8=1, I16=2, U16=3, I32=4, U32=5, F32=6, F64=7)
    for k, v in codes.items():
        assert f"AFHIP_T_{k} = {v}" in header
    assert hip.FSO_TYPE == {"int8": 0, "uint8": 1, "int16": 2, "uint16": 3, "int32": 4, "uint32": 5, "float32": 6, "float64": 7}
    assert "#define AFHIP_ABI_VERSION 4" in header


# ---- the writer ----
def _ds(values):
    import pandas as pd
    time = pd.date_range("2001-01-01", periods=values.shape[0], freq="h")
    return af.Dataset(af.DataArray(values, ["time", "latitude", "longitude"],
                                   {"time": time, "latitude": 30 + 0.5 * np.arange(values.shape[1]), "longitude": 10 + 0.5 * np.arange(values.shape[2])}),
                      lon_is_360=True)


def _tree(path):
    out = {}
    for d, _, files in os.walk(path):
        for f in files:
            with open(os.path.join(d, f), "rb") as h:
                out[os.path.relpath(os.path.join(d, f), path)] = h.read()
    return out


@pytest.mark.parametrize("compress", [True, "zlib", False])
def test_writer_round_trips(tmp_path, compress):
    values, filters = values_for("fso_delta")
    path = str(tmp_path / "w.zarr")
    af.dataset_to_zarr(_ds(values), path, var="t2m", chunks={"time": 10, "latitude": 4, "longitude": 5}, compress=compress, filters=filters)
    with open(os.path.join(path, "t2m", ".zarray")) as f:
        meta = json.load(f)
    assert meta["filters"] == filters and meta["dtype"] == "<f4"
    back = af.dataset_from_path(path, "t2m").cube()
    want = np.empty_like(values)
    for t0 in range(0, T, 10):
        for y0 in range(0, NY, 4):
            for x0 in range(0, NX, 5):
                part = values[t0:t0 + 10, y0:y0 + 4, x0:x0 + 5]
                blk = np.zeros(CHUNKS, dtype=values.dtype)      # (the padding's stored integers precede nothing that is read back ...
                blk[:part.shape[0], :part.shape[1], :part.shape[2]] = part
                # ... only along the fastest axes do they enter a running sum before real cells; the sum wraps back exactly)
                full = np.full(CHUNKS, np.nan, dtype=values.dtype)
                full[:part.shape[0], :part.shape[1], :part.shape[2]] = part
                with np.errstate(invalid="ignore"):
                    stored = encode_chain(full, filters)[1]
                dec = decode_stored(stored, filters).reshape(CHUNKS)
                want[t0:t0 + 10, y0:y0 + 4, x0:x0 + 5] = dec[:part.shape[0], :part.shape[1], :part.shape[2]]
    assert same_bits(back, want)
    assert np.abs(back - values).max() <= 0.05 + 1e-3              # a tenth of a kelvin, rounded to nearest


def test_writer_writes_the_golden_bytes(tmp_path):
    rec = next(c for c in GOLDEN if c["name"] == "fso_delta_i16_wrapping")
    values = np.frombuffer(bytes.fromhex(rec["decoded"]), dtype="<f4").reshape(rec["shape"])
    path = str(tmp_path / "g.zarr")
    af.dataset_to_zarr(_ds(values), path, var="t2m", chunks={"time": 4, "latitude": 2, "longitude": 3}, compress=False, filters=rec["filters"])
    with open(os.path.join(path, "t2m", "0.0.0"), "rb") as f:
        assert f.read().hex() == rec["stored"]


def test_writer_refusals(tmp_path):
    values, filters = values_for("fso_delta")
    with pytest.raises(ValueError, match="format-2"):
        af.dataset_to_zarr(_ds(values), str(tmp_path / "a.zarr"), var="t2m", zarr_format=3, filters=filters)
    with pytest.raises(ValueError, match="filters"):
        af.dataset_to_zarr(_ds(values), str(tmp_path / "b.zarr"), var="t2m", encode="gpu", filters=filters)
    with pytest.raises(ValueError, match="do not connect"):
        af.dataset_to_zarr(_ds(values.astype(np.float64)), str(tmp_path / "c.zarr"), var="t2m", filters=filters)


@pytest.mark.parametrize("fmt", [2, 3])
@pytest.mark.parametrize("compress", [True, "zlib", False])
def test_filters_none_or_empty_write_what_a_call_without_the_keyword_writes(tmp_path, fmt, compress):
    values = field()
    a, b, c = (str(tmp_path / n) for n in ("a.zarr", "b.zarr", "c.zarr"))
    kw = dict(var="t2m", chunks={"time": 10, "latitude": 4, "longitude": 5}, compress=compress, zarr_format=fmt)
    af.dataset_to_zarr(_ds(values), a, **kw)
    af.dataset_to_zarr(_ds(values), b, filters=None, **kw)
    af.dataset_to_zarr(_ds(values), c, filters=[], **kw)
    ta, tb, tc = _tree(a), _tree(b), _tree(c)
    assert ta.keys() == tb.keys() == tc.keys() and len(ta) > 4
    assert all(ta[k] == tb[k] == tc[k] for k in ta)
    if fmt == 2:                                             # the metadata as it stood before ``filters=``: key for key
        assert json.loads(ta[os.path.join("t2m", ".zarray")]) == {
            "zarr_format": 2, "shape": [T, NY, NX], "chunks": [10, 4, 5], "dtype": "<f4", "fill_value": "NaN", "order": "C", "filters": None,
            "compressor": {True: BLOSC, "zlib": ZLIB, False: None}[compress]}
        assert list(json.loads(ta[os.path.join("t2m", ".zarray")])) == ["zarr_format", "shape", "chunks", "dtype", "compressor", "fill_value", "order", "filters"]
