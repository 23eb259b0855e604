"""numcodecs element filters restated in plain numpy, and a writer of Zarr format-2 stores that use them — what the filter tests
(`test_zarr_filters_host.py`, `test_gpu_zarr_filters.py`) expect.  Nothing here calls the package's reader, its `filter_elements` /
`unfilter_elements` or its `_write_array`: the formulas are numcodecs' documented ones (FixedScaleOffset, Delta, Quantize, BitRound,
AsType, Shuffle), written down a second time.  numcodecs itself is not available, so parity with a store it wrote is not checked.

A filter chain is a list of numcodecs configs in WRITE order; the compressor follows the last one.
"""
import json
import os
import zlib

import numpy as np

TYPE_NAMES = ("int8", "uint8", "int16", "uint16", "int32", "uint32", "float32", "float64")


# ---- one filter, both ways ----
def fso_encode(x, scale, offset, astype):
    return np.around((np.asarray(x) - offset) * scale).astype(astype)


def fso_decode(enc, scale, offset, dtype):
    """``enc / scale + offset``: numpy divides an integer array by a float in float64 and a float array in its own type."""
    enc = np.asarray(enc)
    if enc.dtype.kind in "iu":
        return (enc.astype(np.float64) / np.float64(scale) + np.float64(offset)).astype(dtype)
    t = enc.dtype.type
    return (enc / t(scale) + t(offset)).astype(dtype)


def delta_encode(x, astype):
    x = np.asarray(x).reshape(-1).astype(astype)
    out = np.empty_like(x)
    out[0] = x[0]
    out[1:] = x[1:] - x[:-1]                # (integers wrap)
    return out


def delta_decode(enc, dtype):
    """A running sum over the flattened chunk in ``dtype``, one element after the other (integers wrap)."""
    enc = np.asarray(enc).reshape(-1).astype(dtype)
    out = np.empty_like(enc)
    acc = enc.dtype.type(0)
    with np.errstate(over="ignore"):
        for i, v in enumerate(enc):
            acc = enc.dtype.type(acc + v)
            out[i] = acc
    return out


def delta_decode_fast(enc, dtype):
    """`delta_decode` for long chunks: the same wrapping sum through unsigned 64-bit arithmetic (integers only)."""
    dtype = np.dtype(dtype)
    assert dtype.kind in "iu"
    wide = np.cumsum(np.asarray(enc).reshape(-1).astype(dtype).astype(np.int64).view(np.uint64), dtype=np.uint64)
    return wide.astype(np.dtype(f"u{dtype.itemsize}")).view(dtype)


def quantize_encode(x, digits, astype):
    exp = np.log10(10.0 ** -digits)
    exp = int(np.floor(exp)) if exp < 0 else int(np.ceil(exp))
    scale = 2.0 ** int(np.ceil(np.log2(10.0 ** -exp)))
    return (np.around(scale * np.asarray(x)) / scale).astype(astype)


def bitround_encode(x, keepbits):
    x = np.asarray(x)
    bits = {4: 23, 8: 52}[x.dtype.itemsize]
    u = x.view(f"u{x.dtype.itemsize}").copy()
    drop = bits - keepbits
    if drop > 0:
        one = u.dtype.type(1)
        half = (one << u.dtype.type(drop - 1)) - one
        u += half + ((u >> u.dtype.type(drop)) & one)          # round to nearest, ties to even
        u &= ~((one << u.dtype.type(drop)) - one)
    return u.view(x.dtype)


def shuffle_encode(raw: bytes, elementsize: int) -> bytes:
    b = np.frombuffer(raw, dtype=np.uint8)
    n = len(b) // elementsize
    return np.concatenate([b[:n * elementsize].reshape(n, elementsize).T.reshape(-1), b[n * elementsize:]]).tobytes()


# ---- a chain ----
def encode_chain(values, filters):
    """The flattened values of one chunk -> the bytes the compressor is given."""
    x = np.asarray(values).reshape(-1)
    raw = None
    for f in filters:
        if f["id"] == "shuffle":
            raw = shuffle_encode(x.tobytes() if raw is None else raw, int(f["elementsize"]))
            continue
        assert raw is None, "element filters come before the shuffle"
        if f["id"] == "fixedscaleoffset":
            x = fso_encode(x.astype(f["dtype"]), f["scale"], f["offset"], f["astype"])
        elif f["id"] == "delta":
            x = delta_encode(x, f.get("astype") or f["dtype"])
        elif f["id"] == "quantize":
            x = quantize_encode(x.astype(f["dtype"]), f["digits"], f["astype"])
        elif f["id"] == "bitround":
            x = bitround_encode(x, f["keepbits"])
        elif f["id"] == "astype":
            x = x.astype(f["encode_dtype"])
        else:
            raise AssertionError(f["id"])
    return (x.tobytes() if raw is None else raw), x


def decode_stored(stored, filters):
    """The stored elements of one chunk (after the compressor and the byte shuffle are undone) -> its values."""
    x = np.asarray(stored).reshape(-1)
    for f in reversed([f for f in filters if f["id"] not in ("shuffle", "bitround")]):
        if f["id"] == "fixedscaleoffset":
            x = fso_decode(x, f["scale"], f["offset"], f["dtype"])
        elif f["id"] == "delta":
            d = np.dtype(f["dtype"])
            x = delta_decode_fast(x, d) if d.kind in "iu" else delta_decode(x, d)
        elif f["id"] == "quantize":
            x = x.astype(f["dtype"])
        elif f["id"] == "astype":
            x = x.astype(f["decode_dtype"])
    return x


def type_code_arrays(rng, name, n):
    """``n`` stored values of numpy type ``name`` that cover its range (and, for floats, signed zeros and large magnitudes)."""
    dt = np.dtype(name)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        x = rng.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64).astype(dt)
        x[:4] = np.array([info.min, info.max, 0, 1]).astype(dt)[:min(4, n)]
        return x
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, size=n)).astype(dt)
    x[:3] = np.array([0.0, -0.0, 1.0], dtype=dt)[:min(3, n)]
    return x


# ---- a store ----
def _compress(raw: bytes, compressor, typesize: int) -> bytes:
    if compressor is None:
        return raw
    if compressor["id"] == "zlib":
        return zlib.compress(raw, compressor.get("level", 1))
    if compressor["id"] == "blosc":                        # (the compressor is not what these tests are about: the package's encoder)
        from aggfly_amd import codec
        return codec.blosc_encode(np.frombuffer(raw, dtype=np.uint8), typesize, shuffle=compressor.get("shuffle", 1) == 1,
                                  blocksize=compressor.get("blocksize", 0), cname=compressor.get("cname", "lz4"))
    raise AssertionError(compressor)


def write_array(path, name, values, dims, chunks, filters=None, compressor=None, attrs=None, absent=(), fill_value=None):
    """A format-2 array written chunk by chunk through `encode_chain` -> the values a reader must give: every chunk's
    `decode_stored` of what was stored (the filters may be lossy), the fill value where a chunk of ``absent`` is left out."""
    values = np.ascontiguousarray(values)
    d = os.path.join(path, name)
    os.makedirs(d, exist_ok=True)
    filters = list(filters or [])
    if fill_value is None:
        fill_value = "NaN" if values.dtype.kind == "f" else 0
    with open(os.path.join(d, ".zarray"), "w") as f:
        json.dump({"zarr_format": 2, "shape": list(values.shape), "chunks": list(chunks), "dtype": values.dtype.str,
                   "compressor": compressor, "fill_value": fill_value, "order": "C", "filters": filters or None}, f)
    with open(os.path.join(d, ".zattrs"), "w") as f:
        json.dump(dict(attrs or {}, _ARRAY_DIMENSIONS=list(dims)), f)
    want = np.empty_like(values)
    fill = np.nan if fill_value == "NaN" else fill_value
    for idx in np.ndindex(*[-(-s // c) for s, c in zip(values.shape, chunks)]):
        sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, values.shape))
        part = values[sl]
        if tuple(idx) in absent:
            want[sl] = fill
            continue
        blk = np.zeros(chunks, dtype=values.dtype)           # an edge chunk overhangs the array: padded (with zeros)
        blk[tuple(slice(0, n) for n in part.shape)] = part
        raw, stored = encode_chain(blk, filters)
        with open(os.path.join(d, ".".join(str(i) for i in idx)), "wb") as f:
            f.write(_compress(raw, compressor, stored.dtype.itemsize))
        back = decode_stored(stored, filters).reshape(chunks)
        want[sl] = back[tuple(slice(0, n) for n in part.shape)]
    return want


def write_store(path, var, values, chunks, filters=None, compressor=None, attrs=None, absent=(), time_filters=None, time_last=False,
                start_hour=0, fill_value=None):
    """A store `dataset_from_path` opens: ``values`` is (time, latitude, longitude); ``time_last`` writes it (latitude, longitude,
    time) with ``chunks`` reordered alike.  The time coordinate is int64 hours since 2001-01-01, under ``time_filters`` if given (xarray
    writes it with ``delta``).  -> (the data variable's expected values, time-major; hours)"""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, ".zgroup"), "w") as f:
        json.dump({"zarr_format": 2}, f)
    T, ny, nx = values.shape
    if time_last:
        want = write_array(path, var, values.transpose(1, 2, 0), ("latitude", "longitude", "time"), (chunks[1], chunks[2], chunks[0]), filters,
                           compressor, attrs, {(a[1], a[2], a[0]) for a in absent}, fill_value).transpose(2, 0, 1)
    else:
        want = write_array(path, var, values, ("time", "latitude", "longitude"), chunks, filters, compressor, attrs, set(absent), fill_value)
    hours = np.arange(start_hour, start_hour + T, dtype=np.int64)
    got = write_array(path, "time", hours, ("time",), (T,), time_filters, None, {"units": "hours since 2001-01-01", "calendar": "standard"})
    assert np.array_equal(got, hours)
    write_array(path, "latitude", 30 + 0.5 * np.arange(ny), ("latitude",), (ny,))
    write_array(path, "longitude", 10 + 0.5 * np.arange(nx), ("longitude",), (nx,))
    return want, hours


FSO_I16 = {"id": "fixedscaleoffset", "scale": 10.0, "offset": 273.15, "dtype": "<f4", "astype": "<i2"}
DELTA_I16 = {"id": "delta", "dtype": "<i2", "astype": "<i2"}
