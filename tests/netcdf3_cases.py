"""A small catalogue of NetCDF classic files (CDF-1 / CDF-2) for tests/test_netcdf3.py and tests/test_gpu_netcdf3.py, with its own
writer — from "The NetCDF Classic Format Specification" (NetCDF User's Guide, appendix C), independent of aggfly_amd/netcdf3.py
and of scipy.  Every case keeps the arrays (native byte order) and attributes it wrote.

    header = 'C' 'D' 'F' version  numrecs  dim_list  gatt_list  var_list            everything big-endian
    dim    = name length (0: the record dimension)      name = count bytes pad-to-4
    attr   = name type count values pad-to-4            var  = name rank dimids att_list type vsize begin (4 bytes; 8 in CDF-2)

Fixed variables follow the header, each padded to 4 bytes; then ``numrecs`` records, each one step of every record variable,
padded to 4 bytes each — unless the file has exactly one record variable, whose steps then follow each other unpadded.
"""
import os
import struct

import numpy as np

NC_TYPE = {"i1": 1, "S1": 2, "i2": 3, "i4": 4, "f4": 5, "f8": 6}
HOURS = "hours since 1900-01-01 00:00:00.0"


def _pad(b: bytes) -> bytes:
    return b + b"\x00" * (-len(b) % 4)


def _name(s: str) -> bytes:
    b = s.encode()
    return struct.pack(">I", len(b)) + _pad(b)


def _attr_values(v):
    """(type code, count, padded bytes) of an attribute value: str -> char, numpy scalars / arrays by dtype, float -> double, int -> int."""
    if isinstance(v, str):
        b = v.encode()
        return 2, len(b), _pad(b)
    a = np.atleast_1d(np.asarray(v))
    if a.dtype == np.int64:
        a = a.astype(np.int32)
    key = a.dtype.str[1:]
    return NC_TYPE[key], a.size, _pad(a.astype(a.dtype.newbyteorder(">")).tobytes())


def _att_list(attrs: dict) -> bytes:
    if not attrs:
        return struct.pack(">II", 0, 0)
    out = struct.pack(">II", 0x0C, len(attrs))
    for k, v in attrs.items():
        code, n, raw = _attr_values(v)
        out += _name(k) + struct.pack(">II", code, n) + raw
    return out


def write_classic(path, version, dims, variables, numrecs, gattrs=None):
    """``dims``: [(name, length or None for the record dimension)]; ``variables``: [(name, dim names, attrs, array)] in file order.
    A record variable's array has ``numrecs`` leading steps."""
    dimnames = [d for d, _ in dims]
    recdim = next((d for d, n in dims if n is None), None)
    off_fmt = ">I" if version == 1 else ">Q"

    def header(begins):
        h = b"CDF" + bytes([version]) + struct.pack(">I", numrecs)
        h += struct.pack(">II", 0x0A, len(dims)) if dims else struct.pack(">II", 0, 0)
        for d, n in dims:
            h += _name(d) + struct.pack(">I", 0 if n is None else n)
        h += _att_list(gattrs or {})
        h += struct.pack(">II", 0x0B, len(variables)) if variables else struct.pack(">II", 0, 0)
        for (name, vdims, attrs, arr), begin in zip(variables, begins):
            per = arr.dtype.itemsize * int(np.prod(arr.shape[1:] if vdims and vdims[0] == recdim else arr.shape, dtype=np.int64))
            vsize = min(per + (-per % 4), 0xFFFFFFFF)
            h += _name(name) + struct.pack(">I", len(vdims)) + b"".join(struct.pack(">I", dimnames.index(d)) for d in vdims)
            h += _att_list(attrs) + struct.pack(">II", NC_TYPE[arr.dtype.str[1:]], vsize) + struct.pack(off_fmt, begin)
        return h

    is_rec = [bool(vdims) and vdims[0] == recdim for _, vdims, _, _ in variables]
    hlen = len(header([0] * len(variables)))
    big = [arr.astype(arr.dtype.newbyteorder(">")) for _, _, _, arr in variables]
    begins, pos, fixed = [0] * len(variables), hlen, b""
    for i, a in enumerate(big):
        if not is_rec[i]:
            begins[i] = pos
            blob = _pad(a.tobytes())
            fixed += blob
            pos += len(blob)
    recs = [i for i, r in enumerate(is_rec) if r]
    one = len(recs) == 1
    for i in recs:
        begins[i] = pos
        per = big[i].dtype.itemsize * int(np.prod(big[i].shape[1:], dtype=np.int64))
        pos += per if one else per + (-per % 4)
    body = b""
    for r in range(numrecs):
        for i in recs:
            step = big[i][r:r + 1].tobytes()             # (a slice: an indexed scalar would come back in native order)
            body += step if one else _pad(step)
    with open(path, "wb") as f:
        f.write(header(begins) + fixed + body)
    return {v[0]: b for v, b in zip(variables, begins)}, hlen


class Case:
    """One file of the catalogue: ``write(dir)`` -> path (and sets ``begins`` {name: offset of the variable}, ``header_len``); ``var``
    the data variable the tests load; ``stored`` {name: array written}, ``attrs`` {name: attributes written}; ``dims`` / ``numrecs``
    as handed to `write_classic`."""

    def __init__(self, name, version, dims, variables, numrecs, var, gattrs=None):
        self.name, self.version, self.dims, self.variables, self.numrecs, self.var, self.gattrs = name, version, dims, variables, numrecs, var, gattrs
        self.stored = {v[0]: v[3] for v in variables}
        self.attrs = {v[0]: v[2] for v in variables}
        self.vdims = {v[0]: tuple(v[1]) for v in variables}

    def write(self, directory) -> str:
        path = os.path.join(str(directory), self.name + ".nc")
        self.begins, self.header_len = write_classic(path, self.version, self.dims, self.variables, self.numrecs, self.gattrs)
        return path

    def __repr__(self):
        return f"Case({self.name})"


def _grid(ny, nx):
    # descending latitudes, a 0-360 longitude axis (ERA5's layout)
    return (50.0 - 0.25 * np.arange(ny)).astype(np.float32), (230.0 + 0.25 * np.arange(nx)).astype(np.float32)


def _ints(rng, shape, dtype, fill=None, n_fill=4):
    info = np.iinfo(dtype)
    a = rng.integers(info.min + 2, info.max - 2, size=shape, dtype=dtype)
    if fill is not None and a.size:
        flat = a.reshape(-1)
        flat[rng.choice(flat.size, size=min(n_fill, flat.size), replace=False)] = fill
    return a


def _case(name, version, data, data_attrs, var, T=7, ny=3, nx=5, record=True, time_dtype=np.int32, with_time=True, extra=None,
          start_hour=876576, gattrs=None):
    """time (record or fixed) + latitude + longitude + the data variable(s).  ``extra``: further (name, attrs, array) record variables
    written before the data variable."""
    lat, lon = _grid(ny, nx)
    dims = [("time", None if record else T), ("latitude", ny), ("longitude", nx)]
    variables = [("longitude", ("longitude",), {"units": "degrees_east", "long_name": "longitude"}, lon),
                 ("latitude", ("latitude",), {"units": "degrees_north"}, lat)]
    if with_time:
        variables.append(("time", ("time",), {"units": HOURS, "calendar": "gregorian"}, (start_hour + np.arange(T)).astype(time_dtype)))
    for nm, at, arr in (extra or []):
        variables.append((nm, ("time", "latitude", "longitude"), at, arr))
    variables.append((var, ("time", "latitude", "longitude"), data_attrs, data))
    return Case(name, version, dims, variables, T if record else 0, var, gattrs)


def build_cases():
    rng = np.random.default_rng(20240607)
    T, ny, nx = 7, 3, 5
    cases = []
    # short, CDF-1: time + ONE data variable, double scale / offset (ERA5's), a fill value that occurs in the data; 30-byte planes (2 of padding)
    era = {"scale_factor": 0.0018311105046321, "add_offset": 273.6425033329, "_FillValue": np.int16(-32767), "units": "K", "long_name": "2 metre temperature"}
    cases.append(_case("short_cdf1", 1, _ints(rng, (T, ny, nx), np.int16, -32767), dict(era), "t2m"))
    # short, CDF-2: time + TWO data variables, float scale / offset, no fill value; a global attribute list
    f32 = {"scale_factor": np.float32(0.0123), "add_offset": np.float32(-4.5)}
    cases.append(_case("short_cdf2_two", 2, _ints(rng, (T, ny, nx), np.int16), dict(f32), "tp",
                       extra=[("a", dict(era), _ints(rng, (T, ny, nx), np.int16, -32767))], gattrs={"Conventions": "CF-1.6", "history": "x"}))
    # short under _Unsigned = "true": the fill written in the signed type (-1 = 65535) occurs in the data
    cases.append(_case("short_unsigned", 1, _ints(rng, (T, ny, nx), np.int16, -1),
                       {"_Unsigned": "true", "_FillValue": np.int16(-1), "scale_factor": 0.25, "add_offset": 10.0}, "u16v"))
    # exactly one record variable in the file: its 30-byte steps follow each other unpadded (time is a dimension without a variable)
    cases.append(_case("one_record_var", 2, _ints(rng, (T, ny, nx), np.int16, -32767), dict(era), "x", with_time=False))
    # a fixed time dimension: one contiguous block at `begin`
    cases.append(_case("fixed_time", 1, _ints(rng, (T, ny, nx), np.int16, -32767), dict(era), "sst", record=False, time_dtype=np.float64))
    # zero records
    cases.append(_case("zero_records", 1, np.zeros((0, ny, nx), np.int16), dict(era), "t2m", T=0))
    # int: a fill value in the data, a double scale factor alone -> float64 values
    cases.append(_case("int_cdf2", 2, _ints(rng, (T, ny, nx), np.int32, -2147483647), {"_FillValue": np.int32(-2147483647), "scale_factor": 1e-4}, "swvl1"))
    # float: a fill value in the data; attributes of every type, scalars and lists
    fl = rng.normal(280, 15, size=(T, ny, nx)).astype(np.float32)
    fl.reshape(-1)[[3, 17, 40]] = np.float32(9.96921e36)
    every = {"_FillValue": np.float32(9.96921e36), "b": np.int8(-3), "text": "metres per second", "s": np.int16(-12345), "i": np.int32(1 << 20),
             "d": 2.5e-3, "valid_range": np.array([-100, 100], np.int16), "levels": np.array([1.5, 2.5, 3.5]), "flags": np.array([1, 2, 3], np.int8),
             "f2": np.array([0.5, 0.25], np.float32), "i3": np.array([7, 8, 9], np.int32)}
    cases.append(_case("float_cdf1", 1, fl, every, "ws", time_dtype=np.float64))
    # double, no attributes at all
    cases.append(_case("double_cdf2", 2, rng.normal(0, 1, size=(T, ny, nx)), {}, "d"))
    # float without a fill value, beside a short variable (the short file's neighbour on the multi-file float32 route)
    cases.append(_case("float_nofill", 2, rng.normal(280, 15, size=(T, ny, nx)).astype(np.float32), {"units": "K"}, "t2m", start_hour=876576 + T))
    # (3, 33, 130): a launch of several workgroups, nx no multiple of 64
    cases.append(_case("short_wide", 2, _ints(rng, (3, 33, 130), np.int16, -32767, n_fill=50), dict(era), "t2m", T=3, ny=33, nx=130))
    return cases


def damaged_headers(good: bytes):
    """{reason: bytes} — the file ``good`` (a CDF-1 file with records) damaged in each way `netcdf3.NC3File` must refuse."""
    out = {}
    out["cdf5"] = good[:3] + b"\x05" + good[4:]
    out["streaming_numrecs"] = good[:4] + b"\xff\xff\xff\xff" + good[8:]
    out["truncated_header"] = good[:60]
    out["negative_count"] = good[:12] + struct.pack(">i", -2) + good[16:]               # the dimension count
    out["absurd_count"] = good[:12] + struct.pack(">I", 0x7FFFFFF0) + good[16:]
    out["last_record_beyond_the_file"] = good[:-8]
    return out


def with_begin_beyond(good: bytes, header_len: int, begin: int) -> bytes:
    """``good`` (CDF-1) with the variable entry whose 32-bit ``begin`` is the last such value in the header pointing beyond the file."""
    at = good.rfind(struct.pack(">I", begin), 0, header_len)
    assert at > 0
    return good[:at] + struct.pack(">I", len(good) + 4096) + good[at + 4:]
