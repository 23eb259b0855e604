"""uint16-packed cubes, the parts that need no GPU: the holder, the C header and its binding, `io.packing_of`, and the host route's
reading of uint16 storage and of int16 storage under ``_Unsigned = "true"`` (NetCDF User's Guide: the same bits)."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

import aggfly_amd as af
from aggfly_amd import hip
from aggfly_amd import io as afio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _packing_fields(p):
    return (p.n_pairs, p.has_fill, p.fill, p.pad, list(p.mul), list(p.add))


def test_packed_cube_holds_uint16_as_the_int16_of_the_same_bits():
    u = np.array([[0, 1, 32767, 32768, 40000, 65535]], dtype=np.uint16)
    cube = af.PackedCube(u, 0.1, 220.0, 32767)
    assert cube.unsigned and cube.storage == "uint16" and cube.q.dtype == torch.int16
    assert np.array_equal(cube.q.numpy().view(np.uint16), u)                       # a view: the bits are the stored ones
    assert np.array_equal(cube.q.numpy(), u.view(np.int16))
    from_tensor = af.PackedCube(torch.from_numpy(u.view(np.int16)).view(torch.uint16), 0.1, 220.0, 32767)
    assert from_tensor.unsigned and torch.equal(from_tensor.q, cube.q)
    assert af.PackedCube(u, fill_value=65535).fill_value == 65535 and af.PackedCube(u, fill_value=0).fill_value == 0
    for bad in (65536, -1):
        with pytest.raises(ValueError, match="uint16"):
            af.PackedCube(u, fill_value=bad)
    signed = af.PackedCube(u.view(np.int16), 0.1, 220.0, 32767)
    assert not signed.unsigned and signed.storage == "int16"
    with pytest.raises(ValueError, match="int16"):
        af.PackedCube(u.view(np.int16), fill_value=40000)
    assert af.PackedCube(u.view(np.int16), fill_value=-1).fill_value == -1
    with pytest.raises(ValueError):
        af.PackedCube(u, unsigned=False)
    with pytest.raises(TypeError):
        af.PackedCube(np.zeros(3, np.uint32))
    # the rule travels without the signedness: the library takes that from the plan's dtype / the entry point
    assert _packing_fields(cube.packing()) == _packing_fields(signed.packing())
    assert hip._dtype_code(cube) == hip.U16 and hip._dtype_code(signed) == hip.I16
    # the flag rides along with views, copies and folded arithmetic
    for derived in (cube[:, 2:], cube.permute(1, 0), cube.clone(), cube.contiguous(), cube.unsqueeze(0), cube - 273.15, (cube * 1.8) + 32.0):
        assert isinstance(derived, af.PackedCube) and derived.unsigned and derived.fill_value == 32767
    assert (cube - 273.15).pairs == [(np.float32(0.1), np.float32(220.0)), (None, np.float32(-273.15))]
    assert "uint16" in repr(cube) and "int16" in repr(signed) and "uint16" not in repr(signed)
    # int16 bits read as unsigned on request (what `_Unsigned` asks for)
    asked = af.PackedCube(u.view(np.int16), 0.1, 220.0, 65535, unsigned=True)
    assert asked.unsigned and asked.fill_value == 65535


def test_the_header_and_the_binding_know_the_unsigned_storage():
    hdr = open(os.path.join(ROOT, "include", "aggfly_hip.h")).read()
    assert int(re.search(r"#define AFHIP_U16 (\d+)", hdr).group(1)) == hip.U16 == 3
    assert int(re.search(r"#define AFHIP_I16 (\d+)", hdr).group(1)) == hip.I16 == 2
    assert re.search(r"int afhip_unpack_u16\(const void\* q_dev, int64_t n, const afhip_packing\* p, float\* out_dev, void\* stream\);", hdr)
    assert "afhip_unpack_u16" in hip.EXPORTS and "afhip_unpack_i16" in hip.EXPORTS
    assert hip.PACKED_CODES == (hip.I16, hip.U16)


def _standin(dtype, **attrs):
    return SimpleNamespace(dtype=np.dtype(dtype), attrs=attrs)


def test_packing_of_reads_the_signedness():
    gm = dict(scale_factor=0.1, add_offset=220.0)
    u = afio.packing_of(_standin(np.uint16, _FillValue=32767, **gm))
    assert u == (0.1, 220.0, 32767, True)
    assert af.PackedCube(np.zeros(3, np.uint16), *u).unsigned
    hi = afio.packing_of(_standin(np.uint16, _FillValue=65535, **gm))
    assert hi == (0.1, 220.0, 65535, True)
    for spelling in ("true", "True", "TRUE", b"true"):
        assert afio.packing_of(_standin(np.int16, _Unsigned=spelling, _FillValue=-1, **gm)) == hi, spelling
    assert afio.packing_of(_standin(np.int16, _Unsigned="true", _FillValue=65535, **gm)) == hi
    # plain int16 is what it was, with the signedness said
    assert afio.packing_of(_standin(np.int16, scale_factor=0.0017, add_offset=281.3, _FillValue=-32767)) == (0.0017, 281.3, -32767, False)
    assert afio.packing_of(_standin(np.int16, _Unsigned="false", _FillValue=-1, **gm)) == (0.1, 220.0, -1, False)
    assert afio.packing_of(_standin(np.int16)) == (None, None, None, False)
    assert u != afio.packing_of(_standin(np.int16, _FillValue=32767, **gm))          # the signedness is part of the key
    # fills no stored value can be
    assert afio.packing_of(_standin(np.uint16, _FillValue=-1, **gm)) is None
    assert afio.packing_of(_standin(np.uint16, _FillValue=65536, **gm)) is None
    assert afio.packing_of(_standin(np.int16, _FillValue=40000, **gm)) is None
    # other storage
    for dt in (np.uint32, np.uint64, np.uint8, np.int32, np.float32):
        assert afio.packing_of(_standin(dt, **gm)) is None
    with pytest.raises(ValueError, match="_Unsigned"):
        afio.packing_of(_standin(np.uint16, _Unsigned="false", **gm))


def test_the_device_routes_name_the_storage_they_refuse():
    with pytest.raises(ValueError, match="unsigned storage is streamed up to 16 bits"):
        afio._torch_dtype(np.uint32)
    with pytest.raises(ValueError, match="unsigned storage is streamed up to 16 bits"):
        afio._wire_dtype(np.uint64, {})
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        afio._wire_dtype(np.int32, {"_Unsigned": "true"})
    assert afio._wire_dtype(np.uint16, {}) == (np.dtype(np.int16), 65536.0)
    assert afio._wire_dtype(np.int16, {"_Unsigned": "true"}) == (np.dtype(np.int16), 65536.0)
    assert afio._wire_dtype(np.int8, {"_Unsigned": "True"}) == (np.dtype(np.int8), 256.0)
    assert afio._wire_dtype(np.int16, {}) == (np.dtype(np.int16), None)
    assert afio._wire_dtype(np.uint8, {}) == (np.dtype(np.uint8), None)
    assert afio._wire_dtype(np.float32, {"_Unsigned": "true"}) == (np.dtype(np.float32), None)


# ---- the host route ----
T, NY, NX = 48, 4, 5


def _store(tmp_path, name, stored, attrs):
    time = pd.date_range("2011-06-01", periods=T, freq="h")
    tv, tattrs = afio._encode_time(time)
    store = str(tmp_path / name)
    os.makedirs(store)
    json.dump({"zarr_format": 2}, open(os.path.join(store, ".zgroup"), "w"))
    afio._write_array(store, "tmmx", stored, ("time", "latitude", "longitude"), (24, NY, NX), attrs, None)
    afio._write_array(store, "time", np.asarray(tv, dtype=np.float64), ("time",), (T,), tattrs, None)
    afio._write_array(store, "latitude", 35 + 0.25 * np.arange(NY), ("latitude",), (NY,), {}, None)
    afio._write_array(store, "longitude", 250 + 0.25 * np.arange(NX), ("longitude",), (NX,), {}, None)
    return store


def _stored_values():
    rng = np.random.default_rng(4)
    stored = rng.integers(0, 65536, (T, NY, NX)).astype(np.uint16)
    stored.reshape(-1)[:6] = [0, 1, 32766, 32768, 40000, 65535]
    stored[rng.random((T, NY, NX)) < 0.05] = 32767
    stored[:, 1, 2] = 32767
    assert (stored >= 32768).mean() > 0.25
    return stored


def _chain(stored, fill):
    """float32, one rounded operation at a time; NaN at the fill."""
    f = stored.astype(np.float32)
    f = f * np.float32(0.1)
    f = f + np.float32(220.0)
    return np.where(stored == fill, np.float32(np.nan), f)


def _bits_equal(got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_host_route_reads_uint16_storage(tmp_path):
    stored = _stored_values()
    store = _store(tmp_path, "u16.zarr", stored, {"scale_factor": 0.1, "add_offset": 220.0, "_FillValue": 32767})
    want = _chain(stored, 32767)
    assert np.isnan(want).sum() == (stored == 32767).sum() > T
    _bits_equal(np.asarray(af.dataset_from_path(store, "tmmx").cube()), want)


def test_host_route_honours_the_unsigned_attribute(tmp_path):
    """The same bits written as int16 with ``_Unsigned = "true"`` read as the uint16 store does; a fill written in the signed type
    (-1) means 65535."""
    stored = _stored_values()
    as_int16 = _store(tmp_path, "i16u.zarr", stored.view(np.int16), {"scale_factor": 0.1, "add_offset": 220.0, "_FillValue": 32767, "_Unsigned": "true"})
    _bits_equal(np.asarray(af.dataset_from_path(as_int16, "tmmx").cube()), _chain(stored, 32767))
    stored = np.where(stored == 32767, np.uint16(65535), stored)
    minus_one = _store(tmp_path, "i16u_m1.zarr", stored.view(np.int16), {"scale_factor": 0.1, "add_offset": 220.0, "_FillValue": -1, "_Unsigned": "TRUE"})
    as_uint16 = _store(tmp_path, "u16_hi.zarr", stored, {"scale_factor": 0.1, "add_offset": 220.0, "_FillValue": 65535})
    want = _chain(stored, 65535)
    _bits_equal(np.asarray(af.dataset_from_path(minus_one, "tmmx").cube()), want)
    _bits_equal(np.asarray(af.dataset_from_path(as_uint16, "tmmx").cube()), want)
    # without the attribute the bits are signed, as before
    signed = _store(tmp_path, "i16.zarr", stored.view(np.int16), {"scale_factor": 0.1, "add_offset": 220.0, "_FillValue": -1})
    s = stored.view(np.int16)
    f = s.astype(np.float32) * np.float32(0.1) + np.float32(220.0)
    _bits_equal(np.asarray(af.dataset_from_path(signed, "tmmx").cube()), np.where(s == -1, np.float32(np.nan), f))


def test_one_byte_storage_under_the_unsigned_attribute():
    b = np.array([-128, -1, 0, 127], dtype=np.int8)
    out = afio._cf_mask_scale(b, {"_Unsigned": "true", "_FillValue": -1, "scale_factor": 0.5})
    assert out.dtype == np.float32 and np.array_equal(out[[0, 2, 3]], np.float32([64.0, 0.0, 63.5])) and np.isnan(out[1])
    with pytest.raises(ValueError, match="_Unsigned"):
        afio._cf_mask_scale(b.view(np.uint8), {"_Unsigned": "false", "scale_factor": 0.5})
