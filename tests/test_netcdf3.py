"""NetCDF classic files without a GPU: the catalogue's own writer against scipy, the header reader (`aggfly_amd/netcdf3.py`)
against scipy and against the bytes of the file, the headers it must refuse, and the store routes' questions
(`read_time_coordinate`, `distributed._step_bytes`)."""
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import netcdf3_cases as C  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import distributed as D, io as afio, netcdf3  # noqa: E402

CASES = C.build_cases()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("classic")
    return {c.name: c.write(d) for c in CASES}


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype.newbyteorder("=") == b.dtype.newbyteorder("="), (a.shape, a.dtype, b.shape, b.dtype)
    np.testing.assert_array_equal(a.astype(a.dtype.newbyteorder("=")).view(np.uint8), b.astype(b.dtype.newbyteorder("=")).view(np.uint8))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_catalogue_files_are_what_scipy_reads(case, files):
    """The writer of the catalogue is checked by an independent reader: every variable comes back as written."""
    from scipy.io import netcdf_file
    with netcdf_file(files[case.name], "r", mmap=False) as nc:
        assert nc.version_byte == case.version
        assert set(nc.variables) == set(case.stored)
        for name, arr in case.stored.items():
            v = nc.variables[name]
            assert tuple(v.dimensions) == case.vdims[name]
            _same_bits(np.array(v.data), arr)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_header_reader_agrees_with_scipy(case, files):
    from scipy.io import netcdf_file
    f = netcdf3.NC3File(files[case.name])
    with netcdf_file(files[case.name], "r", mmap=False) as nc:
        assert f.version == nc.version_byte and f.numrecs == nc._recs
        assert {k: v for k, v in f.dimensions.items()} == dict(nc.dimensions)
        assert set(f.variables) == set(nc.variables)
        for k, val in nc._attributes.items():
            assert f.attrs[k] == val.decode()
        for name, sv in nc.variables.items():
            v = f.variables[name]
            assert v.dims == tuple(sv.dimensions) and v.shape == tuple(sv.shape), name
            assert v.dtype == sv.data.dtype and v.dtype.byteorder in (">", "|"), name
            assert v.is_record == sv.isrec
            assert set(v.attrs) == set(sv._attributes)
            for k, want in sv._attributes.items():
                got = v.attrs[k]
                if isinstance(want, bytes):
                    assert isinstance(got, str) and got == want.decode()
                else:
                    assert np.ndim(got) == np.ndim(want) and np.asarray(got).dtype == np.asarray(want).dtype.newbyteorder("=")
                    np.testing.assert_array_equal(got, want)
            _same_bits(f.read(name), np.array(sv.data))
    # the attributes in the forms the CF helpers take: what was written comes back
    for k, want in case.attrs[case.var].items():
        got = f.variables[case.var].attrs[k]
        if isinstance(want, str):
            assert got == want
        else:
            np.testing.assert_array_equal(got, want)
            assert np.asarray(got).dtype == (np.asarray(want).dtype if np.asarray(want).dtype != np.int64 else np.int32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_plane_offsets_select_each_steps_bytes(case, files):
    raw = open(files[case.name], "rb").read()
    f = netcdf3.NC3File(files[case.name])
    for name, arr in case.stored.items():
        v = f.variables[name]
        assert v.begin == case.begins[name]
        if not v.shape:
            continue
        inner = int(np.prod(arr.shape[1:], dtype=np.int64)) * arr.dtype.itemsize
        assert v.plane_bytes == inner
        for t in range(v.shape[0]):
            o = v.plane_offset(t)
            assert raw[o:o + inner] == arr[t:t + 1].astype(arr.dtype.newbyteorder(">")).tobytes(), (name, t)
        with pytest.raises(IndexError):
            v.plane_offset(v.shape[0])
    recs = [v for v in f.variables.values() if v.is_record]
    if len(recs) == 1:                                             # the no-padding rule
        assert f.recsize == recs[0].plane_bytes
    else:
        assert f.recsize == sum(v.plane_bytes + (-v.plane_bytes % 4) for v in recs)


def test_record_size_rules_are_exercised():
    """The catalogue holds what its description promises: an odd int16 plane in a file with one record variable (unpadded) and in
    files with two and three (padded), both versions, a fixed time dimension, zero records, names of 1 to 5 characters."""
    by = {c.name: c for c in CASES}
    assert by["one_record_var"].stored["x"][0].nbytes % 4 == 2 and "time" not in by["one_record_var"].stored
    assert {c.version for c in CASES} == {1, 2}
    assert dict(by["fixed_time"].dims)["time"] == 7 and by["zero_records"].numrecs == 0
    assert {len(c.var) for c in CASES} >= {1, 2, 3, 4, 5}
    assert {c.stored[c.var].dtype.str[1:] for c in CASES} == {"i2", "i4", "f4", "f8"}
    assert by["short_wide"].stored["t2m"].shape == (3, 33, 130)


def _damaged(files):
    case = CASES[0]
    good = open(files[case.name], "rb").read()
    out = C.damaged_headers(good)
    out["begin_beyond_the_file"] = C.with_begin_beyond(good, case.header_len, case.begins[case.var])
    return case, out


REASONS = ["cdf5", "streaming_numrecs", "truncated_header", "negative_count", "absurd_count", "last_record_beyond_the_file",
           "begin_beyond_the_file"]


@pytest.mark.parametrize("reason", REASONS)
def test_damaged_headers_are_refused_with_a_reason(reason, files, tmp_path):
    case, damaged = _damaged(files)
    p = str(tmp_path / f"{reason}.nc")
    with open(p, "wb") as f:
        f.write(damaged[reason])
    words = {"cdf5": "CDF-5", "streaming_numrecs": "streaming", "truncated_header": "truncated", "negative_count": "negative",
             "absurd_count": "absurd", "last_record_beyond_the_file": "beyond the end", "begin_beyond_the_file": "beyond the end"}
    with pytest.raises(ValueError, match=words[reason]):
        netcdf3.NC3File(p)
    assert afio._netcdf3_source(p, case.var) is None               # the streaming route declines ...
    assert D._step_bytes(p, case.var) is None


@pytest.mark.parametrize("reason", REASONS)
def test_refused_file_still_opens_on_the_host_route(reason, files, tmp_path, monkeypatch):
    """... and `dataset_from_path` returns what the host route makes of the file: here with scipy's reader stubbed by the intact
    file's dataset, since scipy itself stumbles over most of these headers."""
    case, damaged = _damaged(files)
    p = str(tmp_path / f"{reason}.nc")
    with open(p, "wb") as f:
        f.write(damaged[reason])
    seen = []
    real = afio._open_netcdf3
    monkeypatch.setattr(afio, "_open_netcdf3", lambda path, var: seen.append(path) or real(files[case.name], var))
    monkeypatch.setattr(af.Dataset, "to_device", lambda self, device="cuda": self)      # (no GPU here: the route decision is what is tested)
    ds = af.dataset_from_path(p, case.var, device="cuda")
    assert seen == [p]
    want = afio._cf_mask_scale(case.stored[case.var], case.attrs[case.var])
    _same_bits(ds.cube(), want)


def test_unstreamed_variables_go_to_the_host_route(tmp_path):
    """byte / char variables, arrays that are not time-leading and 4-D variables are not for the streaming route."""
    lat, lon = C._grid(3, 5)
    base = [("longitude", ("longitude",), {}, lon), ("latitude", ("latitude",), {}, lat),
            ("time", ("time",), {"units": C.HOURS}, np.arange(7, dtype=np.int32))]
    dims = [("time", None), ("latitude", 3), ("longitude", 5), ("level", 2)]
    variables = base + [("b", ("time", "latitude", "longitude"), {}, np.zeros((7, 3, 5), np.int8)),
                        ("c", ("time", "latitude", "longitude"), {}, np.full((7, 3, 5), b"x", "S1")),
                        ("yx_t", ("latitude", "longitude", "level"), {}, np.zeros((3, 5, 2), np.float32)),
                        ("four", ("time", "level", "latitude", "longitude"), {}, np.zeros((7, 2, 3, 5), np.float32)),
                        ("ok", ("time", "latitude", "longitude"), {}, np.zeros((7, 3, 5), np.float32))]
    p = str(tmp_path / "mixed.nc")
    C.write_classic(p, 1, dims, variables, 7)
    assert afio._netcdf3_source(p, "ok") is not None
    for name in ("b", "c", "yx_t", "four", "absent"):
        assert afio._netcdf3_source(p, name) is None, name


def test_store_routes_answer_for_a_classic_file(files, monkeypatch):
    by = {c.name: c for c in CASES}
    for name in ("short_cdf1", "fixed_time", "float_cdf1", "zero_records"):
        case = by[name]
        t = afio.read_time_coordinate(files[name], case.var)
        want = pd.Timestamp("1900-01-01") + pd.to_timedelta(case.stored["time"].astype(np.int64), unit="h")
        assert isinstance(t, pd.DatetimeIndex) and t.equals(pd.DatetimeIndex(want))
    with pytest.raises(ValueError):
        afio.read_time_coordinate(files["one_record_var"], "x")            # a time dimension without a variable
    monkeypatch.delenv("AGGFLY_HIP_KEEP_PACKED", raising=False)
    cells = 3 * 5
    assert D._step_bytes(files["short_cdf1"], "t2m") == cells * 4                       # unpacked to float32 in HBM
    assert D._step_bytes(files["short_cdf1"], "t2m", keep_packed=True) == cells * 2     # kept as stored
    assert D._step_bytes(files["short_unsigned"], "u16v", keep_packed=True) == cells * 2
    assert D._step_bytes(files["int_cdf2"], "swvl1", keep_packed=True) == cells * 4
    assert D._step_bytes(files["float_cdf1"], "ws", keep_packed=True) == cells * 4
    assert D._step_bytes(files["double_cdf2"], "d") == cells * 8
    assert D._step_bytes(files["short_wide"], "t2m", keep_packed=True) == 33 * 130 * 2
    monkeypatch.setenv("AGGFLY_HIP_KEEP_PACKED", "1")
    assert D._step_bytes(files["short_cdf1"], "t2m") == cells * 2


def test_cli_asks_the_header_whether_a_classic_file_streams(files, tmp_path):
    """`cli/pipeline.py`: the single-store route and `load_grid` take a classic file whose variable the streaming route takes."""
    from types import SimpleNamespace
    from aggfly_amd.cli import pipeline
    assert pipeline._streams_classic(SimpleNamespace(var="t2m", timecoord="time"), files["short_cdf1"])
    assert pipeline._streams_classic(SimpleNamespace(var="sst", timecoord="time"), files["fixed_time"])
    assert not pipeline._streams_classic(SimpleNamespace(var="absent", timecoord="time"), files["short_cdf1"])
    assert not pipeline._streams_classic(SimpleNamespace(var="t2m", timecoord="valid_time"), files["short_cdf1"])
    other = tmp_path / "not_classic.nc"
    other.write_bytes(b"\x89HDF\r\n\x1a\n" + b"\0" * 64)
    assert not pipeline._streams_classic(SimpleNamespace(var="t2m", timecoord="time"), str(other))


def test_host_route_unpacks_like_every_other_container(files):
    """`_open_netcdf3` hands scipy's numpy scalars on as attributes; the values are unpacked in float32 all the same, as from a Zarr
    store or a netCDF-4 file with the same attributes (Python numbers)."""
    by = {c.name: c for c in CASES}
    for name in ("short_cdf1", "short_cdf2_two", "short_unsigned", "int_cdf2", "float_cdf1"):
        case = by[name]
        host = af.dataset_from_path(files[name], case.var)
        _same_bits(host.cube(), afio._cf_mask_scale(case.stored[case.var], case.attrs[case.var]))
