"""GRIB files on the host: the index and the numpy decode of aggfly_amd/grib.py against two hand-assembled messages
(tests/golden/grib_known_messages.json) and the catalogue of tests/grib_cases.py — bit for bit, NaN positions included —, every refusal
with its reason, and `dataset_from_path` / `read_time_coordinate` on GRIB paths."""
import datetime as dt
import json
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_cases as C  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import grib, io as afio  # noqa: E402

CASES = C.build_cases()
BY = {c.name: c for c in CASES}
KNOWN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grib_known_messages.json")))["messages"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("grib")
    return {c.name: c.write(d) for c in CASES}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, a.dtype, b.shape, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------
# known messages and numbers
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("known", KNOWN, ids=lambda k: k["name"])
def test_known_message(known, tmp_path):
    raw = bytes.fromhex(known["hex"])
    path = str(tmp_path / ("known.grib" if known["edition"] == 1 else "known.grib2"))
    with open(path, "wb") as f:
        f.write(raw)
    assert grib.is_grib(path)
    gf = grib.GribFile(path)
    assert len(gf.messages) == 1
    m = gf.messages[0]
    assert (m.edition, list(m.param), m.level_type, m.level) == (known["edition"], known["param"], known["level_type"], known["level"])
    assert m.valid_time == dt.datetime.fromisoformat(known["valid_time"])
    for key in ("Ni", "Nj", "La1", "Lo1", "La2", "Lo2", "scan", "D", "E", "R", "nbits", "data_offset", "data_length", "bitmap_offset", "bitmap_length"):
        assert getattr(m, key) == known[key], key
    assert m.offset == 0 and m.length == len(raw) and m.n_values == len(known["X"]) and m.short_name == known["var"]
    want = np.array([int(b, 16) for b in known["expected_bits"]], dtype=np.uint32).view(np.float32).reshape(known["Nj"], known["Ni"])
    got = gf.read(known["var"])
    _same_bits(got, want[None])
    # the case writer, given the same numbers, writes the same bytes and expects the same values
    ref = dt.datetime.fromisoformat(known["reference_time"])
    step = C.Step(known["X"], known["nbits"], E=known["E"], D=known["D"], R=known["R"], bitmap=known["bitmap"], valid=m.valid_time)
    g = (known["Ni"], known["Nj"], known["La1"], known["Lo1"], known["La2"], known["Lo2"], known["scan"])
    if known["edition"] == 1:
        mine = C.message1(step, g, param=known["param"][0], table=known["param"][1], level_type=known["level_type"], level=known["level"],
                          ref=ref, p1=known["step_hours"])
    else:
        mine = C.message2(step, g, ref=ref, forecast=known["step_hours"], param=tuple(known["param"]), surface=(known["level_type"], 0, known["level"]))
    assert mine.hex() == known["hex"]
    _same_bits(step.expected(known["Nj"], known["Ni"]), want)
    f = gf.select(known["var"])
    assert f.time.equals(pd.DatetimeIndex([known["valid_time"]]))
    c = f.coords()
    np.testing.assert_array_equal(c["latitude"], np.linspace(known["La1"], known["La2"], known["Nj"]))
    np.testing.assert_array_equal(c["longitude"], np.linspace(known["Lo1"], known["Lo2"], known["Ni"]))


@pytest.mark.parametrize("word,value", [(0x42640000, 100.0), (0xC276A000, -118.625), (0x41100000, 1.0), (0x00000000, 0.0)])
def test_ibm_floats(word, value):
    assert grib.ibm_float(word) == value
    assert int.from_bytes(C.ibm(value), "big") == word


@pytest.mark.parametrize("bits,word,value", [(16, 0x0002, 2), (16, 0x8002, -2), (16, 0x8000, 0), (24, 0x00C350, 50000), (24, 0x802904, -10500),
                                             (32, 0x80989680, -10000000), (32, 0x14DC9380, 350000000), (8, 0x81, -1)])
def test_sign_magnitude(bits, word, value):
    assert grib.sign_magnitude(word, bits) == value
    if value or not word:
        assert int.from_bytes(C.sm(value, bits // 8), "big") == word


@pytest.mark.parametrize("edition", [1, 2])
def test_sign_magnitude_in_headers(edition, tmp_path):
    """E, D, latitudes and longitudes of either sign, through a file."""
    rng = np.random.default_rng(3)
    for j, (E, D, la1, lo1, la2, lo2, scan) in enumerate([(-5, -2, -30.0, -20.0, -31.0, -18.0, 0), (5, 2, 30.0, 20.0, 31.0, 22.0, 0x40),
                                                          (0, 0, 0.5, -1.0, -0.5, 1.0, 0)]):
        st = C.field(rng, 11, 0, E=E, D=D, R=-0.5)
        g = (C.NI, C.NJ, la1, lo1, la2, lo2, scan)
        path = str(tmp_path / f"sm{j}.grib")
        with open(path, "wb") as f:
            f.write((C.message1 if edition == 1 else C.message2)(st, g))
        gf = grib.GribFile(path)
        m = gf.messages[0]
        assert (m.E, m.D, m.La1, m.Lo1, m.La2, m.Lo2, m.scan, m.R) == (E, D, la1, lo1, la2, lo2, scan, -0.5)
        _same_bits(gf.read("t2m")[0], st.expected(C.NJ, C.NI))


# ---------------------------------------------------------------------------------------
# the catalogue on the host route
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_on_the_host_route(case, files):
    gf = grib.GribFile(files[case.name])
    f = gf.select(case.var, **case.read_kw)
    want = case.expected
    _same_bits(gf.read(case.var, **case.read_kw), want)
    assert f.shape == want.shape
    assert list(f.time) == [pd.Timestamp(t) for t in case.times]
    c = f.coords()
    np.testing.assert_array_equal(c["latitude"], case.latitude)
    np.testing.assert_array_equal(c["longitude"], case.longitude)
    assert (c["latitude"][0] < c["latitude"][-1]) == bool(case.grid[6] & 0x40) and (np.diff(c["longitude"]) > 0).all()
    for m, st in zip(f.messages, case.steps):
        assert (m.nbits, m.E, m.D, m.R, m.bitmap_offset is not None) == (st.nbits, st.E, st.D, st.R, st.bitmap is not None)
    ds = af.dataset_from_path(files[case.name], case.var, **case.read_kw)
    _same_bits(np.asarray(ds.cube()), want)


def test_the_catalogue_covers_what_it_should():
    some = BY["e1_bitmap_some_missing"].expected
    assert np.isnan(some).any() and not np.isnan(some).all()
    assert np.isnan(BY["e2_bitmap_all_missing"].expected).all() and not np.isnan(BY["e1_bitmap_none_missing"].expected).any()
    v = BY["e1_varying"].steps
    assert len({s.nbits for s in v}) > 3 and len({s.E for s in v}) > 3 and len({s.R for s in v}) > 3 and {s.bitmap is None for s in v} == {True, False}
    assert BY["e1_south_to_north_lon_wraps"].longitude[-1] == 364.0
    assert not np.array_equal(BY["e1_shuffled_t2m"].expected, BY["e1_shuffled_d2m"].expected)


def test_numeric_variable_names(files):
    for name, numeric in (("e1_shuffled_t2m", "167"), ("e1_shuffled_t2m", "167.128"), ("e1_shuffled_d2m", "168.128"), ("e2_shuffled_d2m", "0.0.6"),
                          ("e2_shuffled_d2m", "0.0.6.103.2")):
        _same_bits(grib.GribFile(files[name]).read(numeric), BY[name].expected)
    with pytest.raises(KeyError, match="msl"):
        grib.GribFile(files["e1_n16"]).select("msl")
    with pytest.raises(KeyError):
        grib.GribFile(files["e1_n16"]).select("167.1")


def test_filter_by_keys_picks_a_level(tmp_path):
    rng = np.random.default_rng(5)
    steps = {lev: [C.field(rng, 16, k) for k in range(3)] for lev in (850, 500)}
    path = str(tmp_path / "levels.grib")
    with open(path, "wb") as f:
        for k in range(3):
            for lev in (850, 500):
                f.write(C.message1(steps[lev][k], C.GRID, param=130, level_type=100, level=lev))
    gf = grib.GribFile(path)
    with pytest.raises(ValueError, match=r"several levels.*\(100, 500\), \(100, 850\)"):
        gf.select("t")
    for lev in (850, 500):
        want = np.stack([s.expected(C.NJ, C.NI) for s in steps[lev]])
        _same_bits(gf.read("t", filter_by_keys={"level": lev}), want)
        _same_bits(np.asarray(af.dataset_from_path(path, "t", filter_by_keys={"level": lev}).cube()), want)
        _same_bits(np.asarray(af.dataset_from_path(path, "t", engine="cfgrib", backend_kwargs={"filter_by_keys": {"level": lev}}).cube()), want)
    with pytest.raises(ValueError, match="typeOfLevel"):
        gf.select("t", filter_by_keys={"typeOfLevel": "surface"})


def test_a_year_of_headers_indexes_quickly(tmp_path):
    """8,760 messages index from page cache in well under a second (the data sections are never read)."""
    import time
    rng = np.random.default_rng(9)
    msgs = [C.message1(C.field(rng, 16, 0), C.GRID)]
    one = bytearray(msgs[0])
    path = str(tmp_path / "year.grib")
    with open(path, "wb") as f:
        for k in range(8760):
            t = C.BASE + dt.timedelta(hours=k)
            one[8 + 12], one[8 + 13], one[8 + 14], one[8 + 15] = t.year - 2000, t.month, t.day, t.hour      # PDS octets 13 - 16
            f.write(one)
    grib.GribFile(path)                                                             # (warm the page cache)
    t0 = time.perf_counter()
    gf = grib.GribFile(path)
    took = time.perf_counter() - t0
    assert len(gf.messages) == 8760 and gf.select("t2m").time[-1] == pd.Timestamp(C.BASE + dt.timedelta(hours=8759))
    assert took < 1.0, took


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,raw,edition,var,kw,reason", C.refusals(), ids=lambda v: v if isinstance(v, str) and v[:1] == "e" and "_" in v else "")
def test_refusals_name_their_reason(name, raw, edition, var, kw, reason, tmp_path):
    path = str(tmp_path / (name + ".grib"))
    with open(path, "wb") as f:
        f.write(raw)
    with pytest.raises(ValueError) as e:
        grib.GribFile(path).read(var, **kw)
    assert reason in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:                         # ... and through the front door: no other reader is tried
        af.dataset_from_path(path, var)
    assert reason in str(e.value), str(e.value)


def test_a_truncated_file_names_the_offset(tmp_path):
    rng = np.random.default_rng(2)
    a, b = C.message1(C.field(rng, 12, 0), C.GRID), C.message1(C.field(rng, 12, 1), C.GRID)
    path = str(tmp_path / "cut.grib")
    with open(path, "wb") as f:
        f.write(a + b[:-5])
    with pytest.raises(ValueError, match=f"offset {len(a)}"):
        grib.GribFile(path)
    with open(path, "wb") as f:
        f.write(a + b[:-4] + b"7778")
    with pytest.raises(ValueError, match=f"offset {len(a)}"):
        grib.GribFile(path)


# ---------------------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------------------
def test_dataset_from_path_routes_grib(files, monkeypatch):
    def refuse(path, var):
        raise AssertionError(f"{path}: scipy was asked to read a GRIB file")
    monkeypatch.setattr(afio, "_open_netcdf3", refuse)
    case = BY["e1_n16"]
    for kw in ({}, {"engine": "cfgrib"}):
        ds = af.dataset_from_path(files[case.name], "t2m", **kw)
        _same_bits(np.asarray(ds.cube()), case.expected)
        assert ds.time.equals(pd.DatetimeIndex(case.times))
        np.testing.assert_array_equal(ds.latitude, case.latitude)
        np.testing.assert_array_equal(ds.longitude, case.longitude)
    case2 = BY["e2_n12"]
    assert af.dataset_from_path(files[case2.name], "t2m").time.equals(pd.DatetimeIndex(case2.times))


def test_a_list_of_two_files_and_time_sel(tmp_path):
    rng = np.random.default_rng(11)
    steps = [C.field(rng, 16, k) for k in range(10)]
    paths = []
    for j, part in enumerate((steps[:4], steps[4:])):
        paths.append(str(tmp_path / f"part{j}.grib"))
        with open(paths[-1], "wb") as f:
            f.write(b"".join(C.message1(s, C.GRID) for s in part))
    want = np.stack([s.expected(C.NJ, C.NI) for s in steps])
    ds = af.dataset_from_path(paths, "t2m")
    _same_bits(np.asarray(ds.cube()), want)
    assert ds.time.equals(pd.DatetimeIndex([s.valid for s in steps]))
    ds = af.dataset_from_path(str(tmp_path / "part*.grib"), "t2m", time_sel=slice("2024-07-15T02:00", "2024-07-15T06:00"))
    _same_bits(np.asarray(ds.cube()), want[2:7])
    assert ds.time.equals(pd.DatetimeIndex([s.valid for s in steps[2:7]]))
    ds = af.dataset_from_path(paths[1], "t2m", time_window=(1, 3))
    _same_bits(np.asarray(ds.cube()), want[5:7])


def test_read_time_coordinate_and_step_bytes(files):
    from aggfly_amd import distributed as D
    for name in ("e1_shuffled_d2m", "e2_templates_0_and_8", "e1_time_ranges"):
        case = BY[name]
        assert afio.read_time_coordinate(files[name], case.var).equals(pd.DatetimeIndex(case.times))
    assert D._step_bytes(files["e1_n12"], "t2m") == C.NJ * C.NI * 4
    assert D._step_bytes(files["e1_n12"], "t2m", keep_packed=True) == C.NJ * C.NI * 4
