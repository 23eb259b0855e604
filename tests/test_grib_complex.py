"""GRIB2 complex packing (data representation templates 5.2 and 5.3) on the host: the index and the numpy decode of aggfly_amd/grib.py
against three hand-worked messages (tests/golden/grib_complex_known.json) and the catalogue of tests/grib_complex_cases.py — bit for bit,
NaN positions included —, every refusal with its reason, and the C-ABI surface of the device entry."""
import ctypes
import datetime as dt
import json
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_cases as C  # noqa: E402
import grib_complex_cases as K  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import distributed as D, grib, hip, io as afio  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.build_cases()
BY = {c.name: c for c in CASES}
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "grib_complex_known.json")))["messages"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gribc")
    return {c.name: c.write(d) for c in CASES}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, a.dtype, b.shape, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------
# known messages
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("known", KNOWN, ids=lambda k: k["name"])
def test_known_message(known, tmp_path):
    raw = bytes.fromhex(known["hex"])
    path = str(tmp_path / "known.grib2")
    with open(path, "wb") as f:
        f.write(raw)
    gf = grib.GribFile(path)
    assert len(gf.messages) == 1
    m = gf.messages[0]
    assert (m.edition, m.packing, m.order, m.extra, m.n_values, m.n_groups) == (2, known["template"], known["order"], known["extra"], known["N"], known["NG"])
    for key in ("Ni", "Nj", "E", "D", "R", "ref_width", "nbits_width", "ref_len", "len_inc", "last_len", "nbits_len"):
        assert getattr(m, key) == known[key], key
    assert m.nbits == known["nbits_ref"] and m.valid_time == dt.datetime.fromisoformat(known["valid_time"]) and m.bitmap_offset is None
    body = bytes.fromhex(known["body"])
    assert raw[m.data_offset:m.data_offset + m.data_length] == body
    # the integers first, then the floats bit for bit
    X = grib.unpack_complex(m, body)
    assert X.dtype == np.int64 and X.tolist() == known["X"]
    want = np.array([int(b, 16) for b in known["expected_bits"]], dtype=np.uint32).view(np.float32).reshape(known["Nj"], known["Ni"])
    _same_bits(gf.read("t2m"), want[None])
    # the working, re-done here from the golden numbers alone: the group tables give raw, and the recurrences of the format give X
    raw_vals, lens, order = known["raw"], known["lengths"], known["order"]
    assert sum(lens) == known["N"] == len(raw_vals) and lens[-1] == known["last_len"]
    Xr = list(raw_vals)
    if order == 1:
        Xr[0] = known["ival1"]
        for n in range(1, len(Xr)):
            Xr[n] = Xr[n - 1] + raw_vals[n] + known["minsd"]
    elif order == 2:
        Xr[0], Xr[1] = known["ival1"], known["ival2"]
        for n in range(2, len(Xr)):
            Xr[n] = raw_vals[n] + known["minsd"] + 2 * Xr[n - 1] - Xr[n - 2]
    assert Xr == known["X"]
    p = 0
    for ref, width, ln in zip(known["refs"], known["widths"], lens):
        assert all(0 <= v - ref < (1 << width) for v in raw_vals[p:p + ln])      # (width 0: every member is the reference)
        p += ln
    s, d = 2.0 ** known["E"], 10.0 ** -known["D"]
    _same_bits(np.array([np.float32(((float(x) * s) + known["R"]) * d) for x in known["X"]], dtype=np.float32).reshape(want.shape), want)
    # the case writer, given the same numbers, writes the same bytes
    st = K.CStep(known["X"], lens, known["template"], order, extra=known["extra"], E=known["E"], D=known["D"], R=known["R"],
                 valid=m.valid_time, **known["writer"])
    assert st.body == body and K.message(st, tuple(known["grid"])).hex() == known["hex"]
    assert st.table_bytes * 8 + st.value_bits == known["used_bits"]


def test_the_known_answer_of_the_issue():
    k = KNOWN[0]
    assert k["body"] == "000A000C800708008180CC008881F6C0" and k["used_bits"] == 123 and (k["template"], k["N"], k["order"], k["extra"]) == (3, 12, 2, 2)
    assert (k["NG"], k["nbits_ref"], k["ref_width"], k["nbits_width"], k["ref_len"], k["len_inc"], k["last_len"], k["nbits_len"]) == (3, 4, 0, 3, 2, 1, 5, 2)
    assert (k["refs"], k["widths"], k["lengths"]) == ([0, 8, 0], [4, 0, 3], [5, 2, 5])
    assert k["raw"] == [0, 0, 8, 8, 8, 8, 8, 0, 7, 6, 6, 6] and (k["ival1"], k["ival2"], k["minsd"]) == (10, 12, -7)
    assert k["X"] == [10, 12, 15, 19, 24, 30, 37, 37, 37, 36, 34, 31]


# ---------------------------------------------------------------------------------------
# the catalogue on the host route
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_on_the_host_route(case, files):
    gf = grib.GribFile(files[case.name])
    f = gf.select(case.var)
    want = case.expected
    got = gf.read(case.var)
    assert np.array_equal(got, want, equal_nan=True)
    _same_bits(got, want)
    assert f.shape == want.shape and list(f.time) == [pd.Timestamp(t) for t in case.times]
    for m, st in zip(f.messages, case.steps):
        if isinstance(st, K.CStep):
            assert (m.packing, m.order, m.n_values, m.n_groups, m.E, m.D, m.R) == (st.template, st.order, len(st.X), len(st.lens), st.E, st.D, st.R)
            assert (m.nbits, m.ref_width, m.nbits_width, m.ref_len, m.len_inc, m.last_len, m.nbits_len) == \
                (st.nbits_ref, st.ref_width, st.nbits_width, st.ref_len, st.len_inc, st.last_len, st.nbits_len)
            data = open(files[case.name], "rb").read()[m.data_offset:m.data_offset + m.data_length]
            assert grib.unpack_complex(m, data).tolist() == st.X               # the integers, before any float
        else:
            assert (m.packing, m.nbits) == (0, st.nbits)
    ds = af.dataset_from_path(files[case.name], case.var, device=None)
    assert np.array_equal(np.asarray(ds.cube()), want, equal_nan=True)
    _same_bits(np.asarray(ds.cube()), want)
    a = f.arrays()
    assert a["packing"].tolist() == [m.packing for m in f.messages] and a["n_groups"].tolist() == [m.n_groups for m in f.messages]


def test_the_catalogue_covers_what_it_should():
    steps = [s for c in CASES for s in c.steps if isinstance(s, K.CStep)]
    assert {(s.template, s.order) for s in steps} == {(2, 0), (3, 1), (3, 2)}
    assert {s.extra for s in steps if s.template == 3} >= {0, 1, 2, 4}
    assert any(s.ival[0] < 0 for s in steps) and any(s.minsd < 0 for s in steps)
    assert {0, 1, 31, 32} <= {w for s in steps for w in s.widths}
    assert any(s.nbits_ref == 0 and s.lens for s in steps) and any(s.nbits_width == 0 and len(s.lens) > 1 for s in steps)
    assert any(s.nbits_len == 0 and len(s.lens) > 1 for s in steps)
    assert any(s.len_inc > 1 and s.ref_len > 0 for s in steps)
    assert any(s.knobs["last_stored"] is not None and s.ref_len + s.len_inc * s.knobs["last_stored"] != s.lens[-1] for s in steps)
    assert any(len(s.lens) == 1 for s in steps) and any(not s.lens for s in steps) and any(len(s.lens) == len(s.X) > 1 for s in steps)
    assert any(s.order == 2 and s.raw[:2] != [0, 0] for s in steps) and any(s.bitmap is not None and 0 < len(s.X) < K.NP for s in steps)
    kinds = [type(s) for s in BY["c3_mixed_with_simple"].steps]
    assert K.CStep in kinds and C.Step in kinds
    assert len({(s.E, s.D, s.R) for s in BY["c3_order2"].steps}) == 4
    assert np.isnan(BY["c3_bitmap"].expected).any() and not np.isnan(BY["c3_bitmap"].expected[:3]).all()


def test_wrapping_sums_are_int64(tmp_path):
    """Order 2 over values near 2^40: the sums stay exact integers (no float in between), and X converts exactly below 2^53."""
    rng = np.random.default_rng(5)
    inc = rng.integers(0, 1 << 31, size=K.NP)
    inc[0], inc[1] = 1 << 20, 5                                          # (ival1 and ival2 are 31-bit magnitudes)
    X = np.cumsum(np.cumsum(inc)).tolist()
    assert max(X) > 1 << 39
    st = K.CStep(X, K.cut(rng, K.NP), 3, 2, extra=4, minsd=0, E=-30, R=0.25)
    path = str(tmp_path / "big.grib2")
    with open(path, "wb") as f:
        f.write(K.message(st))
    gf = grib.GribFile(path)
    m = gf.messages[0]
    assert grib.unpack_complex(m, open(path, "rb").read()[m.data_offset:m.data_offset + m.data_length]).tolist() == X
    _same_bits(gf.read("t2m")[0], st.expected(K.NJ, K.NI))


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,raw,reason,on_read", K.refusals(), ids=[r[0] for r in K.refusals()])
def test_refusals_name_their_reason(name, raw, reason, on_read, tmp_path):
    path = str(tmp_path / (name + (".grib" if raw[7] == 1 else ".grib2")))
    with open(path, "wb") as f:
        f.write(raw)
    if on_read:
        gf = grib.GribFile(path)                                          # the headers are sound: the tables are not
        with pytest.raises(ValueError, match=re.escape(reason)):
            gf.read("t2m")
    else:
        with pytest.raises(ValueError, match=re.escape(reason)):
            grib.GribFile(path)
    with pytest.raises(ValueError, match=re.escape(reason)):
        af.dataset_from_path(path, "t2m", device=None, lon_is_360=False)


def test_a_bitmap_that_disagrees_with_n_is_refused(tmp_path):
    rng = np.random.default_rng(6)
    bm = C.some_bitmap(rng)
    st = K.CStep(K.smooth(rng, sum(bm) - 1), K.cut(rng, sum(bm) - 1), 3, 2, extra=2, bitmap=bm)
    path = str(tmp_path / "bm.grib2")
    with open(path, "wb") as f:
        f.write(K.message(st))
    with pytest.raises(ValueError, match="present grid points"):
        grib.GribFile(path).read("t2m")


# ---------------------------------------------------------------------------------------
# the routes around the decode, and the C ABI
# ---------------------------------------------------------------------------------------
def test_time_coordinate_step_bytes_and_time_sel(files):
    case = BY["c3_shuffled"]
    assert afio.read_time_coordinate(files[case.name], "t2m").equals(pd.DatetimeIndex(case.times))
    assert D._step_bytes(files[case.name], "t2m") == K.NJ * K.NI * 4
    ds = af.dataset_from_path(files[case.name], "t2m", time_sel=slice("2024-07-15T01:00", "2024-07-15T03:00"), lon_is_360=False)
    _same_bits(np.asarray(ds.cube()), case.expected[1:4])


def test_header_exports_and_record_size():
    hdr = open(os.path.join(ROOT, "include", "aggfly_hip.h")).read()
    assert "#define AFHIP_ABI_VERSION 4" in hdr and hip.ABI_VERSION == 4                     # additive: the ABI version stays
    for name in ("afhip_grib_unpack_complex", "afhip_grib_complex_scratch_bytes"):
        assert name in hip.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    assert "afhip_grib_unpack" in hip.EXPORTS and hip.GRIB_STEP.itemsize == 64                # the simple-packing entry is as it was
    body = re.search(r"typedef struct afhip_grib_cstep \{(.*?)\} afhip_grib_cstep;", hdr, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), ctype) for n in names.split(",")]
    sizes = {"int64_t": ("<i8", 8), "int32_t": ("<i4", 4), "double": ("<f8", 8)}
    assert [(n, sizes[t][0]) for n, t in fields] == [(n, hip.GRIB_CSTEP[n].str) for n in hip.GRIB_CSTEP.names]
    assert hip.GRIB_CSTEP.itemsize == sum(sizes[t][1] for _, t in fields) == 112
    lib = hip.load()
    assert lib.afhip_grib_complex_scratch_bytes.restype is ctypes.c_int64
    # the size query: monotone, 16-byte multiples, -1 for absurd sizes
    one = hip.grib_complex_scratch_bytes(1, 4290, 300)
    assert one % 16 == 0 and one >= 4290 * 8 + 300 * 16 and hip.grib_complex_scratch_bytes(3, 4290, 300) >= 3 * (4290 * 8 + 300 * 16)
    assert hip.grib_complex_scratch_bytes(0, 4290, 0) >= 0
    for bad in ((-1, 10, 1), (1, 0, 1), (1, 1 << 31, 1), (1, 10, -1), (1, 10, 1 << 31), (1 << 31, 10, 1), ((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1)):
        with pytest.raises(ValueError):
            hip.grib_complex_scratch_bytes(*bad)
