"""GeoTIFF stacks on the host: the directory reader of `aggfly_amd/tiff.py` (fields, coordinates, times from names), `TiffStack.read`
against the arrays the independent writer of tests/tiff_cases.py started from and against the files Pillow's libtiff wrote
(tests/golden/tiff), the writer itself against Pillow where Pillow imports, `afcodec_lzw_decode_ranges` — the text of lzw_passes.h the
GPU kernel runs — on the stream catalogue between guard bytes, every refusal with its word, the C-ABI surface of the new entries, and
`dataset_from_path` on a glob.  Every comparison of values is bit for bit."""
import json
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_cases as TC  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import codec, hip, io as afio, tiff  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "tiff")
GOLDEN = json.load(open(os.path.join(GOLDEN_DIR, "index.json")))
CASES = TC.file_catalogue()
STREAMS = TC.stream_catalogue()
REFUSALS = TC.refusal_catalogue()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiffs")
    return {c["name"]: TC.write_case(c, str(d / f"c{i}")) for i, c in enumerate(CASES)}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, a.dtype, b.shape, b.dtype)
    assert a.tobytes() == b.tobytes()


def _masked(values, nodata):
    """What `TiffStack.read` makes of stored values: NaN at the nodata value; integers with one become float32 (up to 16 bits) / float64."""
    if nodata is None:
        return values
    out = values.astype(values.dtype if values.dtype.kind == "f" else (np.float32 if values.dtype.itemsize <= 2 else np.float64))
    out[values == nodata] = np.nan
    return out


# ---------------------------------------------------------------------------------------
# the parser
# ---------------------------------------------------------------------------------------
def test_the_catalogue_covers_what_the_issue_lists():
    names = " | ".join(c["name"] for c in CASES)
    for word in ("strips", "tiles", "comp1", "comp5", "comp8", "pred2", "pred3", "MM", "BigTIFF", "multi-page", "nodata", "overviews",
                 "width 1", "width 63", "width 64", "width 65", "width 129", "width 257", "no EOI"):
        assert word in names, word
    assert {c["values"].dtype.str[1:] for c in CASES} == {"f4", "f8", "u1", "i1", "u2", "i2", "u4", "i4", "u8", "i8"}
    assert {len(c["values"]) for c in CASES} >= {3, 4, 5, 7}
    assert TC.H0 % 16 and TC.W0 % 16 and TC.H0 % 5 == 2                       # partial right and bottom tiles; a last strip of 2 rows


def test_parser_fields(files):
    f = tiff.TiffFile(files["u2 comp5 pred2 tiles"][0])
    assert (f.bigtiff, f.byteorder, len(f.pages), f.n_skipped) == (False, "<", 1, 0)
    pg = f.pages[0]
    assert (pg.width, pg.height, pg.bits, pg.sample_format, pg.compression, pg.predictor, pg.spp, pg.planar, pg.fill_order, pg.subfile) == \
        (TC.W0, TC.H0, [16], [1], 5, 2, 1, 1, 1, 0)
    assert (pg.tiled, pg.seg_w, pg.seg_h, pg.across, pg.down, pg.n_segments) == (True, 16, 16, 5, 3, 15)
    assert pg.dtype == np.dtype("u2") and len(pg.offsets) == len(pg.counts) == 15 and pg.nodata is None
    pg = tiff.TiffFile(files["u2 comp8 pred2 strips"][0]).pages[0]
    assert (pg.tiled, pg.seg_w, pg.seg_h, pg.n_segments) == (False, TC.W0, 5, 8)
    k, y, x, rows, pitch, nbytes = pg.segments()
    assert rows.tolist() == [5] * 7 + [2] and pitch.tolist() == [TC.W0] * 8 and nbytes.tolist() == [5 * TC.W0 * 2] * 7 + [2 * TC.W0 * 2]
    k, y, x, rows, pitch, nbytes = pg.segments((6, 11, 0, 3))                 # rows 6..10: strips 1 and 2 only
    assert k.tolist() == [1, 2]
    big = [c for c in CASES if "MM BigTIFF" in c["name"]][0]
    f = tiff.TiffFile(files[big["name"]][0])
    assert (f.bigtiff, f.byteorder, len(f.pages)) == (True, ">", 4)
    f = tiff.TiffFile(files["overviews and masks skipped"][0])
    assert (len(f.pages), f.n_skipped) == (1, 2) and f.pages[0].index == 0
    st = tiff.TiffStack(files["f4 nodata -9999 seven days"])
    assert st.shape == (7, TC.H0, TC.W0) and st.nodata == -9999.0 and st.attrs == {"_FillValue": -9999.0} and st.dtype == np.float32
    st = tiff.TiffStack(files["i2 nodata -32768"])
    assert st.nodata == -32768 and isinstance(st.nodata, int) and st.attrs == {"_FillValue": -32768}


def test_coordinates(tmp_path):
    a = TC.field("f4", 1)[0]
    lon, lat = TC.expected_coords(TC.W0, TC.H0)
    for name, geo, point in (("area", TC.geo_tags(), False), ("point", TC.geo_tags(point=True), True),
                             ("matrix", TC.geo_tags(transformation=True), False), ("matrix_point", TC.geo_tags(transformation=True, point=True), True)):
        p = TC.write_tiff(str(tmp_path / f"{name}_2020.tif"), [TC.page(a, geo=geo)])
        st = tiff.TiffStack(p)
        elon, elat = TC.expected_coords(TC.W0, TC.H0, point=point)
        np.testing.assert_array_equal(st.longitude, elon)
        np.testing.assert_array_equal(st.latitude, elat)
        assert st.latitude[0] > st.latitude[-1]                               # rows stay in stored order: north first
    assert lon[0] == -100.0 + 0.125 and lat[0] == 50.0 - 0.125               # cell centres for RasterPixelIsArea


def test_times_from_names():
    T = pd.Timestamp
    for name, want in (("PRISM_tmean_stable_4kmD2_20200131_bil.tif", T("2020-01-31")), ("chirps-v2.0.2020.01.05.tif", T("2020-01-05")),
                       ("daymet_v4_prcp_2019-12-31.tiff", T("2019-12-31")), ("tavg_202007.tif", T("2020-07-01")), ("x_1999.tif", T("1999-01-01")),
                       ("v2_2001_06_30_v3.tif", T("2001-06-30")), ("a_19991231_b_2005.tif", T("2005-01-01")), ("/d/20200101/t_18500101.tif", T("1850-01-01"))):
        assert tiff.time_from_name(name) == want, name
    for name in ("wc2.1_2.5m_tavg_01.tif", "tile_123456789.tif", "t_20201345.tif"):
        with pytest.raises(ValueError, match="tiff_time"):
            tiff.time_from_name(name)


def test_tiff_time(files):
    multi = [c for c in CASES if "multi-page" in c["name"]][0]
    paths = files[multi["name"]]
    with pytest.raises(ValueError, match="multi-page.*tiff_time"):
        tiff.TiffStack(paths)
    want = pd.DatetimeIndex(multi["tiff_time"])
    assert tiff.TiffStack(paths, multi["tiff_time"]).time.equals(want)
    assert tiff.TiffStack(paths, lambda p: multi["tiff_time"]).time.equals(want)
    with pytest.raises(ValueError, match="3 timestamps"):
        tiff.TiffStack(paths, multi["tiff_time"][:3])
    daily = files["f4 comp5 pred3 strips"]
    assert tiff.TiffStack(daily).time.equals(pd.DatetimeIndex(["2020-01-01", "2020-01-02", "2020-01-03"]))
    assert tiff.TiffStack(daily, lambda p: "1999-05-0" + os.path.basename(p)[9]).time.equals(pd.DatetimeIndex(["1999-05-01", "1999-05-02", "1999-05-03"]))


# ---------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_read_equals_the_writers_arrays(files, case):
    st = tiff.TiffStack(files[case["name"]], case["tiff_time"])
    assert st.shape == case["values"].shape and st.dtype == case["values"].dtype
    _same_bits(st.read_raw(), case["values"])
    _same_bits(st.read(), _masked(case["values"], case["nodata"]))
    _same_bits(st.read(steps=[len(case["values"]) - 1, 0]), _masked(case["values"][[-1, 0]], case["nodata"]))


@pytest.mark.parametrize("row", GOLDEN, ids=[r["name"] for r in GOLDEN])
def test_read_equals_what_libtiff_wrote(row):
    path = os.path.join(GOLDEN_DIR, row["file"])
    want = np.load(os.path.join(GOLDEN_DIR, row["values"]))
    st = tiff.TiffStack(path, None if row["pages"] == 1 else list(np.datetime64("2020-01-01") + np.arange(row["pages"])))
    pg = st.steps[0]
    assert (pg.compression, pg.predictor, st.dtype.str, st.nodata) == (row["compression"], row["predictor"], row["dtype"], row["nodata"])
    _same_bits(st.read_raw(), want)
    _same_bits(st.read(), _masked(want, row["nodata"]))
    np.testing.assert_array_equal(st.longitude[:2], [10.25, 10.75])
    np.testing.assert_array_equal(st.latitude[:2], [59.75, 59.25])


# The sample types Pillow has a mode for.  Big-endian BigTIFF is left out: Pillow tells BigTIFF by the header's third byte, which is 0
# in "MM\0+", and cannot identify such a file (TiffImagePlugin: `ifh[2] == 43`).
_PILLOW_READS = [c for c in CASES if c["values"].dtype.str[1:] in ("u1", "u2", "i4", "f4") and "MM BigTIFF" not in c["name"]]


@pytest.mark.parametrize("case", _PILLOW_READS, ids=[c["name"] for c in _PILLOW_READS])
def test_pillow_reads_the_writers_files(files, case):
    Image = pytest.importorskip("PIL.Image")
    # libtiff hands Pillow the samples of a compressed big-endian file in native order and Pillow's 32-bit big-endian modes swap them once
    # more: such a page must come back as exactly the byte-swapped values
    swapped = "MM" in case["name"] and case["values"].dtype.itemsize == 4
    t = 0
    for path in files[case["name"]]:
        with Image.open(path) as im:
            n = sum(1 for pages in [c for c in case["files"] if path.endswith(c[0])][0][1] if not pages["subfile"])
            for frame in range(n):
                im.seek(frame)
                got = np.asarray(im)
                want = case["values"][t]
                assert got.shape == want.shape, (path, frame, got.shape)
                got = got.astype(want.dtype)
                assert (got.byteswap() if swapped else got).tobytes() == want.tobytes(), (path, frame)
                t += 1
    assert t == len(case["values"])


# ---------------------------------------------------------------------------------------
# the LZW text on the host
# ---------------------------------------------------------------------------------------
def test_the_stream_catalogue_covers_what_the_issue_lists():
    names = [s[0] for s in STREAMS]
    for word in ("one byte", "run of 70000", "random 16 KiB", "switch 511+0", "switch 1023-1", "switch 2047+1", "no EOI", "KwKwK",
                 "L1 ", "L2 ", "L3 ", "L4 ", "L5 "):
        assert any(word in n for n in names), word
    src = open(os.path.join(ROOT, "aggfly_amd", "csrc", "lzw_passes.h")).read()
    for tag in ("L1", "L2", "L3", "L4", "L5"):                                # every damaged stream names a line of the header
        assert re.search(r"return 1;\s*/\* " + tag + ":", src), tag
    rnd = [s for s in STREAMS if s[0] == "random 16 KiB"][0]
    assert TC.pack_codes([(TC.CLEAR, 12)])[:2] in rnd[1][2:]                 # 16 KiB of random bytes: the table fills and is cleared


def test_lzw_decode_ranges_over_the_stream_catalogue(tmp_path):
    path = str(tmp_path / "streams.bin")
    with open(path, "wb") as f:
        f.write(b"".join(s for _, s, _, _ in STREAMS))
    good = [(i, s) for i, s in enumerate(STREAMS) if s[3] is not None]
    offs = np.concatenate([[0], np.cumsum([len(s[1]) for s in STREAMS])])
    GUARD = 64
    backing = [np.full(s[2] + 2 * GUARD, 0xA5, dtype=np.uint8) for _, s in good]
    outs = [b[GUARD:GUARD + s[2]] for b, (_, s) in zip(backing, good)]
    res = codec.lzw_decode_ranges([(path, int(offs[i]), len(s[1])) for i, s in good], outs, threads=4)
    assert res == [s[2] for _, s in good]
    for b, o, (_, s) in zip(backing, outs, good):
        assert o.tobytes() == s[3], s[0]
        assert (b[:GUARD] == 0xA5).all() and (b[GUARD + s[2]:] == 0xA5).all(), s[0]
    for i, s in enumerate(STREAMS):
        if s[3] is None:
            b = np.full(s[2] + 2 * GUARD, 0xA5, dtype=np.uint8)
            with pytest.raises(codec.CodecError, match="lzw_decode_ranges"):
                codec.lzw_decode_ranges([(path, int(offs[i]), len(s[1]))], [b[GUARD:GUARD + s[2]]], threads=1)
            assert (b[:GUARD] == 0xA5).all() and (b[GUARD + s[2]:] == 0xA5).all(), s[0]
    # a good one beside a damaged one: the batch fails, the good one is still decoded; a range beyond the file is refused
    bad = [i for i, s in enumerate(STREAMS) if s[3] is None][0]
    i0, s0 = good[1]
    out = [np.zeros(s0[2], np.uint8), np.zeros(STREAMS[bad][2], np.uint8)]
    with pytest.raises(codec.CodecError):
        codec.lzw_decode_ranges([(path, int(offs[i0]), len(s0[1])), (path, int(offs[bad]), len(STREAMS[bad][1]))], out, threads=2)
    assert out[0].tobytes() == s0[3]
    with pytest.raises(codec.CodecError):
        codec.lzw_decode_ranges([(path, int(offs[-1]) - 2, 8)], [np.zeros(4, np.uint8)])


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_the_refusal_catalogue_covers_the_list():
    names = " | ".join(r[0] for r in REFUSALS)
    for word in ("compression 7", "compression 32773", "compression 50000", "compression 34887", "compression 50001", "old-style LZW",
                 "FillOrder 2", "12 bits", "predictor 2 on floats", "predictor 3 on integers", "chunky", "planar", "complex", "projected",
                 "rotated", "no georeferencing", "differ in grid", "differ in type", "differ in nodata", "offset leaves", "byte count leaves"):
        assert word in names, word


@pytest.mark.parametrize("item", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_their_reason(tmp_path, item):
    path = TC.write_refusal(item, str(tmp_path))
    with pytest.raises(ValueError, match=re.escape(item[3])) as e:
        tiff.TiffStack(path, tiff_time=lambda p: ["2020-01-01", "2020-01-02"][:len(item[1])])
    assert os.path.basename(path) in str(e.value)
    if item[0].startswith("compression"):
        assert item[0].split()[1] in str(e.value)                              # by number and by name
    with pytest.raises(ValueError, match=re.escape(item[3])):                  # the public path raises it too: a TIFF has no other route
        afio.dataset_from_path(path, "v", tiff_time=lambda p: ["2020-01-01", "2020-01-02"][:len(item[1])])


def test_damaged_directories_are_refused(tmp_path):
    a = TC.field("u2", 1)[0]
    p = TC.write_tiff(str(tmp_path / "ok_2020.tif"), [TC.page(a)])
    raw = open(p, "rb").read()
    cut = str(tmp_path / "cut_2020.tif")
    open(cut, "wb").write(raw[:len(raw) - 40])                                # the directory is at the end of the file
    with pytest.raises(ValueError, match="leave"):
        tiff.TiffStack(cut)
    loop = bytearray(raw)
    first = int.from_bytes(raw[4:8], "little")
    n = int.from_bytes(raw[first:first + 2], "little")
    loop[first + 2 + 12 * n:first + 6 + 12 * n] = first.to_bytes(4, "little")  # the next directory is this one
    lp = str(tmp_path / "loop_2020.tif")
    open(lp, "wb").write(loop)
    with pytest.raises(ValueError, match="circle"):
        tiff.TiffStack(lp)
    assert not tiff.is_tiff(str(tmp_path / "absent.tif")) and tiff.is_tiff(p)


# ---------------------------------------------------------------------------------------
# the C-ABI surface
# ---------------------------------------------------------------------------------------
def test_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "aggfly_hip.h")).read()
    assert "#define AFHIP_ABI_VERSION 4" in hdr and hip.ABI_VERSION == 4       # additive: the ABI version stays
    for name in ("afhip_lzw_decode", "afhip_tiff_place"):
        assert name in hip.EXPORTS and re.search(r"\b" + name + r"\s*\(", hdr), name
    chdr = open(os.path.join(ROOT, "include", "aggfly_codec.h")).read()
    assert "afcodec_lzw_decode_ranges" in codec.EXPORTS and re.search(r"\bafcodec_lzw_decode_ranges\s*\(", chdr)
    assert hasattr(codec.load(), "afcodec_lzw_decode_ranges")
    sizes = {"int64_t": ("<i8", 8), "int32_t": ("<i4", 4)}

    def fields_of(text, name):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                ctype, names = decl.split(None, 1)
                out += [(n.strip(), ctype) for n in names.split(",")]
        return out

    fields = fields_of(hdr, "afhip_tiff_seg")
    assert [(n, sizes[t][0]) for n, t in fields] == [(n, hip.TIFF_SEG[n].str) for n in hip.TIFF_SEG.names]
    assert hip.TIFF_SEG.itemsize == sum(sizes[t][1] for _, t in fields) == 56
    # the passes' own record (lzw_passes.h) has the same fields in the same order
    assert fields_of(open(os.path.join(ROOT, "aggfly_amd", "csrc", "lzw_passes.h")).read(), "lzw_seg") == fields
    assert afio.GPU_DECODE_AUTO_BYTES_LZW is None or afio.GPU_DECODE_AUTO_BYTES_LZW > 0


# ---------------------------------------------------------------------------------------
# the public path, host route
# ---------------------------------------------------------------------------------------
def test_dataset_from_path_on_a_glob(files):
    case = [c for c in CASES if c["name"] == "f4 nodata -9999 seven days"][0]
    d = os.path.dirname(files[case["name"]][0])
    ds = afio.dataset_from_path(os.path.join(d, "v_*.tif"), "tmean")
    assert ds.da.name == "tmean" and set(ds.da.dims) == {"time", "latitude", "longitude"}
    _same_bits(np.asarray(ds.cube()), _masked(case["values"], -9999.0))
    assert pd.DatetimeIndex(ds.da.coords["time"]).equals(pd.date_range("2020-01-01", periods=7))
    lon, lat = TC.expected_coords(TC.W0, TC.H0)
    np.testing.assert_array_equal(np.asarray(ds.da.coords["latitude"], dtype=float), lat)
    # a list, a time selection, and the time coordinate alone
    ds = afio.dataset_from_path(files[case["name"]][2:5], "tmean", time_sel=slice("2020-01-04", "2020-01-05"))
    _same_bits(np.asarray(ds.cube()), _masked(case["values"][3:5], -9999.0))
    assert afio.read_time_coordinate(files[case["name"]][0], "tmean")[0] == pd.Timestamp("2020-01-01")
    # integers with a nodata value: floats with NaN; a multi-page file with tiff_time=
    case = [c for c in CASES if c["name"] == "i2 nodata -32768"][0]
    ds = afio.dataset_from_path(files[case["name"]], "v")
    _same_bits(np.asarray(ds.cube()), _masked(case["values"], -32768))
    multi = [c for c in CASES if "multi-page" in c["name"]][0]
    ds = afio.dataset_from_path(files[multi["name"]][0], "v", tiff_time=multi["tiff_time"])
    _same_bits(np.asarray(ds.cube()), multi["values"])
    with pytest.raises(ValueError, match="tiff_time"):
        afio.dataset_from_path(files[multi["name"]][0], "v")
