"""Multi-band GeoTIFF files on the host: every file of tests/tiff_band_cases.py's catalogue and every file Pillow's libtiff wrote
(tests/golden/tiff_bands/) through `TiffStack.read_raw` / `read` and `dataset_from_path`, bit for bit against the arrays the writers
started from; `steps=` subsets and what they decode; the time axis from sequences, callables and band descriptions; the refusals; the
C-ABI surface of `afhip_tiff_place_bands`."""
import json
import os
import re
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_band_cases as BC  # noqa: E402
import tiff_cases as TC  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import codec, hip, tiff  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "tiff_bands")
GOLDEN = json.load(open(os.path.join(GOLDEN_DIR, "index.json")))
CASES = BC.band_catalogue()
BY = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiff_bands")
    return {c["name"]: BC.write_case(c, str(d / f"c{i}")) for i, c in enumerate(CASES)}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, a.dtype, b.shape, b.dtype)
    assert a.tobytes() == b.tobytes()


def _masked(values, nodata):
    """What `TiffStack.read` makes of stored values: NaN at nodata; integers with a nodata value become floats."""
    if nodata is None:
        return values
    out = values.astype(np.float32 if values.dtype.itemsize <= 2 else np.float64) if values.dtype.kind != "f" else values.copy()
    out[values == nodata] = np.nan
    return out


# ---------------------------------------------------------------------------------------
# the writer itself
# ---------------------------------------------------------------------------------------
def test_the_catalogue_covers_what_the_issue_lists():
    names = [c["name"] for c in CASES]
    for word in ("chunky B2 ", "chunky B3 ", "chunky B4 ", "chunky B12 ", "chunky B70 ", "planar B3 ", "planar B70 ", " u1 ", " u2 ", " i4 ", " f4 ", " f8 ",
                 " i8 pred2", "pred1", "pred2", "pred3", "comp1", "comp5", "comp8", "strips", "tiles", " MM", " II", "BigTIFF", "two pages x three bands",
                 "two files of 3 and 4 bands", "chunky file beside planar file", "descriptions give the time"):
        assert any(word in n for n in names), word
    assert any(pg["extra"] for c in CASES for f in c["files"] for pg in f[1])


def test_the_writers_predictors_are_libtiffs_on_one_band_and_differ_at_a_stride():
    a = TC.field("f4", 3, height=4, width=9, seed=1)
    for pred in (1, 2, 3):
        v = a if pred == 3 else a.view("u4")
        one = np.ascontiguousarray(v[:1].transpose(1, 2, 0))
        assert BC.apply_band_predictor(one, pred, "<") == TC.apply_predictor(v[0], pred, "<")           # B = 1: the single-band writer's bytes
    three = np.ascontiguousarray(a.transpose(1, 2, 0))
    raw = np.frombuffer(BC.apply_band_predictor(three, 3, "<"), np.uint8).reshape(4, 4, 27)
    # the first three bytes of a row are the most significant bytes of pixel 0's three bands, undifferenced
    _same_bits(raw[:, 0, :3], np.ascontiguousarray(a[:, :, 0].T.astype(">f4")).view(np.uint8).reshape(4, 3, 4)[:, :, 0])


# Pillow has modes for three 8-bit samples, and for four where ExtraSamples names the fourth; it cannot identify a big-endian BigTIFF
_PILLOW_READS = [c for c in CASES if c["name"].startswith("chunky") and c["values"].dtype == np.uint8 and "MM BigTIFF" not in c["name"]
                 and (len(c["values"]) == 3 or (len(c["values"]) == 4 and c["files"][0][1][0]["extra"]))]


@pytest.mark.parametrize("case", _PILLOW_READS, ids=[c["name"] for c in _PILLOW_READS])
def test_pillow_reads_the_writers_chunky_uint8_files(files, case):
    Image = pytest.importorskip("PIL.Image")
    with Image.open(files[case["name"]][0]) as im:
        got = np.asarray(im)
    _same_bits(np.ascontiguousarray(got.transpose(2, 0, 1)), case["values"])


# ---------------------------------------------------------------------------------------
# values
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_read_equals_the_writers_arrays(files, case):
    st = tiff.TiffStack(files[case["name"]], case["tiff_time"])
    assert st.shape == case["values"].shape and st.dtype == case["values"].dtype and len(st.steps) == len(case["values"])
    assert st.time.equals(pd.DatetimeIndex(case["times"]))
    _same_bits(st.read_raw(), case["values"])
    _same_bits(st.read(), _masked(case["values"], case["nodata"]))
    pick = [len(case["values"]) - 1, 0, 1]
    _same_bits(st.read(steps=pick), _masked(case["values"][pick], case["nodata"]))
    # steps are bands in page order, then band order
    want = [(i, b) for i, f in enumerate(case["files"]) for j, pg in enumerate(f[1]) for b in range(len(pg["array"]))]
    assert [s.band for s in st.steps] == [b for _, b in want]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dataset_from_path_equals_the_writers_arrays(files, case):
    ds = af.dataset_from_path(files[case["name"]], "v", lon_is_360=False, tiff_time=case["tiff_time"])
    _same_bits(np.asarray(ds.cube()), _masked(case["values"], case["nodata"]))
    assert ds.time.equals(pd.DatetimeIndex(case["times"]))
    lon, lat = TC.expected_coords(BC.W0, BC.H0)
    np.testing.assert_array_equal(ds.longitude, lon)
    np.testing.assert_array_equal(ds.latitude, lat)


@pytest.mark.parametrize("row", GOLDEN, ids=[r["name"] for r in GOLDEN])
def test_read_equals_what_libtiff_wrote(row):
    path = os.path.join(GOLDEN_DIR, row["file"])
    want = np.load(os.path.join(GOLDEN_DIR, row["values"]))
    tt = BC.days(row["bands"])
    st = tiff.TiffStack(path, tt)
    pg = st.steps[0]
    assert (pg.bands, pg.chunky, pg.compression, pg.predictor, st.nodata) == (row["bands"], True, row["compression"], row["predictor"], row["nodata"])
    _same_bits(st.read_raw(), want)
    _same_bits(st.read(), _masked(want, row["nodata"]))
    ds = af.dataset_from_path(path, "v", lon_is_360=False, tiff_time=tt)
    _same_bits(np.asarray(ds.cube()), _masked(want, row["nodata"]))
    np.testing.assert_array_equal(ds.longitude[:2], [10.25, 10.75])
    np.testing.assert_array_equal(ds.latitude[:2], [59.75, 59.25])


def test_multi_band_files_equal_the_same_values_as_single_pages(files, tmp_path):
    for name in ("chunky B12 f4 pred3 comp8 tiles II BigTIFF", "two files of 3 and 4 bands i2 nodata", "chunky file beside planar file f4 nodata"):
        case = BY[name]
        single = BC.as_single_pages(case, str(tmp_path / name.replace(" ", "_")))
        a = af.dataset_from_path(files[name], "v", lon_is_360=False, tiff_time=case["tiff_time"])
        b = af.dataset_from_path(single, "v", lon_is_360=False, tiff_time=case["tiff_time"])
        _same_bits(np.asarray(a.cube()), np.asarray(b.cube()))
        assert a.time.equals(b.time)


# ---------------------------------------------------------------------------------------
# steps= decode only what they need
# ---------------------------------------------------------------------------------------
def _count_decodes(monkeypatch, st, steps):
    n = []
    for fn in ("decode_ranges", "lzw_decode_ranges"):
        real = getattr(codec, fn)
        monkeypatch.setattr(codec, fn, (lambda real: lambda *a, **k: n.append(len(a[-2])) or real(*a, **k))(real))
    out = st.read_raw(steps=steps)
    monkeypatch.undo()
    return out, sum(n)


def test_steps_of_a_chunky_page_decode_its_segments_once(files, monkeypatch):
    case = BY["two pages x three bands chunky f4 pred3"]
    st = tiff.TiffStack(files[case["name"]], case["tiff_time"])
    got, n = _count_decodes(monkeypatch, st, [2, 0, 1])                       # three bands of page 0: its 15 tiles once
    _same_bits(got, case["values"][[2, 0, 1]])
    assert n == 15
    got, n = _count_decodes(monkeypatch, st, [5, 1])                          # a band of each page
    _same_bits(got, case["values"][[5, 1]])
    assert n == 30
    got, n = _count_decodes(monkeypatch, st, range(6))
    assert n == 30


def test_steps_of_a_planar_page_decode_their_bands_segments_only(files, monkeypatch):
    case = BY["planar B12 i4 pred2 comp8 tiles II"]
    st = tiff.TiffStack(files[case["name"]], case["tiff_time"])
    got, n = _count_decodes(monkeypatch, st, [7, 3])
    _same_bits(got, case["values"][[7, 3]])
    assert n == 2 * 15
    pg = st.steps[7].page
    assert pg.n_segments == 12 * 15 and not pg.chunky
    k = st.steps[7].segments()[0]
    assert k.tolist() == list(range(7 * 15, 8 * 15))                           # TIFF 6.0: band b's segments at b * across * down + k
    k, y, x, rows, pitch, nbytes = st.steps[7].segments((6, 11, 0, 3))
    assert k.tolist() == [7 * 15] and nbytes.tolist() == [16 * 16 * 4]


def test_segments_of_a_chunky_page_count_the_bands(files):
    case = BY["chunky B3 u2 pred2 comp8 strips MM BigTIFF"]
    pg = tiff.TiffFile(files[case["name"]][0]).pages[0]
    assert (pg.bands, pg.chunky, pg.planar, pg.n_segments) == (3, True, 1, 8)
    k, y, x, rows, pitch, nbytes = pg.segments()
    assert pitch.tolist() == [BC.W0] * 8 and nbytes.tolist() == [5 * BC.W0 * 2 * 3] * 7 + [2 * BC.W0 * 2 * 3]


# ---------------------------------------------------------------------------------------
# the predictors at a stride
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,pred", [("u1", 2), ("u2", 2), ("i4", 2), ("i8", 2), ("f4", 3), ("f8", 3), ("f4", 1)])
def test_undo_predictor_at_a_stride(dt, pred):
    for B in (1, 2, 3, 70):
        a = np.ascontiguousarray(BC.field(dt, B, height=3, width=67, seed=B).transpose(1, 2, 0))
        for bo in ("<", ">"):
            raw = np.frombuffer(BC.apply_band_predictor(a, pred, bo), np.uint8).copy()
            got = tiff.undo_predictor(raw, 3, 67, dt, pred, bo, B)
            _same_bits(got, a if B > 1 else a[:, :, 0])


# ---------------------------------------------------------------------------------------
# time
# ---------------------------------------------------------------------------------------
def test_time_from_sequences_and_callables(files):
    case = BY["two files of 3 and 4 bands i2 nodata"]
    paths = files[case["name"]]
    want = pd.DatetimeIndex(case["times"])
    assert tiff.TiffStack(paths, case["times"]).time.equals(want)
    per_file = {paths[0]: case["times"][:3], paths[1]: case["times"][3:]}
    assert tiff.TiffStack(paths, lambda p: per_file[p]).time.equals(want)
    with pytest.raises(ValueError, match="6 timestamps, the stack has 7 steps"):
        tiff.TiffStack(paths, case["times"][:6])
    with pytest.raises(ValueError, match=r"y2002.tif: tiff_time gave 3 timestamp\(s\) for 1 page\(s\) of 4 band\(s\)"):
        tiff.TiffStack(paths, lambda p: case["times"][:3])
    two = BY["two pages x three bands chunky f4 pred3"]
    with pytest.raises(ValueError, match=r"2 timestamp\(s\) for 2 page\(s\) of 6 band\(s\)"):
        tiff.TiffStack(files[two["name"]], lambda p: two["times"][:2])
    assert tiff.TiffStack(files[two["name"]], lambda p: two["times"]).time.equals(pd.DatetimeIndex(two["times"]))
    with pytest.raises(ValueError, match="multi-page.*tiff_time.*band descriptions that hold a date"):
        tiff.TiffStack(files[two["name"]])
    with pytest.raises(ValueError, match="multi-band.*tiff_time.*band descriptions that hold a date"):
        tiff.TiffStack(paths)


def test_time_from_band_descriptions(files, tmp_path):
    for name in ("descriptions give the time chunky", "descriptions give the time planar"):
        case = BY[name]
        st = tiff.TiffStack(files[name])
        assert st.time.equals(pd.DatetimeIndex(case["times"]))
        ds = af.dataset_from_path(files[name][0], "v", lon_is_360=False)
        assert ds.time.equals(pd.DatetimeIndex(case["times"]))
        assert tiff.TiffStack(files[name], BC.days(4)).time.equals(pd.DatetimeIndex(BC.days(4)))      # tiff_time wins
    pg = tiff.TiffFile(files["descriptions give the time planar"][0]).pages[0]
    assert pg.band_descriptions()[1] == "tmean 2019-12-31 & more"
    a = BC.field("u2", 3, seed=1)
    for k, desc in enumerate((["20200101", None, "20200103"], ["20200101", "no date here", "20200103"], None)):
        path = BC.write_band_tiff(str(tmp_path / f"d{k}.tif"), [BC.band_page(a, descriptions=desc)])
        assert tiff.TiffFile(path).pages[0].band_descriptions() == (desc or [None] * 3)
        with pytest.raises(ValueError, match="tiff_time.*or band descriptions that hold a date"):
            tiff.TiffStack(path)
    # single quotes, another order of the attributes, a description of the dataset (no sample): read; a sample beyond the bands: ignored
    xml = ("<GDALMetadata><Item name='DESCRIPTION'>the dataset 1999-01-01</Item><Item role='description' sample='1' name='DESCRIPTION'>b 2001-02-03</Item>"
           '<Item name="DESCRIPTION" sample="0" role="description">a 2001-02-02</Item><Item name="DESCRIPTION" sample="9" role="description">x</Item>'
           '<Item name="OFFSET" sample="0" role="offset">2001-01-01</Item></GDALMetadata>')
    path = BC.write_band_tiff(str(tmp_path / "q.tif"), [BC.band_page(a[:2], tags={42112: (2, xml.encode() + b"\0")})])
    assert tiff.TiffStack(path).time.equals(pd.DatetimeIndex(["2001-02-02", "2001-02-03"]))


def test_the_shared_probe_sees_the_bands_as_steps(files):
    """`io._streamed_source` is what `distributed._step_bytes`, the sharded entry points and the CLI ask: they get the new shape through it."""
    from aggfly_amd import distributed, io as afio
    path = files["descriptions give the time chunky"][0]
    src = afio._streamed_source(path, "v")
    assert src.shape == (4, BC.H0, BC.W0) and src.step_bytes() == BC.H0 * BC.W0 * 4
    assert distributed._step_bytes(path, "v") == BC.H0 * BC.W0 * 4
    case = BY["chunky B70 u2 pred2 comp8 strips MM"]
    src = afio._streamed_source(files[case["name"]], "v", tiff_time=case["tiff_time"])
    assert src.shape == (70, BC.H0, BC.W0) and src.step_bytes() == BC.H0 * BC.W0 * 4               # uint16 becomes float32 in HBM
    assert distributed._step_bytes(files[case["name"]][0], "v") is None                            # no tiff_time there: as for a multi-page file


# ---------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------
def test_mixed_band_types_are_refused_by_name(tmp_path):
    a = BC.field("u2", 3, seed=2)
    for tags, word in (({258: (3, [16, 16, 8])}, "BitsPerSample"), ({339: (3, [1, 2, 1])}, "SampleFormat"), ({258: (3, [16, 16])}, "BitsPerSample holds 2 values"),
                       ({284: (3, [3])}, "PlanarConfiguration 3")):
        path = BC.write_band_tiff(str(tmp_path / "m_20200101.tif"), [BC.band_page(a, tags=tags)])
        with pytest.raises(ValueError, match=word):
            tiff.TiffStack(path, BC.days(3))
        with pytest.raises(ValueError, match=word):
            af.dataset_from_path(path, "v", lon_is_360=False, tiff_time=BC.days(3))
    with pytest.raises(ValueError, match="mixed band types are not read"):
        tiff.TiffStack(BC.write_band_tiff(str(tmp_path / "n.tif"), [BC.band_page(a, tags={258: (3, [16, 32, 16])})]), BC.days(3))


def test_samples_declared_over_the_bytes_of_one_band_name_their_count(tmp_path):
    """tests/tiff_cases.py's two SamplesPerPixel refusals declare three samples over the bytes of one: they fail on their byte counts
    (chunky) and on their number of offsets (planar), and both messages name SamplesPerPixel = 3."""
    items = {i[0]: i for i in TC.refusal_catalogue()}
    for name, word in (("three samples chunky", r"holds 5180 bytes, its samples \(SamplesPerPixel = 3, PlanarConfiguration 1\) need 15540"),
                       ("three samples planar", r"3 strips need as many offsets and byte counts \(SamplesPerPixel = 3, PlanarConfiguration 2\) \(1 and 1")):
        path = TC.write_refusal(items[name], str(tmp_path))
        with pytest.raises(ValueError, match=word):
            tiff.TiffStack(path)
        with pytest.raises(ValueError, match="SamplesPerPixel"):
            af.dataset_from_path(path, "v", lon_is_360=False)
    # pages of one stack may differ in band count and configuration, not in type
    a = BC.field("u2", 5, seed=3)
    ok = BC.write_band_tiff(str(tmp_path / "ok.tif"), [BC.band_page(a[:2]), BC.band_page(a[2:], planar=2)])
    _same_bits(tiff.TiffStack(ok, BC.days(5)).read_raw(), a)
    bad = BC.write_band_tiff(str(tmp_path / "bad.tif"), [BC.band_page(a[:2]), BC.band_page(a[2:].astype("i2"))])
    with pytest.raises(ValueError, match="differs.*type"):
        tiff.TiffStack(bad, BC.days(5))


# ---------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_additive():
    header = open(os.path.join(ROOT, "include", "aggfly_hip.h")).read()
    assert re.search(r"#define\s+AFHIP_ABI_VERSION\s+4\b", header)
    m = re.search(r"int afhip_tiff_place_bands\(([^;]*)\);", header)
    assert m, "afhip_tiff_place_bands is not declared"
    base = re.search(r"int afhip_tiff_place\(([^;]*)\);", header).group(1)
    norm = lambda t: [" ".join(a.split()) for a in t.split(",")]
    args, old = norm(m.group(1)), norm(base)
    assert "int64_t bands" in args and [a for a in args if a != "int64_t bands"] == old       # afhip_tiff_place's arguments and the band count
    assert "afhip_tiff_place_bands" in hip.EXPORTS and "afhip_tiff_place" in hip.EXPORTS
    api = open(os.path.join(ROOT, "aggfly_amd", "csrc", "afhip_api.hip")).read()
    assert 'extern "C" int afhip_tiff_place_bands(' in api
    assert callable(hip.tiff_place_bands)
