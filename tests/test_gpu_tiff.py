"""GeoTIFF stacks on the GPU: `hip.lzw_decode` over the whole stream catalogue of tests/tiff_cases.py in one launch against the host run
of the same text, `hip.tiff_place` against numpy (each predictor, element size, byte order, pitch, boxes that cut tiles, bad arguments),
the public route `dataset_from_path(files, device="cuda")` against the host route bit for bit — strips and tiles, the three
compressions, both LZW routes, windows, regions, overview pages, integers with nodata —, and one `aggregate_dataset` on a seven-day
stack against the oracle."""
import json
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_cases as TC  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import codec, hip, io as afio, tiff  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden", "tiff")
GOLDEN = json.load(open(os.path.join(GOLDEN_DIR, "index.json")))
CASES = TC.file_catalogue()
BY = {c["name"]: c for c in CASES}
STREAMS = TC.stream_catalogue()
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiffs_gpu")
    return {c["name"]: TC.write_case(c, str(d / f"c{i}")) for i, c in enumerate(CASES)}


@pytest.fixture
def no_host_route(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the host route was asked to read a TIFF stack bound for a device")
    monkeypatch.setattr(afio, "_open_tiff", refuse)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, a.dtype, b.shape, b.dtype)
    assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------
# hip.lzw_decode
# ---------------------------------------------------------------------------------------
def test_lzw_decode_the_stream_catalogue_in_one_launch(torch_cuda, tmp_path):
    torch = torch_cuda
    # the host run of the same text, stream by stream (a damaged one raises)
    path = str(tmp_path / "streams.bin")
    with open(path, "wb") as f:
        f.write(b"".join(s[1] for s in STREAMS))
    offs = np.concatenate([[0], np.cumsum([len(s[1]) for s in STREAMS])])
    host = []
    for i, s in enumerate(STREAMS):
        out = np.zeros(s[2], np.uint8)
        try:
            codec.lzw_decode_ranges([(path, int(offs[i]), len(s[1]))], [out], threads=1)
            host.append(out)
        except codec.CodecError:
            host.append(None)
    assert [h is None for h in host] == [s[3] is None for s in STREAMS]
    # one stage (streams at odd offsets, a byte between them), one decoded buffer with guard bytes around every output
    rec = np.zeros(len(STREAMS), dtype=hip.TIFF_SEG)
    stage, at, dec_at = bytearray(b"\xee"), 1, GUARD
    for i, s in enumerate(STREAMS):
        rec[i]["src_off"], rec[i]["src_bytes"], rec[i]["dec_off"], rec[i]["dec_bytes"] = len(stage), len(s[1]), dec_at, s[2]
        stage += s[1] + b"\xee"
        dec_at += s[2] + GUARD
    rec["bad"] = 7                                                            # the kernel sets and clears it
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    out = torch.full((dec_at,), FILL, dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    recs = dev(rec.view(np.uint8).reshape(-1))
    hip.lzw_decode(dev(np.frombuffer(bytes(stage), np.uint8)), recs, len(STREAMS), out, errors)
    torch.cuda.synchronize()
    got, after = out.cpu().numpy(), recs.cpu().numpy().view(hip.TIFF_SEG)
    n_bad = sum(h is None for h in host)
    assert int(errors.item()) == n_bad and n_bad >= 8
    want = np.full(dec_at, FILL, np.uint8)
    for r, h in zip(rec, host):
        if h is not None:
            want[r["dec_off"]:r["dec_off"] + r["dec_bytes"]] = h               # a damaged stream's output stays untouched
    for r, s in zip(rec, STREAMS):
        a, b = int(r["dec_off"]), int(r["dec_off"] + r["dec_bytes"])
        assert got[a:b].tobytes() == want[a:b].tobytes(), s[0]
        assert (got[a - GUARD:a] == FILL).all() and (got[b:b + GUARD] == FILL).all(), s[0]
    assert got.tobytes() == want.tobytes()
    assert after["bad"].tolist() == [int(h is None) for h in host]


def test_lzw_decode_refuses_records_that_leave_the_buffers(torch_cuda):
    torch = torch_cuda
    s = [x for x in STREAMS if x[0] == "smooth 6000"][0]
    stage = torch.from_numpy(np.frombuffer(s[1], np.uint8).copy()).cuda()
    rec = np.zeros(6, dtype=hip.TIFF_SEG)
    rec["src_bytes"], rec["dec_bytes"] = len(s[1]), s[2]
    rec[1]["src_off"] = 1                                                     # the stream would leave the stage
    rec[2]["src_bytes"] = -1
    rec[3]["dec_off"] = 1                                                     # the output would leave the decoded buffer
    rec[4]["dec_bytes"] = 1 << 40
    rec[5]["dec_off"] = -8
    out = torch.full((s[2],), FILL, dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    recs = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    hip.lzw_decode(stage, recs[56:], 5, out, errors)
    torch.cuda.synchronize()
    assert int(errors.item()) == 5 and bool((out == FILL).all())
    assert recs.cpu().numpy().view(hip.TIFF_SEG)["bad"].tolist() == [0, 1, 1, 1, 1, 1]
    hip.lzw_decode(stage, recs, 1, out, errors)
    hip.lzw_decode(stage, recs, 0, out, errors)
    torch.cuda.synchronize()
    assert int(errors.item()) == 5 and out.cpu().numpy().tobytes() == s[3]
    with pytest.raises(ValueError, match="records"):
        hip.lzw_decode(stage, recs[:100], 2, out, errors)
    with pytest.raises(ValueError, match="one device"):
        hip.lzw_decode(stage, recs.cpu(), 1, out, errors)


# ---------------------------------------------------------------------------------------
# hip.tiff_place
# ---------------------------------------------------------------------------------------
def _segments(values, tile, rows_per_strip, predictor, byteorder, junk_seed=3):
    """The decoded segments of the pages ``values`` (T, H, W) as a writer lays them out: -> (decoded bytes, records)."""
    T, H, W = values.shape
    E = values.dtype.itemsize
    rng = np.random.default_rng(junk_seed)
    blob, recs = bytearray(), []
    for t in range(T):
        if tile:
            tw, th = tile
            PH, PW = -(-H // th) * th, -(-W // tw) * tw
            padded = rng.integers(0, 256, PH * PW * E, dtype=np.uint8).view(values.dtype).reshape(PH, PW).copy()
            padded[:H, :W] = values[t]
            segs = [(y, x, padded[y:y + th, x:x + tw]) for y in range(0, PH, th) for x in range(0, PW, tw)]
        else:
            segs = [(y, 0, values[t, y:y + rows_per_strip]) for y in range(0, H, rows_per_strip)]
        for y, x, s in segs:
            raw = TC.apply_predictor(np.ascontiguousarray(s), predictor, byteorder)
            recs.append((len(blob), len(raw), s.shape[0], s.shape[1], t, y, x))
            blob += raw
    rec = np.zeros(len(recs), dtype=hip.TIFF_SEG)
    for i, (off, nb, rows, pitch, t, y, x) in enumerate(recs):
        rec[i]["dec_off"], rec[i]["dec_bytes"], rec[i]["rows"], rec[i]["pitch"], rec[i]["t"], rec[i]["y"], rec[i]["x"] = off, nb, rows, pitch, t, y, x
    return np.frombuffer(bytes(blob), np.uint8).copy(), rec


def _place(torch, values, blob, rec, predictor, swap, box, at=(0, 0, 0), cube_shape=None, order=None):
    """-> (cube as numpy in the values' type, errors): the cube starts as FILL bytes."""
    T, H, W = values.shape
    y0, x0, ny, nx = box
    shape = cube_shape or (T, ny, nx)
    E = values.dtype.itemsize
    tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[E]
    cube = torch.full((int(np.prod(shape)) * E,), FILL, dtype=torch.uint8, device="cuda").view(tdt).view(shape)
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    if order is not None:
        rec = rec[order]
    hip.tiff_place(torch.from_numpy(blob).cuda(), torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda(), len(rec), int(rec["rows"].max()),
                   predictor, swap, cube, box, at, errors)
    torch.cuda.synchronize()
    return cube.cpu().numpy().view(values.dtype), int(errors.item())


PLACE_TYPES = [("u1", 2), ("i1", 1), ("u2", 2), ("i2", 2), ("u4", 2), ("f4", 3), ("f4", 1), ("u8", 2), ("i8", 1), ("f8", 3)]


@pytest.mark.parametrize("byteorder", ["<", ">"])
@pytest.mark.parametrize("dt,predictor", PLACE_TYPES, ids=[f"{d}-pred{p}" for d, p in PLACE_TYPES])
def test_tiff_place_tiles_and_strips_against_numpy(torch_cuda, dt, predictor, byteorder):
    """37 x 70 in 16 x 16 tiles (partial right and bottom tiles, junk in their padding) and in strips of 5 rows (a last strip of 2), three
    pages: the whole image, and boxes that cut tiles, into a larger cube at an offset."""
    values = TC.field(dt, 3, seed=5)
    swap = byteorder == ">" and values.dtype.itemsize > 1
    fill = np.frombuffer(bytes([FILL]) * 8, dtype=values.dtype)[0]
    for tile, rps in (((16, 16), None), (None, 5)):
        blob, rec = _segments(values, tile, rps, predictor, byteorder)
        got, err = _place(torch_cuda, values, blob, rec, predictor, swap, (0, 0, TC.H0, TC.W0))
        assert err == 0
        _same_bits(got, values)
        for box in ((3, 9, 20, 41), (15, 15, 2, 2), (16, 16, 16, 16), (0, 69, 37, 1), (36, 0, 1, 70)):
            y0, x0, ny, nx = box
            got, err = _place(torch_cuda, values, blob, rec, predictor, swap, box, at=(1, 2, 3), cube_shape=(5, ny + 4, nx + 5),
                              order=np.random.default_rng(1).permutation(len(rec)))
            want = np.full((5, ny + 4, nx + 5), fill, dtype=values.dtype)
            want[1:4, 2:2 + ny, 3:3 + nx] = values[:, y0:y0 + ny, x0:x0 + nx]
            assert err == 0
            _same_bits(got, want)                                             # nothing outside the box is written


@pytest.mark.parametrize("width", [1, 63, 64, 65, 129, 257])
def test_tiff_place_row_widths_carry_the_scan(torch_cuda, width):
    for dt, predictor, bo in (("u2", 2, "<"), ("u2", 2, ">"), ("i1", 2, "<"), ("u4", 2, ">"), ("u8", 2, "<"), ("f4", 3, "<"), ("f8", 3, ">")):
        values = TC.field(dt, 2, height=6, width=width, seed=width)
        swap = bo == ">" and values.dtype.itemsize > 1
        blob, rec = _segments(values, None, 4, predictor, bo)
        got, err = _place(torch_cuda, values, blob, rec, predictor, swap, (0, 0, 6, width))
        assert err == 0
        _same_bits(got, values)
        # a tile wider than the image: the padding columns are part of the sum and of the plane stride
        blob, rec = _segments(values, (width + 15, 8), None, predictor, bo)
        got, err = _place(torch_cuda, values, blob, rec, predictor, swap, (0, 0, 6, width))
        assert err == 0
        _same_bits(got, values)


def test_tiff_place_refuses_bad_arguments_and_skips_bad_records(torch_cuda):
    torch = torch_cuda
    values = TC.field("f4", 2, seed=8)
    blob, rec = _segments(values, (16, 16), None, 3, "<")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dec, recs = dev(blob), dev(rec.view(np.uint8).reshape(-1))
    cube = torch.full((2, TC.H0, TC.W0), 7, dtype=torch.int32, device="cuda").view(torch.float32)
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    n, box = len(rec), (0, 0, TC.H0, TC.W0)
    with pytest.raises(ValueError, match="predictor"):
        hip.tiff_place(dec, recs, n, 16, 4, False, cube, box, (0, 0, 0), errors)
    with pytest.raises(ValueError, match="floating-point predictor"):
        hip.tiff_place(dec, recs, n, 16, 3, False, cube.view(torch.int16), box, (0, 0, 0), errors)
    with pytest.raises(ValueError, match="box outside the cube"):
        hip.tiff_place(dec, recs, n, 16, 3, False, cube, (0, 0, TC.H0 + 1, TC.W0), (0, 0, 0), errors)
    with pytest.raises(ValueError, match="box outside the cube"):
        hip.tiff_place(dec, recs, n, 16, 3, False, cube, box, (0, 1, 0), errors)
    with pytest.raises(ValueError, match="box outside the cube"):
        hip.tiff_place(dec, recs, n, 16, 3, False, cube, box, (3, 0, 0), errors)
    with pytest.raises(ValueError, match="records"):
        hip.tiff_place(dec, recs[:-8], n, 16, 3, False, cube, box, (0, 0, 0), errors)
    with pytest.raises(ValueError, match="one device"):
        hip.tiff_place(dec, recs, n, 16, 3, False, cube, box, (0, 0, 0), errors.cpu())
    with pytest.raises(ValueError, match="aligned"):
        hip.tiff_place(dec[1:], recs, n, 16, 3, False, cube, box, (0, 0, 0), errors)
    hip.tiff_place(dec, recs, 0, 16, 3, False, cube, box, (0, 0, 0), errors)
    hip.tiff_place(dec, recs, n, 16, 3, False, cube, (0, 0, 0, TC.W0), (0, 0, 0), errors)        # an empty box: nothing to do
    torch.cuda.synchronize()
    assert int(errors.item()) == 0 and bool((cube.view(torch.int32) == 7).all())
    # records: one flagged bad (skipped, not counted), three unsound (not placed, counted once each); the rest are placed
    r = rec.copy()
    r[0]["bad"] = 1
    r[1]["dec_off"] = len(blob) - 8                                           # its samples leave the decoded buffer
    r[2]["dec_off"] += 2                                                      # not a multiple of the element size
    r[3]["t"] = 2                                                             # a step the cube does not have
    hip.tiff_place(dec, dev(r.view(np.uint8).reshape(-1)), n, 16, 3, False, cube, box, (0, 0, 0), errors)
    torch.cuda.synchronize()
    assert int(errors.item()) == 3
    got = cube.cpu().numpy()
    want = values.copy()
    for k in range(4):                                                        # (tiles 0..3 of page 0: the first row of tiles)
        want[0, 0:16, 16 * k:16 * k + 16] = np.frombuffer(np.int32(7).tobytes(), np.float32)[0]
    _same_bits(got, want)


# ---------------------------------------------------------------------------------------
# the public route
# ---------------------------------------------------------------------------------------
def _host_as(host, dtype):
    """The host route's cube in the type of the device cube: stored integers without a nodata value stay integers on the host and are
    floats in HBM (float32 up to 16 bits, float64 beyond), the exact conversion of every other container's streaming route."""
    host = np.asarray(host)
    return host if host.dtype == dtype else host.astype(dtype)


def _is_lzw(case):
    return all(pg["compression"] == 5 for f in case["files"] for pg in f[1] if not pg["subfile"])


# every case with the host team decoding, and the LZW stacks once more with the streams decoded in HBM
ROUTES = [(c, "0") for c in CASES] + [(c, "1") for c in CASES if _is_lzw(c)]


@pytest.mark.parametrize("case,gpu_decode", ROUTES, ids=[f"{c['name']}-gpu_decode{m}" for c, m in ROUTES])
def test_every_case_streams_into_hbm(torch_cuda, case, files, gpu_decode, no_host_route, monkeypatch):
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", gpu_decode)
    calls = []
    real = hip.lzw_decode
    monkeypatch.setattr(hip, "lzw_decode", lambda *a: calls.append(a[2]) or real(*a))
    kw = dict(device="cuda", lon_is_360=False, tiff_time=case["tiff_time"])
    if case["values"].dtype.str[1:] in ("u4", "u8"):
        with pytest.raises(ValueError, match="no device representation"):
            af.dataset_from_path(files[case["name"]], "v", **kw)
        return
    ds = af.dataset_from_path(files[case["name"]], "v", **kw)
    cube = ds.cube()
    assert cube.is_cuda and not ds.is_packed and (len(calls) > 0) == (gpu_decode == "1")
    monkeypatch.undo()
    host = af.dataset_from_path(files[case["name"]], "v", lon_is_360=False, tiff_time=case["tiff_time"])
    got = cube.cpu().numpy()
    _same_bits(got, _host_as(host.cube(), got.dtype))                          # NaN positions included: the bits are compared
    if case["nodata"] is not None:
        assert np.isnan(got).any() and np.isnan(got).tobytes() == (case["values"] == case["nodata"]).tobytes()
    assert ds.time.equals(host.time)
    np.testing.assert_array_equal(ds.latitude, host.latitude)
    np.testing.assert_array_equal(ds.longitude, host.longitude)


GOLDEN_ROUTES = [(r, "0") for r in GOLDEN] + [(r, "1") for r in GOLDEN if r["compression"] == 5]


@pytest.mark.parametrize("row,gpu_decode", GOLDEN_ROUTES, ids=[f"{r['name']}-gpu_decode{m}" for r, m in GOLDEN_ROUTES])
def test_files_libtiff_wrote_stream_into_hbm(torch_cuda, row, gpu_decode, no_host_route, monkeypatch):
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", gpu_decode)
    want = np.load(os.path.join(GOLDEN_DIR, row["values"]))
    tt = None if row["pages"] == 1 else list(np.datetime64("2020-01-01") + np.arange(row["pages"]))
    ds = af.dataset_from_path(os.path.join(GOLDEN_DIR, row["file"]), "v", device="cuda", lon_is_360=False, tiff_time=tt)
    exp = want.astype(np.float32) if want.dtype.kind != "f" else want.copy()
    if row["nodata"] is not None:
        exp[want == row["nodata"]] = np.nan
    _same_bits(ds.cube().cpu().numpy(), exp)


def _regions():
    # rows 10..20 (centres 47.375 .. 44.875 N) and columns 20..40 (94.875 .. 89.875 W) of the catalogue's grid: a box that cuts tiles
    return af.GeoRegions(pd.DataFrame({"geoid": ["a"], "minx": [-94.95], "miny": [44.80], "maxx": [-89.80], "maxy": [47.45]}))


TIME_WINDOWS = {"all": {}, "window": {"time_window": (2, 6)}, "none": {"time_window": (0, 0)}, "sel": {"time_sel": slice("2020-01-02", "2020-01-04")}}
SPACE_WINDOWS = {"grid": lambda: {}, "regions": lambda: {"georegions": _regions()}, "band": lambda: {"lat_window": (9, 23)},
                 "regions+band": lambda: {"georegions": _regions(), "lat_window": (2, 7)}}
# LZW tiles of floats on both LZW routes; Deflate strips of integers; both with nodata.  (name, AGGFLY_HIP_GPU_DECODE, what reads, where its locators are)
WINDOW_CASES = [("f4 nodata -9999 seven days", "0", "lzw_decode_ranges", 0), ("f4 nodata -9999 seven days", "1", "read_packed", 0),
                ("i2 nodata -32768", "0", "decode_ranges", 1)]


@pytest.mark.parametrize("space", list(SPACE_WINDOWS))
@pytest.mark.parametrize("time", list(TIME_WINDOWS))
@pytest.mark.parametrize("name,gpu_decode,reader,arg", WINDOW_CASES, ids=[f"{c[0]}-gpu_decode{c[1]}" for c in WINDOW_CASES])
def test_windows_read_what_the_host_route_reads(torch_cuda, files, name, gpu_decode, reader, arg, time, space, monkeypatch):
    time_kw = {"time_window": (1, 4)} if name.startswith("i2") and time == "window" else TIME_WINDOWS[time]      # (the i2 stack has five days)
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", gpu_decode)
    read = []
    real = getattr(codec, reader)
    monkeypatch.setattr(codec, reader, lambda *a, **k: read.append(len(a[arg])) or real(*a, **k))
    kw = dict(lon_is_360=False, **time_kw, **SPACE_WINDOWS[space]())
    ds = af.dataset_from_path(files[name], "v", device="cuda", **kw)
    n_read = sum(read)
    monkeypatch.undo()
    cube = ds.cube()
    assert cube.is_cuda
    if time == "none":
        assert cube.shape[0] == len(ds.time) == 0 and n_read == 0
        return
    host = af.dataset_from_path(files[name], "v", **kw)
    _same_bits(cube.cpu().numpy(), np.asarray(host.cube()))
    assert ds.time.equals(host.time)
    np.testing.assert_array_equal(ds.latitude, host.latitude)
    np.testing.assert_array_equal(ds.longitude, host.longitude)
    T = len(ds.time)
    if space == "grid":
        assert cube.shape[1:] == (TC.H0, TC.W0)
    else:
        assert cube.shape[1] < TC.H0
        # only the strips or tiles that touch the box are read: fewer than every segment of the steps read
        per_page = 15 if "f4" in name else 8
        assert 0 < n_read < T * per_page, (n_read, T)


def test_slabs_of_two_steps_and_overview_pages(torch_cuda, files, no_host_route, monkeypatch):
    case = BY["f4 nodata -9999 seven days"]
    monkeypatch.setenv("AGGFLY_HIP_SLAB_MB", repr(2.5 * 15 * 16 * 16 * 4 / (1 << 20)))          # (a step stages its 15 whole tiles)
    for mode in ("0", "1"):
        monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
        calls = []
        real = hip.tiff_place
        monkeypatch.setattr(hip, "tiff_place", lambda dec, recs, n, *a: calls.append(n) or real(dec, recs, n, *a))
        ds = af.dataset_from_path(files[case["name"]], "v", device="cuda", lon_is_360=False)
        monkeypatch.setattr(hip, "tiff_place", real)
        assert len(calls) >= (3 if mode == "0" else 2) and sum(calls) == 7 * 15, calls       # (compressed steps are smaller: more of them to a slab)
        want = case["values"].copy()
        want[case["values"] == -9999.0] = np.nan
        _same_bits(ds.cube().cpu().numpy(), want)
    cog = BY["overviews and masks skipped"]
    ds = af.dataset_from_path(files[cog["name"]], "v", device="cuda", lon_is_360=False)
    _same_bits(ds.cube().cpu().numpy(), cog["values"])
    assert ds.time.equals(pd.DatetimeIndex(["2021-01-01", "2022-01-01", "2023-01-01"]))


def test_a_damaged_segment_in_a_file_is_an_error(torch_cuda, files, tmp_path, monkeypatch):
    src = files["f4 comp5 pred3 tiles"][0]
    pg = tiff.TiffFile(src).pages[0]
    raw = bytearray(open(src, "rb").read())
    k = 7
    raw[int(pg.offsets[k]) + 2:int(pg.offsets[k]) + 6] = b"\xff\xff\xff\xff"        # codes above the next free one
    path = str(tmp_path / "damaged_20200101.tif")
    open(path, "wb").write(raw)
    for mode, word in (("0", "lzw_decode_ranges"), ("1", "refused by the kernels")):
        monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
        with pytest.raises(ValueError, match=word):
            af.dataset_from_path(path, "v", device="cuda", lon_is_360=False)


def test_aggregate_dataset_on_a_seven_day_stack_against_the_oracle(torch_cuda, tmp_path, no_host_route):
    """`test_gpu_api.test_whole_path_c2_against_oracle`'s spec and tolerance (float32 storage against the reference run on the float64
    cast of the same values), the cube streamed from seven daily LZW + predictor 3 files."""
    from aggfly_amd import synth
    from oracle import ref_aggregate as ra
    spec = dict(
        dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": "month"})],
        tavg=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 5)}),
              ("aggregate", {"calc": "sum", "groupby": "month"})],
    )
    T, ny, nx, R = 7, 12, 20, 13
    cube = synth.temperature_cube(T, ny, nx, dtype=np.float32, seed=21, ocean_frac=0.08, scattered_nan=10)
    stored = np.where(np.isnan(cube), np.float32(-9999.0), cube).astype(np.float32)
    geo = TC.geo_tags(lon0=-120.0, lat0=33.0)
    time = pd.date_range("2001-01-28", periods=T, freq="D")                  # (the month ends inside the stack)
    paths = [TC.write_tiff(str(tmp_path / f"tmean_{day.strftime('%Y%m%d')}.tif"),
                           [TC.page(stored[t], compression=5, predictor=3, tile=(16, 16), nodata="-9999", geo=geo)]) for t, day in enumerate(time)]
    ds = af.dataset_from_path(paths, "tmean", device="cuda", lon_is_360=False)
    lon, lat = TC.expected_coords(nx, ny, lon0=-120.0, lat0=33.0)
    assert ds.time.equals(time)
    tab = synth.weights_table(ny, nx, R, seed=22, secondary=True, zero_frac=0.1)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}), regionid="geoid")
    w = af.weights_from_objects(ds, gr, table=tab)
    got = af.aggregate_dataset(dataset=ds, weights=w, **spec)
    ods = ra.ODataset(cube.astype(np.float64), time, lat, lon, False)
    ow = ra.OWeights(tab, np.arange(ny * nx), gr.shp["geoid"], "geoid", "nan")
    want = ra.aggregate_dataset(ow, ods, engine="numba", **spec)
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    assert (got["geoid"].values == want["geoid"].values).all() and (got["time"].values == want["time"].values).all()
    cols = [c for c in got.columns if c not in ("geoid", "time")]
    np.testing.assert_allclose(got[cols].values, want[cols].values, rtol=1e-10, atol=0, equal_nan=True)
