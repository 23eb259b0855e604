"""GRIB files on the device route: the unpack kernel (`hip.grib_unpack`) against the expectation of the case writer of
tests/grib_cases.py — bit for bit, NaN positions included, a sentinel everywhere outside the box —, its refusals, and
`dataset_from_path(device="cuda")` on the catalogue with time / space windows and several files."""
import datetime as dt
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_cases as C  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import distributed as D, grib, hip, io as afio  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = C.build_cases()
BY = {c.name: c for c in CASES}
SENTINEL = 0x5A5A5A5A
T, NY, NX = 3, 33, 130                 # a row is no multiple of a wave (64) or of a lane's run (8); 4,290 points cross 32-bit words and 4,096
WIDTHS = (0, 1, 7, 8, 12, 16, 24, 31, 32)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("grib")
    return {c.name: c.write(d) for c in CASES}


@pytest.fixture
def no_host_route(monkeypatch):
    """The host decode is not an answer here."""
    def refuse(*a, **k):
        raise AssertionError("the host route was taken")
    monkeypatch.setattr(afio, "_open_grib", refuse)
    monkeypatch.setattr(grib, "decode_message", refuse)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, a.dtype, b.shape, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fields(nbits, with_map, ny=NY, nx=NX, seed=0):
    """Three steps of ``nbits``-bit values on a ny x nx grid with their expected arrays, computed once: (steps, expected (3, ny, nx))."""
    rng = np.random.default_rng(1000 * nbits + 2 * seed + with_map)
    steps = [C.field(rng, nbits, k, n=ny * nx, bitmap=C.some_bitmap(rng, ny * nx) if with_map else None, E=-2 if nbits < 24 else -12,
                     D=k % 2, R=(-118.625, 273.125, 0.0)[k]) for k in range(T)]
    want = np.stack([s.expected(ny, nx) for s in steps])
    want.setflags(write=False)
    return steps, want


def _pad4(b: bytes) -> bytes:
    return b + b"\x00" * (-len(b) % 4)


def _stage(steps, n_points, first_point=0):
    """The stage of ``steps`` as the route lays it out — per step the bitmap, then the packed bits from value ``first_point`` on (from
    the byte that holds its first bit), each padded to 4 bytes — and the records.  The stage ends with the last step's last word:
    there is no slack behind it."""
    stage, rec = b"", np.zeros(len(steps), dtype=hip.GRIB_STEP)
    for k, s in enumerate(steps):
        r = rec[k]
        r["bitmap_off"] = -1
        if s.bitmap is not None:
            assert first_point == 0
            r["bitmap_off"] = len(stage)
            stage += _pad4(C.pack_bits(s.bitmap, 1)[0])
        data = C.pack_bits(s.X, s.nbits)[0]
        cut = first_point * s.nbits // 8
        r["data_off"], r["data_bytes"], r["first_point"], r["first_bit"] = len(stage), len(data) - cut, first_point, first_point * s.nbits % 8
        r["nbits"], r["R"], r["s"], r["d"] = s.nbits, s.R, 2.0 ** s.E, 10.0 ** -s.D
        stage += _pad4(data[cut:])
    return np.frombuffer(stage if stage else b"\x00" * 4, dtype=np.uint8).copy(), rec


def _run(torch, stage, rec, grid, box, cube_shape, at, n_steps=None):
    """-> (cube as numpy, errors) after one `hip.grib_unpack` into a cube full of the sentinel."""
    n_steps = len(rec) if n_steps is None else n_steps
    cube = torch.full(cube_shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    rank = torch.empty(hip.grib_rank_bytes(n_steps, grid[0] * grid[1]), dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.grib_unpack(torch.from_numpy(stage).cuda(), torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda(), n_steps, grid, box, cube, at, rank, errors)
    torch.cuda.synchronize()
    return cube.cpu().numpy(), int(errors.item())


def _check_box(got, want, box, at):
    y0, x0, ny, nx = box
    t0, cy, cx = at
    inside = np.zeros(got.shape, bool)
    inside[t0:t0 + want.shape[0], cy:cy + ny, cx:cx + nx] = True
    _same_bits(got[inside].reshape(want.shape[0], ny, nx), want[:, y0:y0 + ny, x0:x0 + nx])
    assert (got.view(np.uint32)[~inside] == SENTINEL).all()


@pytest.mark.parametrize("with_map", [False, True], ids=["plain", "bitmap"])
@pytest.mark.parametrize("nbits", WIDTHS)
def test_unpack_against_the_case_writer(torch_cuda, nbits, with_map):
    steps, want = _fields(nbits, with_map)
    stage, rec = _stage(steps, NY * NX)
    assert np.isnan(want).any() == with_map and (nbits == 0 or len(np.unique(want[~np.isnan(want)])) > 2)
    # the whole grid ...
    got, errors = _run(torch_cuda, stage, rec, (NY, NX), (0, 0, NY, NX), (T, NY, NX), (0, 0, 0))
    assert errors == 0
    _same_bits(got, want)
    # ... and the box y 2..31, x 3..127 at an offset in a larger cube
    box, at = (2, 3, 29, 124), (1, 4, 5)
    got, errors = _run(torch_cuda, stage, rec, (NY, NX), box, (T + 2, NY + 7, NX + 11), at)
    assert errors == 0
    _check_box(got, want, box, at)


def test_a_step_staged_from_the_middle_of_its_data(torch_cuda):
    """12-bit values on a grid of odd width staged from row 3 on: a0 * NX = 393 is odd, the first staged bit is bit 4 of its byte."""
    ny, nx, a0 = 33, 131, 3
    steps, want = _fields(12, False, ny, nx)
    stage, rec = _stage(steps, ny * nx, first_point=a0 * nx)
    assert (rec["first_bit"] == 4).all() and (rec["first_point"] == 393).all()
    box, at = (a0, 5, ny - a0 - 2, 120), (0, 0, 0)
    got, errors = _run(torch_cuda, stage, rec, (ny, nx), box, (T, box[2], box[3]), at)
    assert errors == 0
    _check_box(got, want, box, at)
    # a box that begins before the first staged point is refused: nothing to read its first rows from
    got, errors = _run(torch_cuda, stage, rec, (ny, nx), (a0 - 1, 5, 4, 120), (T, 4, 120), at)
    assert errors == T and (got.view(np.uint32) == SENTINEL).all()


def test_three_widths_in_one_batch(torch_cuda):
    steps = [_fields(16, False)[0][0], _fields(12, True)[0][1], _fields(7, False)[0][2]]
    want = np.stack([_fields(16, False)[1][0], _fields(12, True)[1][1], _fields(7, False)[1][2]])
    stage, rec = _stage(steps, NY * NX)
    assert list(rec["nbits"]) == [16, 12, 7] and list(rec["bitmap_off"] >= 0) == [False, True, False]
    box, at = (1, 2, 31, 127), (0, 1, 1)
    got, errors = _run(torch_cuda, stage, rec, (NY, NX), box, (T, NY, NX), at)
    assert errors == 0
    _check_box(got, want, box, at)


def _break(rec, stage, what):
    r = rec[1]
    if what == "data beyond the stage":
        r["data_off"] = len(stage) - 8
    elif what == "data offset beyond the stage":
        r["data_off"] = len(stage) + 4
    elif what == "negative data offset":
        r["data_off"] = -4
    elif what == "negative byte count":
        r["data_bytes"] = -1
    elif what == "33 bits":
        r["nbits"] = 33
    elif what == "negative bits":
        r["nbits"] = -1
    elif what == "first bit 8":
        r["first_bit"] = 8
    elif what == "one byte too few":
        r["data_bytes"] -= 1
    elif what == "bitmap beyond the stage":
        r["bitmap_off"] = len(stage) - (NY * NX + 7) // 8 + 1
    elif what == "bitmap offset -2":
        r["bitmap_off"] = -2
    elif what == "bitmap with a first point":
        r["first_point"] = 1
    elif what == "huge byte count":
        r["data_bytes"] = (1 << 62)
    else:
        raise KeyError(what)


@pytest.mark.parametrize("with_map,what", [(False, "data beyond the stage"), (False, "data offset beyond the stage"), (False, "negative data offset"),
                                           (False, "negative byte count"), (False, "33 bits"), (False, "negative bits"), (False, "first bit 8"),
                                           (False, "one byte too few"), (False, "huge byte count"), (True, "one byte too few"),
                                           (True, "bitmap beyond the stage"), (True, "bitmap offset -2"), (True, "bitmap with a first point"),
                                           (True, "33 bits"), (True, "data beyond the stage")])
def test_a_refused_record_writes_nothing_and_is_counted(torch_cuda, with_map, what):
    steps, want = _fields(12, with_map)
    stage, rec = _stage(steps, NY * NX)
    rec = rec.copy()
    if what == "one byte too few":                                  # (the 12-bit data of 4,290 or fewer values: the last value then ends beyond the bytes)
        assert rec[1]["data_bytes"] == (len(steps[1].X) * 12 + 7) // 8
    _break(rec, stage, what)
    got, errors = _run(torch_cuda, stage, rec, (NY, NX), (0, 0, NY, NX), (T, NY, NX), (0, 0, 0))
    assert errors == 1
    assert (got[1].view(np.uint32) == SENTINEL).all()
    _same_bits(got[0], want[0])
    _same_bits(got[2], want[2])


def test_a_box_that_needs_fewer_bytes_is_served(torch_cuda):
    """The same shortened record is sound for a box that ends before the missing value."""
    steps, want = _fields(12, False)
    stage, rec = _stage(steps, NY * NX)
    rec = rec.copy()
    rec["data_bytes"] -= 1
    box, at = (0, 0, NY - 1, NX), (0, 0, 0)
    got, errors = _run(torch_cuda, stage, rec, (NY, NX), box, (T, NY, NX), at)
    assert errors == 0
    _check_box(got, want, box, at)


def test_the_entry_refuses_what_it_cannot_place(torch_cuda):
    torch = torch_cuda
    steps, want = _fields(16, False)
    stage, rec = _stage(steps, NY * NX)
    for box, shape, at in [((0, 0, NY + 1, NX), (T, NY + 1, NX), (0, 0, 0)), ((0, 1, NY, NX), (T, NY, NX), (0, 0, 0)),       # outside the grid
                           ((-1, 0, 2, 2), (T, NY, NX), (0, 0, 0)), ((0, 0, NY, NX), (T, NY, NX - 1), (0, 0, 0)),                   # ... the cube
                           ((0, 0, NY, NX), (T, NY, NX), (0, 1, 0)), ((0, 0, NY, NX), (T - 1, NY, NX), (0, 0, 0)),
                           ((0, 0, 2, 2), (T, NY, NX), (1, 0, 0)), ((0, 0, 2, 2), (T, NY, NX), (0, 0, -1))]:
        with pytest.raises(ValueError):
            _run(torch, stage, rec, (NY, NX), box, shape, at)
    dev = lambda a: torch.from_numpy(a).cuda()
    rank = torch.empty(hip.grib_rank_bytes(T, NY * NX), dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    recs = dev(rec.view(np.uint8).reshape(-1))
    for cube in (torch.zeros((T, NY, NX), dtype=torch.float64, device="cuda"), torch.zeros((T, NY, NX), dtype=torch.int32, device="cuda"),
                 torch.zeros((T, NY, NX), dtype=torch.float16, device="cuda")):
        with pytest.raises(ValueError):
            hip.grib_unpack(dev(stage), recs, T, (NY, NX), (0, 0, NY, NX), cube, (0, 0, 0), rank, errors)
    cube = torch.full((T, NY, NX), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    with pytest.raises(ValueError, match="4-byte words"):
        hip.grib_unpack(dev(stage)[:-2], recs, T, (NY, NX), (0, 0, NY, NX), cube, (0, 0, 0), rank, errors)
    with pytest.raises(ValueError, match="rank scratch"):
        hip.grib_unpack(dev(stage), recs, T, (NY, NX), (0, 0, NY, NX), cube, (0, 0, 0), rank[:-4], errors)
    with pytest.raises(ValueError):
        hip.grib_unpack(dev(stage), recs[:-8], T, (NY, NX), (0, 0, NY, NX), cube, (0, 0, 0), rank, errors)
    torch.cuda.synchronize()
    assert int(errors.item()) == 0 and bool((cube.view(torch.int32) == SENTINEL).all())
    hip.grib_unpack(dev(stage), recs, T, (NY, NX), (0, 0, 0, NX), cube, (0, 0, 0), rank, errors)          # an empty box: nothing to do
    hip.grib_unpack(dev(stage), recs, 0, (NY, NX), (0, 0, NY, NX), cube, (0, 0, 0), rank, errors)
    torch.cuda.synchronize()
    assert bool((cube.view(torch.int32) == SENTINEL).all())


# ---------------------------------------------------------------------------------------
# the route
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_streams_into_hbm(torch_cuda, case, files, no_host_route):
    ds = af.dataset_from_path(files[case.name], case.var, device="cuda", **case.read_kw)
    cube = ds.cube()
    assert cube.is_cuda and cube.dtype == torch_cuda.float32 and not ds.is_packed
    _same_bits(cube.cpu().numpy(), case.expected)
    assert ds.time.equals(pd.DatetimeIndex(case.times))
    np.testing.assert_array_equal(ds.latitude, case.latitude)
    np.testing.assert_array_equal(ds.longitude, case.longitude)


def test_the_device_route_matches_the_host_route(torch_cuda, files):
    for name in ("e1_varying", "e2_varying", "e1_bitmap_some_missing"):
        host = af.dataset_from_path(files[name], "t2m")
        dev = af.dataset_from_path(files[name], "t2m", device="cuda", engine="cfgrib", keep_packed=True)
        assert not dev.is_packed
        _same_bits(dev.cube().cpu().numpy(), np.asarray(host.cube()))


@pytest.mark.parametrize("name", ["e1_varying", "e2_n12"])
def test_both_staging_buffers_are_reused(torch_cuda, name, files, no_host_route, monkeypatch):
    """Slabs of one or two steps: the 7 steps go through at least three slabs."""
    case = BY[name]
    monkeypatch.setenv("AGGFLY_HIP_SLAB_MB", repr(2.5 * 96 / (1 << 20)))
    calls = []
    real = hip.grib_unpack
    monkeypatch.setattr(hip, "grib_unpack", lambda stage, steps, n, *a: calls.append(n) or real(stage, steps, n, *a))
    ds = af.dataset_from_path(files[name], case.var, device="cuda")
    assert len(calls) >= 3 and sum(calls) == 7, calls
    _same_bits(ds.cube().cpu().numpy(), case.expected)


GRID360 = (C.NI, C.NJ, 50.0, 230.0, 49.0, 232.0, 0x00)


@pytest.fixture(scope="module")
def windows_files(tmp_path_factory):
    """7 hourly steps from 2024-07-15 00:00 on a 5 x 9 grid at 230..232 degrees east: plain 16-bit, 12-bit (rows begin inside bytes),
    and with a bitmap."""
    d = tmp_path_factory.mktemp("gribwin")
    rng = np.random.default_rng(77)
    out = {}
    for name, nbits, with_map, ed in (("plain16", 16, False, 1), ("plain12", 12, False, 2), ("bitmap12", 12, True, 1)):
        steps = [C.field(rng, nbits, k, bitmap=C.some_bitmap(rng) if with_map else None, R=-118.625) for k in range(C.STEPS)]
        case = C.Case(name, "t2m", [(C.message1 if ed == 1 else C.message2)(s, GRID360) for s in steps], steps, grid=GRID360, edition=ed)
        out[name] = (case, case.write(d))
    return out


def _regions():
    # half a cell (0.125 degrees) around rows 1..2 (49.75, 49.5) and columns 1..3 (230.25 .. 230.75)
    return af.GeoRegions(pd.DataFrame({"geoid": ["a"], "minx": [-129.70], "miny": [49.55], "maxx": [-129.30], "maxy": [49.70]}))


TIME_WINDOWS = {"all": ({}, slice(0, 7)), "window": ({"time_window": (2, 5)}, slice(2, 5)), "none": ({"time_window": (0, 0)}, slice(0, 0)),
                "sel": ({"time_sel": slice("2024-07-15 01:00", "2024-07-15 04:00")}, slice(1, 5))}
SPACE_WINDOWS = {"grid": (lambda: {}, slice(0, 5), slice(0, 9)), "regions": (lambda: {"georegions": _regions()}, slice(1, 3), slice(1, 4)),
                 "band": (lambda: {"lat_window": (1, 4)}, slice(1, 4), slice(0, 9))}


@pytest.mark.parametrize("space", list(SPACE_WINDOWS))
@pytest.mark.parametrize("time", list(TIME_WINDOWS))
@pytest.mark.parametrize("name", ["plain16", "plain12", "bitmap12"])
def test_windows_read_the_same_box(torch_cuda, name, time, space, windows_files, no_host_route, monkeypatch):
    case, path = windows_files[name]
    tkw, ts = TIME_WINDOWS[time]
    skw, ys, xs = SPACE_WINDOWS[space]
    staged = []
    real = hip.grib_unpack
    monkeypatch.setattr(hip, "grib_unpack", lambda stage, steps, n, *a: staged.append((stage.numel(), n)) or real(stage, steps, n, *a))
    ds = af.dataset_from_path(path, "t2m", device="cuda", **tkw, **skw())
    cube = ds.cube()
    assert cube.is_cuda
    _same_bits(cube.cpu().numpy(), case.expected[ts, ys, xs])
    np.testing.assert_array_equal(ds.latitude, case.latitude[ys])
    np.testing.assert_array_equal(ds.longitude, case.longitude[xs])
    assert len(ds.time) == ts.stop - ts.start
    if name != "bitmap12" and staged:
        # without a bitmap only the bytes of the box's rows are staged (each step padded to whole words)
        nbits, rows = (16 if name == "plain16" else 12), ys.stop - ys.start
        assert all(nbytes <= n * (rows * C.NI * nbits // 8 + 8) for nbytes, n in staged), staged


def test_several_files_and_preprocess(torch_cuda, tmp_path, no_host_route):
    rng = np.random.default_rng(11)
    steps = [C.field(rng, (16, 12)[k % 2], k, bitmap=C.some_bitmap(rng) if k == 5 else None) for k in range(10)]
    paths = []
    for j, part in enumerate((steps[:4], steps[4:])):
        paths.append(str(tmp_path / f"part{j}.grib"))
        with open(paths[-1], "wb") as f:
            f.write(b"".join(C.message1(s, C.GRID) for s in part))
    want = np.stack([s.expected(C.NJ, C.NI) for s in steps])
    pre = lambda x: x - 273.15
    for p in (paths, str(tmp_path / "part*.grib")):
        ds = af.dataset_from_path(p, "t2m", device="cuda", lon_is_360=False, preprocess=pre)
        assert ds.cube().is_cuda and ds.time.equals(pd.DatetimeIndex([s.valid for s in steps]))
        _same_bits(ds.cube().cpu().numpy(), want - np.float32(273.15))
    ds = af.dataset_from_path(paths, "t2m", device="cuda", lon_is_360=False, time_sel=slice("2024-07-15T02:00", "2024-07-15T06:00"))
    _same_bits(ds.cube().cpu().numpy(), want[2:7])
    assert D._step_bytes(paths[0], "t2m") == C.NJ * C.NI * 4
    assert afio.read_time_coordinate(paths[1], "t2m").equals(pd.DatetimeIndex([s.valid for s in steps[4:]]))


def test_a_file_cut_inside_the_data_is_an_error(torch_cuda, tmp_path):
    """A data section shorter than its grid needs: the route says so instead of unpacking what is not there."""
    rng = np.random.default_rng(4)
    st = C.field(rng, 16, 0)
    short = C.Step(st.X[:-3], 16, st.E, st.D, st.R, None, st.valid)
    path = str(tmp_path / "short.grib")
    with open(path, "wb") as f:
        f.write(C.message1(short, C.GRID))
    with pytest.raises(ValueError, match="data section"):
        af.dataset_from_path(path, "t2m", device="cuda", lon_is_360=False)


# ---------------------------------------------------------------------------------------
# the store routes
# ---------------------------------------------------------------------------------------
def test_store_sharded_streams_a_grib_file_in_windows(torch_cuda, tmp_path, no_host_route, monkeypatch):
    """`aggregate_store_sharded` on one GRIB file (January 30th to February 4th, monthly output; 16-bit messages with a bitmap over the
    ocean) under a budget of two days per window: each window streams its own messages, and the frame equals `aggregate_dataset` on
    the whole dataset exactly (the comparison of tests/test_gpu_netcdf3.py::test_store_sharded_streams_a_classic_file_in_windows)."""
    import types
    from aggfly_amd import engine as eng, synth
    from aggfly_amd.cli import pipeline
    T_, ny, nx = 24 * 6, 10, 12
    cube = synth.temperature_cube(T_, ny, nx, dtype=np.float32, seed=61, ocean_frac=0.1, scattered_nan=30) + np.float32(273.15)
    g = (nx, ny, 50.0, 230.0, 50.0 - 0.25 * (ny - 1), 230.0 + 0.25 * (nx - 1), 0x00)
    msgs = []
    for k in range(T_):
        have = ~np.isnan(cube[k].ravel())
        X = np.round((cube[k].ravel()[have].astype(np.float64) - 250.0) * 256.0).astype(np.int64)
        st = C.Step(X.tolist(), 16, E=-8, D=0, R=250.0, bitmap=[int(b) for b in have], valid=dt.datetime(2000, 1, 30) + dt.timedelta(hours=k))
        msgs.append(C.message1(st, g))
    path = str(tmp_path / "era.grib")
    with open(path, "wb") as f:
        f.write(b"".join(msgs))
    assert pipeline._streams_grib(types.SimpleNamespace(var="t2m", timecoord="time"), path)
    assert not pipeline._streams_grib(types.SimpleNamespace(var="msl", timecoord="time"), path)
    tab = synth.weights_table(ny, nx, 6, seed=62, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}))
    spec = dict(dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": "month"})],
                t=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 3)}),
                   ("aggregate", {"calc": "sum", "groupby": "month"})])
    weights_of = lambda ds: af.weights_from_objects(ds, gr, table=tab)
    pre = lambda x: x - 273.15
    opened = []
    real_open = afio.dataset_from_path
    monkeypatch.setattr(afio, "dataset_from_path", lambda *a, **k: opened.append(k.get("time_window")) or real_open(*a, **k))
    old = eng.config.exact_order
    try:
        eng.config.exact_order = True
        got = D.aggregate_store_sharded(weights_of, path, "t2m", spec, lon_is_360=True, preprocess=pre, max_window_bytes=2 * 24 * ny * nx * 4)
        assert len(opened) >= 2 and opened[0][0] == 0 and opened[-1][1] == T_, opened
        assert all(a[1] == b[0] for a, b in zip(opened, opened[1:])), opened
        whole = real_open(path, "t2m", lon_is_360=True, preprocess=pre, device="cuda")
        assert not whole.is_packed and bool(whole.cube().isnan().any())
        want = af.aggregate_dataset(dataset=whole, weights=weights_of(whole), aggregator_dict=spec)
        assert len(got) == len(want) > 0
        pd.testing.assert_frame_equal(got.reset_index(drop=True), want.reset_index(drop=True), check_exact=True)
    finally:
        eng.config.exact_order = old
