"""GRIB2 complex packing (templates 5.2 / 5.3) on the device route: the entry `hip.grib_unpack_complex` against the expectation of the
case writer of tests/grib_complex_cases.py — bit for bit, NaN positions included, a sentinel everywhere outside the box —, across the
seams of its passes (the scan's tiles, the tile sums' rounds, the group scan's carry), its refusals, and
`dataset_from_path(device="cuda")` on the catalogue with windows, a file of mixed packings, and the sharded store route.  Every
comparison is exact: no tolerance is involved."""
import datetime as dt
import functools
import os
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_cases as C  # noqa: E402
import grib_complex_cases as K  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import distributed as D, grib, hip, io as afio  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = K.build_cases()
BY = {c.name: c for c in CASES}
SENTINEL = 0x5A5A5A5A
TILE = 2048                              # int64 elements of one tile of the running sums (16 KiB)
FORMS = {"5.2": (2, 0), "order1": (3, 1), "order2": (3, 2)}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gribc")
    return {c.name: c.write(d) for c in CASES}


@pytest.fixture(scope="module")
def host(files):
    """What the host route reads of every case, computed once (before any test disables that route)."""
    out = {}
    for c in CASES:
        a = grib.GribFile(files[c.name]).read(c.var)
        a.setflags(write=False)
        out[c.name] = a
    return out


@pytest.fixture
def no_host_route(monkeypatch):
    """The host decode is not an answer here."""
    def refuse(*a, **k):
        raise AssertionError("the host route was taken")
    monkeypatch.setattr(afio, "_open_grib", refuse)
    monkeypatch.setattr(grib, "decode_message", refuse)
    monkeypatch.setattr(grib, "unpack_complex", refuse)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, a.dtype, b.shape, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------
# the entry
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _field(form, with_map, ny, nx, seed=0, mean=6, **kw):
    """One step of ``form`` on a ny x nx grid with its expected array, computed once: (step, expected (ny, nx))."""
    tmpl, order = FORMS[form]
    rng = np.random.default_rng(100 * ny + nx + 7 * seed + with_map + 3 * order)
    bm = C.some_bitmap(rng, ny * nx) if with_map else None
    n = ny * nx if bm is None else sum(bm)
    st = K.CStep(K.smooth(rng, n, 0 if tmpl == 2 else -3000, 3000), K.cut(rng, n, mean), tmpl, order, extra=2, E=-2 - seed, D=seed % 2,
                 R=(-118.625, 273.125, 0.5)[seed % 3], bitmap=bm, **dict(kw))
    want = st.expected(ny, nx)
    want.setflags(write=False)
    return st, want


def _pad4(b: bytes) -> bytes:
    return b + b"\x00" * (-len(b) % 4)


def _stage(steps):
    """The stage of ``steps`` as the route lays it out — per step the bitmap, then the body of section 7, each padded to 4 bytes — and
    the records.  The stage ends with the last step's last word: there is no slack behind it."""
    stage, rec = b"", np.zeros(len(steps), dtype=hip.GRIB_CSTEP)
    for k, s in enumerate(steps):
        r = rec[k]
        r["bitmap_off"] = -1
        if s.bitmap is not None:
            r["bitmap_off"] = len(stage)
            stage += _pad4(C.pack_bits(s.bitmap, 1)[0])
        r["data_off"], r["data_bytes"], r["n_values"], r["n_groups"] = len(stage), len(s.body), len(s.X), len(s.lens)
        r["ref_len"], r["last_len"], r["nbits_ref"], r["ref_width"], r["nbits_width"] = s.ref_len, s.last_len, s.nbits_ref, s.ref_width, s.nbits_width
        r["len_inc"], r["nbits_len"], r["order"], r["extra"] = s.len_inc, s.nbits_len, s.order, s.extra if s.template == 3 else 0
        r["R"], r["s"], r["d"] = s.R, 2.0 ** s.E, 10.0 ** -s.D
        stage += _pad4(s.body)
    return np.frombuffer(stage if stage else b"\x00" * 4, dtype=np.uint8).copy(), rec


def _run(torch, stage, rec, order, grid, box, cube_shape, at, max_groups=None):
    """-> (cube as numpy, errors) after one `hip.grib_unpack_complex` into a cube full of the sentinel."""
    n = len(rec)
    max_groups = int(max(rec["n_groups"].max(), 0)) if max_groups is None else max_groups
    cube = torch.full(cube_shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    scratch = torch.empty(hip.grib_complex_scratch_bytes(n, grid[0] * grid[1], max_groups), dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.grib_unpack_complex(torch.from_numpy(stage).cuda(), torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda(), n, order, max_groups, grid, box,
                            cube, at, scratch, errors)
    torch.cuda.synchronize()
    return cube.cpu().numpy(), int(errors.item())


def _check_box(got, want, box, at):
    y0, x0, ny, nx = box
    t0, cy, cx = at
    inside = np.zeros(got.shape, bool)
    inside[t0:t0 + want.shape[0], cy:cy + ny, cx:cx + nx] = True
    _same_bits(got[inside].reshape(want.shape[0], ny, nx), want[:, y0:y0 + ny, x0:x0 + nx])
    assert (got.view(np.uint32)[~inside] == SENTINEL).all()


# N = 2 T + 3 values on one row (4,099 is prime): odd, so the running sums take their element-wise path, and the third tile is cut short;
# 37 x 111 = 4,107 the same on a grid that has rows to clip; 33 x 130 = 4,290 even: the 16-byte path.
@pytest.mark.parametrize("ny,nx", [(1, 2 * TILE + 3), (37, 111), (33, 130)], ids=["4099_odd", "37x111_odd", "33x130_even"])
@pytest.mark.parametrize("with_map", [False, True], ids=["plain", "bitmap"])
@pytest.mark.parametrize("form", list(FORMS))
def test_unpack_against_the_case_writer(torch_cuda, form, with_map, ny, nx):
    steps, wants = zip(*[_field(form, with_map, ny, nx, seed) for seed in range(2)])
    want = np.stack(wants)
    stage, rec = _stage(steps)
    assert np.isnan(want).any() == with_map and len(np.unique(want[~np.isnan(want)])) > 100 and min(len(s.lens) for s in steps) > 256
    order = FORMS[form][1]
    got, errors = _run(torch_cuda, stage, rec, order, (ny, nx), (0, 0, ny, nx), (2, ny, nx), (0, 0, 0))
    assert errors == 0
    _same_bits(got, want)
    # ... and a box at an offset in a larger cube
    box = (0, 3, 1, nx - 8) if ny == 1 else (2, 3, ny - 4, nx - 6)
    at = (1, 4, 5)
    got, errors = _run(torch_cuda, stage, rec, order, (ny, nx), box, (4, ny + 7, nx + 11), at)
    assert errors == 0
    _check_box(got, want, box, at)


def test_more_tiles_than_one_round_of_tile_sums(torch_cuda):
    """One step of 257 tiles and 3 values under order 2: the tile sums are scanned 256 a round, so both running sums cross that carry.
    (Some 88,000 groups: the group scan carries a few hundred times, and the binary search is 17 steps deep.)"""
    n = 257 * TILE + 3
    st, want = _field("order2", False, 1, n)
    assert len(st.lens) > 50000 and (n - 1) // TILE + 1 == 258
    stage, rec = _stage([st])
    got, errors = _run(torch_cuda, stage, rec, 2, (1, n), (0, 0, 1, n), (1, 1, n), (0, 0, 0))
    assert errors == 0
    _same_bits(got, want[None])


def test_group_counts_257_1_and_0(torch_cuda):
    """NG = 257 and 513 (the group scan's carry after one and two full rounds), NG = 1 and NG = 0 in one batch, order 2; then 5.2."""
    ny, nx = 9, 57                                                       # 513 points
    rng = np.random.default_rng(3)
    for tmpl, order in ((3, 2), (2, 0)):
        lo = 0 if tmpl == 2 else -500
        steps = [K.CStep(K.smooth(rng, 513, lo), [2] * 256 + [1], tmpl, order, extra=2, R=1.0), K.CStep(K.smooth(rng, 513, lo), [1] * 513, tmpl, order, extra=2),
                 K.CStep(K.smooth(rng, 513, lo), [513], tmpl, order, extra=2, E=-1), K.CStep([0] * 513, [], tmpl, order, extra=2, R=-7.5),
                 K.CStep([0] * 513, [], tmpl, order, extra=0, R=2.0)]
        assert [len(s.lens) for s in steps] == [257, 513, 1, 0, 0]
        want = np.stack([s.expected(ny, nx) for s in steps])
        stage, rec = _stage(steps)
        got, errors = _run(torch_cuda, stage, rec, order, (ny, nx), (0, 0, ny, nx), (5, ny, nx), (0, 0, 0))
        assert errors == 0
        _same_bits(got, want)
        # a scratch sized for fewer groups than a record has refuses that record, and only that one
        got, errors = _run(torch_cuda, stage, rec, order, (ny, nx), (0, 0, ny, nx), (5, ny, nx), (0, 0, 0), max_groups=300)
        assert errors == 1 and (got[1].view(np.uint32) == SENTINEL).all()
        _same_bits(got[[0, 2, 3, 4]], want[[0, 2, 3, 4]])


def _break(rec, stage, steps, what):
    r = rec[1]
    if what == "data beyond the stage":
        r["data_off"] = len(stage) - 8
    elif what == "data offset beyond the stage":
        r["data_off"] = len(stage) + 4
    elif what == "negative data offset":
        r["data_off"] = -4
    elif what == "negative byte count":
        r["data_bytes"] = -1
    elif what == "huge byte count":
        r["data_bytes"] = 1 << 62
    elif what == "lengths do not sum to N":
        r["last_len"] += 1
    elif what == "lengths sum beyond N":
        r["ref_len"] += 1
    elif what == "width 33":
        r["ref_width"] += 33 - max(steps[1].widths)
    elif what == "table width 33":
        r["nbits_ref"] = 33
    elif what == "a table running past the data":
        r["data_bytes"] = steps[1].table_bytes - 1
    elif what == "one byte too few":
        r["data_bytes"] -= 1
    elif what == "more groups than there are bits":
        r["n_groups"] = (1 << 31) - 1
    elif what == "another order":
        r["order"] = 1
    elif what == "extra 5":
        r["extra"] = 5
    elif what == "more values than grid points":
        r["n_values"] += 1
    elif what == "bitmap beyond the stage":
        r["bitmap_off"] = len(stage) - 8
    elif what == "bitmap offset -2":
        r["bitmap_off"] = -2
    elif what == "a bitmap with other 1-bits than N":
        r["n_values"] -= 1
        r["last_len"] -= 1
    else:
        raise KeyError(what)


@pytest.mark.parametrize("with_map,what", [(False, "data beyond the stage"), (False, "data offset beyond the stage"), (False, "negative data offset"),
                                           (False, "negative byte count"), (False, "huge byte count"), (False, "lengths do not sum to N"),
                                           (False, "lengths sum beyond N"), (False, "width 33"), (False, "table width 33"),
                                           (False, "a table running past the data"), (False, "one byte too few"),
                                           (False, "more groups than there are bits"), (False, "another order"), (False, "extra 5"),
                                           (False, "more values than grid points"), (True, "bitmap beyond the stage"), (True, "bitmap offset -2"),
                                           (True, "a bitmap with other 1-bits than N"), (True, "one byte too few"), (True, "width 33")])
def test_a_refused_record_writes_nothing_and_is_counted(torch_cuda, with_map, what):
    """Malformed records: each is counted once, its step stays untouched, its neighbours are served — and every lane stays inside the
    stage and the scratch by the kernels' own checks."""
    ny, nx = 9, 57
    steps, wants = zip(*[_field("order2", with_map, ny, nx, seed, mean=3) for seed in range(3)])
    want = np.stack(wants)
    stage, rec = _stage(steps)
    rec = rec.copy()
    if what == "one byte too few":                                  # (the last value then ends beyond the bytes)
        assert steps[1].table_bytes * 8 + steps[1].value_bits > (len(steps[1].body) - 1) * 8
    max_groups = int(rec["n_groups"].max())
    _break(rec, stage, steps, what)
    got, errors = _run(torch_cuda, stage, rec, 2, (ny, nx), (0, 0, ny, nx), (3, ny, nx), (0, 0, 0), max_groups=max_groups)
    assert errors == 1
    assert (got[1].view(np.uint32) == SENTINEL).all()
    _same_bits(got[0], want[0])
    _same_bits(got[2], want[2])


def test_the_entry_refuses_what_it_cannot_place(torch_cuda):
    torch = torch_cuda
    ny, nx = 9, 57
    steps, _ = zip(*[_field("order1", False, ny, nx, seed) for seed in range(2)])
    stage, rec = _stage(steps)
    for box, shape, at in [((0, 0, ny + 1, nx), (2, ny + 1, nx), (0, 0, 0)), ((0, 1, ny, nx), (2, ny, nx), (0, 0, 0)), ((-1, 0, 2, 2), (2, ny, nx), (0, 0, 0)),
                           ((0, 0, ny, nx), (2, ny, nx - 1), (0, 0, 0)), ((0, 0, ny, nx), (1, ny, nx), (0, 0, 0)), ((0, 0, 2, 2), (2, ny, nx), (1, 0, 0))]:
        with pytest.raises(ValueError):
            _run(torch, stage, rec, 1, (ny, nx), box, shape, at)
    for order in (-1, 3):
        with pytest.raises(ValueError, match="order"):
            _run(torch, stage, rec, order, (ny, nx), (0, 0, ny, nx), (2, ny, nx), (0, 0, 0))
    dev = lambda a: torch.from_numpy(a).cuda()
    mg = int(rec["n_groups"].max())
    scratch = torch.empty(hip.grib_complex_scratch_bytes(2, ny * nx, mg), dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    recs = dev(rec.view(np.uint8).reshape(-1))
    cube = torch.full((2, ny, nx), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    with pytest.raises(ValueError):
        hip.grib_unpack_complex(dev(stage), recs, 2, 1, mg, (ny, nx), (0, 0, ny, nx), cube.double(), (0, 0, 0), scratch, errors)
    with pytest.raises(ValueError, match="4-byte words"):
        hip.grib_unpack_complex(dev(stage)[:-2], recs, 2, 1, mg, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch, errors)
    with pytest.raises(ValueError, match="scratch too small"):
        hip.grib_unpack_complex(dev(stage), recs, 2, 1, mg, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch[:-16], errors)
    with pytest.raises(ValueError, match="scratch too small"):
        hip.grib_unpack_complex(dev(stage), recs, 2, 1, mg + 1, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch, errors)
    with pytest.raises(ValueError):
        hip.grib_unpack_complex(dev(stage), recs[:-8], 2, 1, mg, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch, errors)
    hip.grib_unpack_complex(dev(stage), recs, 2, 1, mg, (ny, nx), (0, 0, 0, nx), cube, (0, 0, 0), scratch, errors)          # an empty box: nothing to do
    hip.grib_unpack_complex(dev(stage), recs, 0, 1, mg, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch, errors)
    torch.cuda.synchronize()
    assert int(errors.item()) == 0 and bool((cube.view(torch.int32) == SENTINEL).all())


# ---------------------------------------------------------------------------------------
# the route
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_streams_into_hbm(torch_cuda, case, files, host, no_host_route):
    ds = af.dataset_from_path(files[case.name], case.var, device="cuda")
    cube = ds.cube()
    assert cube.is_cuda and cube.dtype == torch_cuda.float32 and not ds.is_packed
    got = cube.cpu().numpy()
    _same_bits(got, host[case.name])
    _same_bits(got, case.expected)
    assert ds.time.equals(pd.DatetimeIndex(case.times))
    np.testing.assert_array_equal(ds.latitude, case.latitude)
    np.testing.assert_array_equal(ds.longitude, case.longitude)


def test_three_kinds_in_one_batch_around_a_clipped_box(torch_cuda, tmp_path, no_host_route, monkeypatch):
    """Steps of 5.0, 5.2 and 5.3 (orders 2 and 1) in one slab of `_GribSource.to_device`, rows 1..3 of the grid: each run of one kind goes
    to its entry with its own records and time offset.  Every call is repeated here into a larger cube full of a sentinel, at an offset:
    the cells around the box keep it."""
    torch = torch_cuda
    rng = np.random.default_rng(21)
    steps = [C.field(rng, 12, 0), C.field(rng, 16, 1), K.CStep(K.smooth(rng, K.NP, 0), K.cut(rng, K.NP), 2, valid=K.hours(2)),
             K.CStep(K.smooth(rng, K.NP), K.cut(rng, K.NP), 3, 2, extra=2, E=-1, valid=K.hours(3)),
             K.CStep(K.smooth(rng, K.NP, -100, 100), K.cut(rng, K.NP), 3, 2, extra=1, minsd=-40, valid=K.hours(4)), C.field(rng, 7, 5),
             K.CStep(K.smooth(rng, K.NP), K.cut(rng, K.NP), 3, 1, extra=2, R=3.5, valid=K.hours(6))]
    case = C.Case("kinds", "t2m", [K.message(s) if isinstance(s, K.CStep) else C.message2(s, C.GRID) for s in steps], steps, edition=2)
    path = case.write(tmp_path)
    big = torch.full((len(steps) + 2, 9, 14), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    calls = []
    real = {"simple": hip.grib_unpack, "complex": hip.grib_unpack_complex}

    def simple(stage, recs, n, grid, box, dst, at, rank, errors):
        calls.append(("simple", at[0], n))
        real["simple"](stage, recs, n, grid, box, big, (at[0] + 1, 2, 3), rank, errors)
        real["simple"](stage, recs, n, grid, box, dst, at, rank, errors)

    def cplx(stage, recs, n, order, mg, grid, box, dst, at, scratch, errors):
        calls.append(("complex", order, at[0], n))
        real["complex"](stage, recs, n, order, mg, grid, box, big, (at[0] + 1, 2, 3), scratch, errors)
        real["complex"](stage, recs, n, order, mg, grid, box, dst, at, scratch, errors)

    monkeypatch.setattr(hip, "grib_unpack", simple)
    monkeypatch.setattr(hip, "grib_unpack_complex", cplx)
    ds = af.dataset_from_path(path, "t2m", device="cuda", lat_window=(1, 4))
    assert calls == [("simple", 0, 2), ("complex", 0, 2, 1), ("complex", 2, 3, 2), ("simple", 5, 1), ("complex", 1, 6, 1)]
    _same_bits(ds.cube().cpu().numpy(), case.expected[:, 1:4])
    _check_box(big.cpu().numpy(), case.expected, (1, 0, 3, K.NI), (1, 2, 3))


GRID360 = (C.NI, C.NJ, 50.0, 230.0, 49.0, 232.0, 0x00)


@pytest.fixture(scope="module")
def windows_files(tmp_path_factory):
    """7 hourly steps from 2024-07-15 00:00 on a 5 x 9 grid at 230..232 degrees east: order 2 plain, and order 1 with a bitmap."""
    d = tmp_path_factory.mktemp("gribcwin")
    rng = np.random.default_rng(78)
    out = {}
    for name, order, with_map in (("plain", 2, False), ("bitmap", 1, True)):
        steps = []
        for k in range(C.STEPS):
            bm = C.some_bitmap(rng) if with_map else None
            n = K.NP if bm is None else sum(bm)
            steps.append(K.CStep(K.smooth(rng, n), K.cut(rng, n), 3, order, extra=2, E=-2, R=-118.625, bitmap=bm, valid=K.hours(k)))
        case = C.Case(name, "t2m", [K.message(s, GRID360) for s in steps], steps, grid=GRID360, edition=2)
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
@pytest.mark.parametrize("name", ["plain", "bitmap"])
def test_windows_read_the_same_box(torch_cuda, name, time, space, windows_files, no_host_route):
    case, path = windows_files[name]
    tkw, ts = TIME_WINDOWS[time]
    skw, ys, xs = SPACE_WINDOWS[space]
    ds = af.dataset_from_path(path, "t2m", device="cuda", keep_packed=True, **tkw, **skw())
    cube = ds.cube()
    assert cube.is_cuda and not ds.is_packed
    _same_bits(cube.cpu().numpy(), case.expected[ts, ys, xs])
    np.testing.assert_array_equal(ds.latitude, case.latitude[ys])
    np.testing.assert_array_equal(ds.longitude, case.longitude[xs])
    assert len(ds.time) == ts.stop - ts.start


def test_slabs_of_one_or_two_steps_and_the_scratch_cap(torch_cuda, files, no_host_route, monkeypatch):
    """A tiny slab: the 7 steps of the mixed file go through several slabs, each cut into its runs."""
    case = BY["c3_mixed_with_simple"]
    monkeypatch.setenv("AGGFLY_HIP_SLAB_MB", repr(2.5 * 96 / (1 << 20)))
    calls = []
    real_s, real_c = hip.grib_unpack, hip.grib_unpack_complex
    monkeypatch.setattr(hip, "grib_unpack", lambda stage, steps, n, *a: calls.append(n) or real_s(stage, steps, n, *a))
    monkeypatch.setattr(hip, "grib_unpack_complex", lambda stage, steps, n, *a: calls.append(n) or real_c(stage, steps, n, *a))
    ds = af.dataset_from_path(files[case.name], case.var, device="cuda")
    assert len(calls) >= 5 and sum(calls) == 7, calls
    _same_bits(ds.cube().cpu().numpy(), case.expected)


def test_several_files_and_preprocess(torch_cuda, tmp_path, no_host_route):
    rng = np.random.default_rng(12)
    steps = [K.CStep(K.smooth(rng, K.NP), K.cut(rng, K.NP), 3, 1 + k % 2, extra=2, E=-3, R=280.0, valid=K.hours(k)) for k in range(8)]
    paths = []
    for j, part in enumerate((steps[:3], steps[3:])):
        paths.append(str(tmp_path / f"part{j}.grib2"))
        with open(paths[-1], "wb") as f:
            f.write(b"".join(K.message(s) for s in part))
    want = np.stack([s.expected(K.NJ, K.NI) for s in steps])
    pre = lambda x: x - 273.15
    for p in (paths, str(tmp_path / "part*.grib2")):
        ds = af.dataset_from_path(p, "t2m", device="cuda", lon_is_360=False, preprocess=pre)
        assert ds.cube().is_cuda and ds.time.equals(pd.DatetimeIndex([s.valid for s in steps]))
        _same_bits(ds.cube().cpu().numpy(), want - np.float32(273.15))
    assert D._step_bytes(paths[0], "t2m") == K.NJ * K.NI * 4


def test_unsound_tables_in_a_file_are_an_error(torch_cuda, tmp_path):
    """Group lengths that do not sum to N pass the index (the headers are sound): the kernels refuse the step and the route says so."""
    rng = np.random.default_rng(13)
    st = K.CStep(K.smooth(rng, K.NP), [9] * 5, 3, 2, extra=2, last_len=8)
    path = str(tmp_path / "unsound.grib2")
    with open(path, "wb") as f:
        f.write(K.message(st))
    with pytest.raises(ValueError, match="refused by the unpack kernels"):
        af.dataset_from_path(path, "t2m", device="cuda", lon_is_360=False)


# ---------------------------------------------------------------------------------------
# the store routes
# ---------------------------------------------------------------------------------------
def test_store_sharded_streams_a_complex_packed_file_in_windows(torch_cuda, tmp_path, no_host_route, monkeypatch):
    """`aggregate_store_sharded` on one GRIB2 file in 5.3 order 2 with a bitmap over the ocean (January 30th to February 2nd, monthly
    output) under a budget of two days per window: each window streams its own messages, and the frame equals `aggregate_dataset` on
    the whole dataset exactly (the comparison of tests/test_gpu_grib.py::test_store_sharded_streams_a_grib_file_in_windows)."""
    import types
    from aggfly_amd import engine as eng, synth
    from aggfly_amd.cli import pipeline
    T_, ny, nx = 24 * 4, 10, 12
    cube = synth.temperature_cube(T_, ny, nx, dtype=np.float32, seed=63, ocean_frac=0.1, scattered_nan=30) + np.float32(273.15)
    g = (nx, ny, 50.0, 230.0, 50.0 - 0.25 * (ny - 1), 230.0 + 0.25 * (nx - 1), 0x00)
    rng = np.random.default_rng(64)
    msgs = []
    for k in range(T_):
        have = ~np.isnan(cube[k].ravel())
        X = np.round((cube[k].ravel()[have].astype(np.float64) - 250.0) * 256.0).astype(np.int64).tolist()
        st = K.CStep(X, K.cut(rng, len(X), 8), 3, 2, extra=2, E=-8, D=0, R=250.0, bitmap=[int(b) for b in have],
                     valid=dt.datetime(2000, 1, 30) + dt.timedelta(hours=k))
        msgs.append(K.message(st, g))
    path = str(tmp_path / "ncep.grib2")
    with open(path, "wb") as f:
        f.write(b"".join(msgs))
    assert pipeline._streams_grib(types.SimpleNamespace(var="t2m", timecoord="time"), path)
    tab = synth.weights_table(ny, nx, 6, seed=62, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}))
    spec = dict(dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": "month"})],
                t=[("aggregate", {"calc": "mean", "groupby": "date"}), ("aggregate", {"calc": "sum", "groupby": "month"})])
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
