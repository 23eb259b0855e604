"""GRIB2 CCSDS packing (template 5.42) on the device route: the entry `hip.grib_unpack_ccsds` against the expectation of the case writer
of tests/grib_ccsds_cases.py and the streams of tests/golden/grib_ccsds_streams.json — bit for bit, NaN positions included, a sentinel
everywhere outside the box —, across the seams of its passes (every RSI boundary, zero runs across the 64-block segment, an FS run longer
than the wave's window of 2,048 bits), its refusals, and `dataset_from_path(device="cuda")` on the catalogue with windows, a file that
mixes simple, complex and CCSDS packing, and the sharded store route.  Every comparison is exact: no tolerance is involved."""
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
import grib_ccsds_cases as A  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import distributed as D, grib, hip, io as afio  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = A.build_cases()
BY = {c.name: c for c in CASES}
GOLDEN = A.golden()
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("griba")
    return {c.name: c.write(d) for c in CASES}


@pytest.fixture
def no_host_route(monkeypatch):
    """The host decode is not an answer here."""
    def refuse(*a, **k):
        raise AssertionError("the host route was taken")
    monkeypatch.setattr(afio, "_open_grib", refuse)
    monkeypatch.setattr(grib, "decode_message", refuse)
    monkeypatch.setattr(grib, "unpack_ccsds", refuse)
    monkeypatch.setattr(grib, "unpack_complex", refuse)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (a.shape, a.dtype, b.shape, b.dtype)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------
# the entry
# ---------------------------------------------------------------------------------------
def _pad4(b: bytes) -> bytes:
    return b + b"\x00" * (-len(b) % 4)


def _stage(steps):
    """The stage of ``steps`` as the route lays it out — per step the bitmap, then the body of section 7, each padded to 4 bytes — and
    the records.  The stage ends with the last step's last word: there is no slack behind it."""
    stage, rec = b"", np.zeros(len(steps), dtype=hip.GRIB_ASTEP)
    for k, s in enumerate(steps):
        r = rec[k]
        r["bitmap_off"] = -1
        if s.bitmap is not None:
            r["bitmap_off"] = len(stage)
            stage += _pad4(C.pack_bits(s.bitmap, 1)[0])
        r["data_off"], r["data_bytes"], r["n_values"] = len(stage), len(s.body), len(s.X)
        r["nbits"], r["flags"], r["block_size"], r["rsi"] = s.nbits, s.flags, s.J, s.rsi
        r["R"], r["s"], r["d"] = s.R, 2.0 ** s.E, 10.0 ** -s.D
        stage += _pad4(s.body)
    return np.frombuffer(stage if stage else b"\x00" * 4, dtype=np.uint8).copy(), rec


def _max_rsis(rec):
    per = np.maximum(rec["rsi"].astype(np.int64) * rec["block_size"], 1)
    return int(np.max(-(-rec["n_values"] // per)))


def _run(torch, stage, rec, grid, box, cube_shape, at, max_rsis=None):
    """-> (cube as numpy, errors) after one `hip.grib_unpack_ccsds` into a cube full of the sentinel."""
    n = len(rec)
    max_rsis = _max_rsis(rec) if max_rsis is None else max_rsis
    cube = torch.full(cube_shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    scratch = torch.empty(hip.grib_ccsds_scratch_bytes(n, grid[0] * grid[1], max_rsis), dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.grib_unpack_ccsds(torch.from_numpy(stage).cuda(), torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda(), n, max_rsis, grid, box, cube, at,
                          scratch, errors)
    torch.cuda.synchronize()
    return cube.cpu().numpy(), int(errors.item())


def _check_box(got, want, box, at):
    y0, x0, ny, nx = box
    t0, cy, cx = at
    inside = np.zeros(got.shape, bool)
    inside[t0:t0 + want.shape[0], cy:cy + ny, cx:cx + nx] = True
    _same_bits(got[inside].reshape(want.shape[0], ny, nx), want[:, y0:y0 + ny, x0:x0 + nx])
    assert (got.view(np.uint32)[~inside] == SENTINEL).all()


def _both_ways(torch, steps, ny, nx):
    """The whole grid, then a box at an offset in a larger cube full of the sentinel."""
    want = np.stack([s.expected(ny, nx) for s in steps])
    stage, rec = _stage(steps)
    got, errors = _run(torch, stage, rec, (ny, nx), (0, 0, ny, nx), (len(steps), ny, nx), (0, 0, 0))
    assert errors == 0
    _same_bits(got, want)
    box, at = (2, 3, ny - 4, nx - 6), (1, 4, 5)
    got, errors = _run(torch, stage, rec, (ny, nx), box, (len(steps) + 2, ny + 7, nx + 11), at)
    assert errors == 0
    _check_box(got, want, box, at)
    return want


@functools.lru_cache(maxsize=None)
def _grid_steps(name, with_map):
    """Two or three steps of differing parameters on the grid ``name``, built once."""
    rng = np.random.default_rng({"19x23": 1, "37x53": 2, "70x61": 3}[name] + 10 * with_map)
    ny, nx = (int(v) for v in name.split("x"))
    bm = lambda: C.some_bitmap(rng, ny * nx) if with_map else None
    count = lambda b: ny * nx if b is None else sum(b)
    steps = []
    if name == "19x23":                                                  # J = 8, rsi = 4: 14 RSIs, the last one short
        for k, (n, pp) in enumerate(((12, True), (16, True), (9, False))):
            b = bm()
            steps.append(A.AStep(A.smooth(rng, count(b), n, step=(9, 300, 2)[k]), n, J=8, rsi=4, flags=(A.PREPROCESS if pp else 0) | 4, E=-2 - k, D=k % 2,
                                 R=(-118.625, 273.125, 0.5)[k], bitmap=b))
        assert -(-19 * 23 // 32) == 14
    elif name == "37x53":                                                # J = 8, rsi = 128: constant and near-constant, runs across the segment seam
        for k, X in enumerate(([1234], None, None)):
            b = bm()
            X = X * count(b) if X else A.near_constant(rng, count(b), 16, p=(0, 0.004, 0.03)[k])
            steps.append(A.AStep(X, 16, J=8, rsi=128, E=-3, R=(2.0, 273.125, -0.5)[k], bitmap=b))
    else:                                                                # the defaults: J = 32, rsi = 128: one full RSI and a short one
        for k, n in enumerate((16, 24)):
            b = bm()
            steps.append(A.AStep(A.smooth(rng, count(b), n, step=40), n, E=-4 - k, R=250.0, bitmap=b))
    return tuple(steps), ny, nx


@pytest.mark.parametrize("with_map", [False, True], ids=["plain", "bitmap"])
@pytest.mark.parametrize("name", ["19x23", "37x53", "70x61"])
def test_unpack_against_the_case_writer(torch_cuda, name, with_map):
    steps, ny, nx = _grid_steps(name, with_map)
    want = _both_ways(torch_cuda, list(steps), ny, nx)
    assert np.isnan(want).any() == with_map
    if name == "37x53" and not with_map:                                 # the writer did write runs that end at a segment seam
        assert len(steps[0].body) < 40 and steps[0].rsi * steps[0].J < ny * nx


@pytest.mark.skipif(A.load_libaec() is None, reason="libaec cannot be loaded on this machine")
@pytest.mark.parametrize("name", ["19x23", "37x53", "70x61"])
def test_unpack_streams_libaec_wrote(torch_cuda, name):
    steps, ny, nx = _grid_steps(name, False)
    mine = [A.AStep(s.X, s.nbits, J=s.J, rsi=s.rsi, flags=s.flags, E=s.E, D=s.D, R=s.R,
                    stream=A.libaec_encode(s.X, s.nbits, s.J, s.rsi, s.flags & A.PREPROCESS)) for s in steps]
    _both_ways(torch_cuda, mine, ny, nx)


def test_every_golden_stream_in_one_call_per_length(torch_cuda):
    """The fixture's streams — every block option, the forced ones, the FS run of more than 2,048 bits, X >= 2^31 — as steps of one call
    each batch: streams of one length share a grid of 1 x length."""
    by_len = {}
    for row in GOLDEN:
        by_len.setdefault(len(row["samples"]), []).append(row)
    assert any(r["name"] == "forced_long_fs" for r in GOLDEN)
    for n, rows in sorted(by_len.items()):
        steps = [A.AStep(r["samples"], r["nbits"], J=r["block_size"], rsi=r["rsi"], flags=A.PREPROCESS if r["preprocess"] else 0,
                         E=0, R=0.0, stream=bytes.fromhex(r["hex"])) for r in rows]
        stage, rec = _stage(steps)
        got, errors = _run(torch_cuda, stage, rec, (1, n), (0, 0, 1, n), (len(steps), 1, n), (0, 0, 0))
        assert errors == 0, [r["name"] for r in rows]
        want = np.stack([s.expected(1, n) for s in steps])
        _same_bits(got, want)
        assert all(got[k, 0].astype(np.float64).tolist() == [float(np.float32(v)) for v in r["samples"]] for k, r in enumerate(rows))


def test_nbits_0_and_differing_parameters_in_one_call(torch_cuda):
    ny, nx = 9, 57
    rng = np.random.default_rng(4)
    bm = C.some_bitmap(rng, ny * nx)
    steps = [A.AStep([0] * (ny * nx), 0, R=280.5), A.AStep(A.smooth(rng, ny * nx, 8), 8, J=64, rsi=1, E=1, R=-3.0),
             A.AStep([0] * sum(bm), 0, J=8, rsi=1, R=-1.25, D=1, bitmap=bm), A.AStep(A.smooth(rng, ny * nx, 32, step=1 << 20), 32, J=16, rsi=4096, E=-20),
             A.AStep(A.smooth(rng, sum(bm), 1, step=1), 1, J=8, rsi=2, flags=0, bitmap=bm)]
    assert steps[0].body == b"" and max(steps[3].X) >= 1 << 31
    _both_ways(torch_cuda, steps, ny, nx)


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
    elif what == "one byte too few":
        r["data_bytes"] -= 1
    elif what == "half the stream":
        r["data_bytes"] //= 2
    elif what == "no bytes":
        r["data_bytes"] = 0
    elif what == "nbits 33":
        r["nbits"] = 33
    elif what == "negative nbits":
        r["nbits"] = -1
    elif what == "flag 1":
        r["flags"] |= 1
    elif what == "flag 16":
        r["flags"] |= 16
    elif what == "flag 32":
        r["flags"] |= 32
    elif what == "block size 12":
        r["block_size"] = 12
    elif what == "block size 0":
        r["block_size"] = 0
    elif what == "rsi 0":
        r["rsi"] = 0
    elif what == "rsi 4097":
        r["rsi"] = 4097
    elif what == "more intervals than the scratch holds":
        r["rsi"] = 1
    elif what == "more values than grid points":
        r["n_values"] += 1
    elif what == "negative values":
        r["n_values"] = -1
    elif what == "bitmap beyond the stage":
        r["bitmap_off"] = len(stage) - 8
    elif what == "bitmap offset -2":
        r["bitmap_off"] = -2
    elif what == "a bitmap with other 1-bits than N":
        r["n_values"] -= 1
    else:
        raise KeyError(what)


@pytest.mark.parametrize("with_map,what", [(False, "data beyond the stage"), (False, "data offset beyond the stage"), (False, "negative data offset"),
                                           (False, "negative byte count"), (False, "huge byte count"), (False, "one byte too few"),
                                           (False, "half the stream"), (False, "no bytes"), (False, "nbits 33"), (False, "negative nbits"),
                                           (False, "flag 1"), (False, "flag 16"), (False, "flag 32"), (False, "block size 12"), (False, "block size 0"),
                                           (False, "rsi 0"), (False, "rsi 4097"), (False, "more intervals than the scratch holds"),
                                           (False, "more values than grid points"), (False, "negative values"), (True, "bitmap beyond the stage"),
                                           (True, "bitmap offset -2"), (True, "a bitmap with other 1-bits than N"), (True, "one byte too few")])
def test_a_refused_record_writes_nothing_and_is_counted(torch_cuda, with_map, what):
    """Malformed records and truncated streams: each is counted once, its step stays untouched, its neighbours are served — and every lane
    stays inside the stage and the scratch by the passes' own checks (aec_passes.h: the safety contract)."""
    ny, nx = 9, 57
    rng = np.random.default_rng(8 + with_map)
    steps = []
    for k in range(3):
        bm = C.some_bitmap(rng, ny * nx) if with_map else None
        # noisy in its last samples: the stream's last byte holds bits of a sample
        X = A.smooth(rng, (ny * nx if bm is None else sum(bm)) - 20, 12) + [int(v) for v in rng.integers(0, 4096, size=20)]
        steps.append(A.AStep(X, 12, J=8, rsi=4, E=-2, R=1.0 + k, bitmap=bm))
    want = np.stack([s.expected(ny, nx) for s in steps])
    stage, rec = _stage(steps)
    rec = rec.copy()
    max_rsis = _max_rsis(rec)
    _break(rec, stage, steps, what)
    got, errors = _run(torch_cuda, stage, rec, (ny, nx), (0, 0, ny, nx), (3, ny, nx), (0, 0, 0), max_rsis=max_rsis)
    assert errors == 1
    assert (got[1].view(np.uint32) == SENTINEL).all()
    _same_bits(got[0], want[0])
    _same_bits(got[2], want[2])


def _bits_to_bytes(s):
    s += "0" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big")


def test_damaged_streams_are_counted_and_leave_the_cube_untouched(torch_cuda):
    """Streams whose record is sound and whose bits are not: a zero run beyond the RSI's last block, a second-extension code above 90, a
    delta above xmax, an FS run that never ends, and bit flips of a good stream (whatever they decode to, nothing is written outside
    the step and the error count is 0 or 1 per step)."""
    n = 16
    ref = A.bits(5, 8)
    bad = [A.bits(0, 3) + "0" + ref + A.fs(2),                                          # 3 zero blocks where the RSI (rsi = 2) has 2
           A.bits(0, 3) + "1" + ref + A.fs(91) + A.fs(0) * 3 + A.bits(1, 3) + A.fs(0) * 8,
           A.bits(5, 3) + ref + A.fs(16) + A.fs(0) * 6 + A.bits(0, 4) * 7 + A.bits(1, 3) + A.fs(0) * 8,   # k = 4, q = 16: delta 256 in 8 bits
           A.bits(1, 3) + ref + "0" * 4000]
    good = A.AStep([5] * 8 + [6, 5, 5, 7, 5, 5, 5, 5], 8, J=8, rsi=2, R=0.5)
    steps = [good] + [A.AStep([0] * n, 8, J=8, rsi=2, stream=_bits_to_bytes(s)) for s in bad] + [good]
    stage, rec = _stage(steps)
    got, errors = _run(torch_cuda, stage, rec, (1, n), (0, 0, 1, n), (len(steps), 1, n), (0, 0, 0))
    assert errors == len(bad)
    assert (got[1:-1].view(np.uint32) == SENTINEL).all()
    _same_bits(got[0], good.expected(1, n))
    _same_bits(got[-1], good.expected(1, n))
    # single-bit flips of one stream, every flip a step of one call
    rng = np.random.default_rng(9)
    X = A.smooth(rng, 200, 12)
    base = A.AStep(X, 12, J=8, rsi=4)
    flips = []
    for bit in rng.choice(len(base.body) * 8, size=48, replace=False):
        b = bytearray(base.body)
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        flips.append(A.AStep(X, 12, J=8, rsi=4, stream=bytes(b)))
    stage, rec = _stage([base] + flips + [base])
    got, errors = _run(torch_cuda, stage, rec, (1, 200), (0, 0, 1, 200), (len(flips) + 2, 1, 200), (0, 0, 0))
    assert 0 <= errors <= len(flips)
    untouched = (got[1:-1].view(np.uint32) == SENTINEL).all(axis=(1, 2))
    assert int(untouched.sum()) == errors                                # a refused step is written by nobody, an accepted one whole
    _same_bits(got[0], base.expected(1, 200))
    _same_bits(got[-1], base.expected(1, 200))
    # the host decoder, which runs the same passes, refuses the same flips
    from aggfly_amd import codec
    for k, st in enumerate(flips):
        try:
            host = codec.aec_decode(st.body, 200, 12, A.PREPROCESS, 8, 4)
        except codec.CodecError:
            host = None
        assert (host is None) == bool(untouched[k]), k
        if host is not None:
            _same_bits(got[1 + k, 0], host.astype(np.float64).astype(np.float32))


def test_the_entry_refuses_what_it_cannot_place(torch_cuda):
    torch = torch_cuda
    ny, nx = 9, 57
    rng = np.random.default_rng(10)
    steps = [A.AStep(A.smooth(rng, ny * nx, 12), 12, J=8, rsi=4) for _ in range(2)]
    stage, rec = _stage(steps)
    for box, shape, at in [((0, 0, ny + 1, nx), (2, ny + 1, nx), (0, 0, 0)), ((0, 1, ny, nx), (2, ny, nx), (0, 0, 0)), ((-1, 0, 2, 2), (2, ny, nx), (0, 0, 0)),
                           ((0, 0, ny, nx), (2, ny, nx - 1), (0, 0, 0)), ((0, 0, ny, nx), (1, ny, nx), (0, 0, 0)), ((0, 0, 2, 2), (2, ny, nx), (1, 0, 0))]:
        with pytest.raises(ValueError):
            _run(torch, stage, rec, (ny, nx), box, shape, at)
    dev = lambda a: torch.from_numpy(a).cuda()
    mr = _max_rsis(rec)
    scratch = torch.empty(hip.grib_ccsds_scratch_bytes(2, ny * nx, mr), dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    recs = dev(rec.view(np.uint8).reshape(-1))
    cube = torch.full((2, ny, nx), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    with pytest.raises(ValueError):
        hip.grib_unpack_ccsds(dev(stage), recs, 2, mr, (ny, nx), (0, 0, ny, nx), cube.double(), (0, 0, 0), scratch, errors)
    with pytest.raises(ValueError, match="4-byte words"):
        hip.grib_unpack_ccsds(dev(stage)[:-2], recs, 2, mr, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch, errors)
    with pytest.raises(ValueError, match="scratch too small"):
        hip.grib_unpack_ccsds(dev(stage), recs, 2, mr, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch[:-16], errors)
    with pytest.raises(ValueError, match="scratch too small"):
        hip.grib_unpack_ccsds(dev(stage), recs, 2, mr + 2, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch, errors)
    with pytest.raises(ValueError):
        hip.grib_unpack_ccsds(dev(stage), recs[:-8], 2, mr, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch, errors)
    hip.grib_unpack_ccsds(dev(stage), recs, 2, mr, (ny, nx), (0, 0, 0, nx), cube, (0, 0, 0), scratch, errors)          # an empty box: nothing to do
    hip.grib_unpack_ccsds(dev(stage), recs, 0, mr, (ny, nx), (0, 0, ny, nx), cube, (0, 0, 0), scratch, errors)
    torch.cuda.synchronize()
    assert int(errors.item()) == 0 and bool((cube.view(torch.int32) == SENTINEL).all())


# ---------------------------------------------------------------------------------------
# the route
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_case_streams_into_hbm(torch_cuda, case, files, no_host_route):
    ds = af.dataset_from_path(files[case.name], case.var, device="cuda")
    cube = ds.cube()
    assert cube.is_cuda and cube.dtype == torch_cuda.float32 and not ds.is_packed
    _same_bits(cube.cpu().numpy(), case.expected)
    assert ds.time.equals(pd.DatetimeIndex(case.times))
    np.testing.assert_array_equal(ds.latitude, case.latitude)
    np.testing.assert_array_equal(ds.longitude, case.longitude)


def test_three_packings_in_one_batch_around_a_clipped_box(torch_cuda, tmp_path, no_host_route, monkeypatch):
    """Steps of 5.0, 5.3, 5.2 and 5.42 in one slab of `_GribSource.to_device`, rows 1..3 of the grid: each run of one kind goes to its
    entry with its own records and time offset."""
    rng = np.random.default_rng(22)
    steps = [C.field(rng, 12, 0), A.AStep(A.smooth(rng, K.NP, 16), 16, J=8, rsi=2, E=-2, R=3.5, valid=A.hours(1)),
             A.AStep(A.smooth(rng, K.NP, 9), 9, J=16, rsi=1, flags=0, valid=A.hours(2)),
             K.CStep(K.smooth(rng, K.NP), K.cut(rng, K.NP), 3, 2, extra=2, E=-1, valid=K.hours(3)), A.AStep([0] * K.NP, 0, R=7.0, valid=A.hours(4)),
             C.field(rng, 7, 5), K.CStep(K.smooth(rng, K.NP, 0), K.cut(rng, K.NP), 2, valid=K.hours(6)),
             A.AStep(A.smooth(rng, K.NP, 24), 24, valid=A.hours(7))]
    msg = lambda s: A.message(s) if isinstance(s, A.AStep) else K.message(s) if isinstance(s, K.CStep) else C.message2(s, C.GRID)
    case = C.Case("kinds", "t2m", [msg(s) for s in steps], steps, edition=2)
    path = case.write(tmp_path)
    calls = []
    real = {"simple": hip.grib_unpack, "complex": hip.grib_unpack_complex, "ccsds": hip.grib_unpack_ccsds}
    monkeypatch.setattr(hip, "grib_unpack", lambda stage, recs, n, grid, box, dst, at, *a: calls.append(("simple", at[0], n)) or
                        real["simple"](stage, recs, n, grid, box, dst, at, *a))
    monkeypatch.setattr(hip, "grib_unpack_complex", lambda stage, recs, n, order, mg, grid, box, dst, at, *a: calls.append(("complex", order, at[0], n)) or
                        real["complex"](stage, recs, n, order, mg, grid, box, dst, at, *a))
    monkeypatch.setattr(hip, "grib_unpack_ccsds", lambda stage, recs, n, mr, grid, box, dst, at, *a: calls.append(("ccsds", at[0], n)) or
                        real["ccsds"](stage, recs, n, mr, grid, box, dst, at, *a))
    ds = af.dataset_from_path(path, "t2m", device="cuda", lat_window=(1, 4), keep_packed=True)
    assert calls == [("simple", 0, 1), ("ccsds", 1, 2), ("complex", 2, 3, 1), ("ccsds", 4, 1), ("simple", 5, 1), ("complex", 0, 6, 1), ("ccsds", 7, 1)]
    assert not ds.is_packed
    _same_bits(ds.cube().cpu().numpy(), case.expected[:, 1:4])


GRID360 = (C.NI, C.NJ, 50.0, 230.0, 49.0, 232.0, 0x00)


@pytest.fixture(scope="module")
def windows_files(tmp_path_factory):
    """7 hourly steps from 2024-07-15 00:00 on a 5 x 9 grid at 230..232 degrees east: plain, and with a bitmap."""
    d = tmp_path_factory.mktemp("gribawin")
    rng = np.random.default_rng(79)
    out = {}
    for name, with_map in (("plain", False), ("bitmap", True)):
        steps = []
        for k in range(C.STEPS):
            bm = C.some_bitmap(rng) if with_map else None
            steps.append(A.AStep(A.smooth(rng, A.NP if bm is None else sum(bm), 14), 14, J=8, rsi=3, E=-2, R=-118.625, bitmap=bm, valid=A.hours(k)))
        case = C.Case(name, "t2m", [A.message(s, GRID360) for s in steps], steps, grid=GRID360, edition=2)
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
    """A tiny slab: the 7 steps go through several slabs."""
    case = BY["a_varying_forced_options"]
    monkeypatch.setenv("AGGFLY_HIP_SLAB_MB", repr(2.5 * 96 / (1 << 20)))
    calls = []
    real = hip.grib_unpack_ccsds
    monkeypatch.setattr(hip, "grib_unpack_ccsds", lambda stage, steps, n, *a: calls.append(n) or real(stage, steps, n, *a))
    ds = af.dataset_from_path(files[case.name], case.var, device="cuda")
    assert len(calls) >= 3 and sum(calls) == 7, calls
    _same_bits(ds.cube().cpu().numpy(), case.expected)


def test_a_damaged_stream_in_a_file_is_an_error(torch_cuda, tmp_path):
    """A section 7 cut short passes the index (the headers are sound): the kernels refuse the step and the route says so."""
    rng = np.random.default_rng(13)
    st = A.AStep(A.smooth(rng, A.NP - 6, 12) + [int(v) for v in rng.integers(0, 4096, size=6)], 12, J=8, rsi=2, cut7=2)
    path = str(tmp_path / "cut.grib2")
    with open(path, "wb") as f:
        f.write(A.message(A.AStep(A.smooth(rng, A.NP, 12), 12, J=8, rsi=2, valid=A.hours(1))) + A.message(st))
    with pytest.raises(ValueError, match="refused by the unpack kernels"):
        af.dataset_from_path(path, "t2m", device="cuda", lon_is_360=False)


# ---------------------------------------------------------------------------------------
# the store routes
# ---------------------------------------------------------------------------------------
def test_store_sharded_streams_a_ccsds_packed_file_in_windows(torch_cuda, tmp_path, no_host_route, monkeypatch):
    """`aggregate_store_sharded` on one GRIB2 file in 5.42 with a bitmap over the ocean (January 30th to February 2nd, monthly output)
    under a budget of two days per window: each window streams its own messages, and the frame equals `aggregate_dataset` on the whole
    dataset exactly (the comparison of tests/test_gpu_grib_complex.py::test_store_sharded_streams_a_complex_packed_file_in_windows)."""
    import types
    from aggfly_amd import engine as eng, synth
    from aggfly_amd.cli import pipeline
    T_, ny, nx = 24 * 4, 10, 12
    cube = synth.temperature_cube(T_, ny, nx, dtype=np.float32, seed=63, ocean_frac=0.1, scattered_nan=30) + np.float32(273.15)
    g = (nx, ny, 50.0, 230.0, 50.0 - 0.25 * (ny - 1), 230.0 + 0.25 * (nx - 1), 0x00)
    msgs = []
    for k in range(T_):
        have = ~np.isnan(cube[k].ravel())
        X = np.round((cube[k].ravel()[have].astype(np.float64) - 250.0) * 256.0).astype(np.int64).tolist()
        st = A.AStep(X, 16, J=8, rsi=4, E=-8, D=0, R=250.0, bitmap=[int(b) for b in have], valid=dt.datetime(2000, 1, 30) + dt.timedelta(hours=k))
        msgs.append(A.message(st, g))
    path = str(tmp_path / "ifs.grib2")
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
