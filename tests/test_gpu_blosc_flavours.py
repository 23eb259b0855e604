"""The Blosc-1 flavours of the decode-in-HBM route beyond LZ4 + byte shuffle — Zstandard streams with any shuffle, LZ4 streams
under the bit shuffle — on the GPU: `afcodec_blosc_plan`'s five record lists run through `afhip_lz4_decode_streams`,
`afhip_zstd_decode` (into the shuffle scratch), `afhip_unshuffle_blocks` and `afhip_bitunshuffle_blocks`.  Every chunk the real
c-blosc 1.21 wrote decodes bit-exact in one batch of mixed flavours; the bit-unshuffle kernel alone matches a numpy reference at
every size and alignment where it takes another path; the in-tree encoder's chunks of all three new flavours decode bit-exact;
damaged Zstandard payloads are counted, never followed out of bounds; stores read through `dataset_from_path(device="cuda")`
give the same cube on both routes; and a store that turns blosclz midway finishes on the host route."""
import base64
import json
import os
import sys

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_blosc_fixtures import recipe          # noqa: E402
import make_blosc_flavour_fixtures as ff        # noqa: E402

import aggfly_amd as af                         # noqa: E402
from aggfly_amd import codec, synth             # noqa: E402

pytestmark = pytest.mark.gpu
CASES = json.load(open(os.path.join(HERE, "golden", "blosc_fixtures.json")))["cases"] + ff.load()["cases"]
GUARD = 64
WAVE_ELEMENTS = 512                              # k_bitunshuffle_blocks: a lane takes 8 elements, a wave 512 a step


def bit_unshuffle_reference(src: np.ndarray, ts: int) -> np.ndarray:
    """Blosc's bit shuffle undone for one block, in numpy alone."""
    n = len(src) // ts
    out = src.copy()
    if n % 8 != 0 or n == 0:
        return out
    bits = np.unpackbits(src[:n * ts].reshape(ts * 8, n // 8), axis=1, bitorder="little")
    out[:n * ts] = np.packbits(bits.reshape(ts, 8, n).transpose(2, 0, 1), axis=2, bitorder="little").reshape(n * ts)
    return out


def _pack(chunks, nbytes):
    offs = np.concatenate([[0], np.cumsum([(len(c) + 63) // 64 * 64 for c in chunks])]).astype(np.int64)
    base = np.zeros(max(int(offs[-1]), 64), dtype=np.uint8)
    for o, c in zip(offs, chunks):
        base[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)
    out_off = np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 + GUARD for n in nbytes])]).astype(np.int64)
    return base, offs[:-1], out_off


def _plan(chunks, nbytes, strict=True):
    base, co, out_off = _pack(chunks, nbytes)
    nblk = sum(-(-n // max(codec.blosc_info(c)["blocksize"], 1)) + 1 for c, n in zip(chunks, nbytes))
    lists = [np.zeros(16 * nblk + sum(nbytes) // 65536 + 64, dtype=codec.LZ4_STREAM), np.zeros(nblk + 1, dtype=codec.SHUFFLE_BLOCK),
             np.zeros(nblk + 1, dtype=codec.SHUFFLE_BLOCK), np.zeros(nblk + 1, dtype=codec.ZSTD_FRAME),
             np.zeros(sum(nbytes) // 16384 + 4 * nblk + 64, dtype=codec.ZSTD_BLOCK)]
    p = codec.blosc_plan(base, co, [len(c) for c in chunks], out_off[:-1], nbytes, *lists, strict=strict)
    return base, out_off, lists, p


def _run(torch, base, out_off, lists, p, nbytes):
    """The four launches of the route on one batch -> (decoded arrays | None where the planner refused, errors, host copy of out)."""
    from aggfly_amd import hip
    counts = (p.n_streams, p.n_shuf, p.n_bits, p.n_frames, p.n_blocks)
    comp = torch.from_numpy(base).cuda()
    st, sh, bt, fr, zb = (torch.from_numpy(a[:max(n, 1)].view(np.uint8).copy()).cuda() for a, n in zip(lists, counts))
    out = torch.full((max(int(out_off[-1]), 64),), 0xAB, dtype=torch.uint8, device="cuda")
    tmp = torch.zeros(max(p.tmp_bytes, 64), dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    if p.n_streams:
        hip.lz4_decode_streams(comp, st, p.n_streams, p.max_dsize, tmp, out, errors)
    if p.n_frames:
        scratch = torch.empty(hip.zstd_scratch_bytes(p), dtype=torch.uint8, device="cuda")
        hip.zstd_decode(comp, base.nbytes, fr, zb, p, scratch, tmp, errors)
    if p.n_shuf:
        hip.unshuffle_blocks(tmp, out, sh, p.n_shuf, p.max_shuf)
    if p.n_bits:
        hip.bitunshuffle_blocks(tmp, out, bt, p.n_bits, p.max_bits)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    got = [host[o:o + n] if r >= 0 else None for o, n, r in zip(out_off[:-1], nbytes, p.results)]
    return got, int(errors.item()), host


def _guards_untouched(host, out_off, nbytes):
    return all((host[o + n:nxt] == 0xAB).all() for o, n, nxt in zip(out_off[:-1], nbytes, out_off[1:]))


def test_real_cblosc_chunks_of_every_flavour_decode_in_one_batch(torch_cuda):
    chunks = [base64.b64decode(c["chunk_b64"]) for c in CASES]
    raws = [recipe(c["recipe"], c["n"], c["dtype"], c["seed"]) for c in CASES]
    nbytes = [r.nbytes for r in raws]
    base, out_off, lists, p = _plan(chunks, nbytes)
    assert p.n_streams and p.n_shuf and p.n_bits and p.n_frames          # one batch of mixed flavours
    got, nerr, host = _run(torch_cuda, base, out_off, lists, p, nbytes)
    assert nerr == 0
    taken = {}
    for c, ch, g, r in zip(CASES, chunks, got, raws):
        if ch[2] & 0x02 or c["cname"] in ("lz4", "lz4hc", "zstd"):
            assert g is not None and g.tobytes() == r.tobytes(), (c["cname"], c["shuffle"], c["dtype"], c["recipe"], c["n"])
            taken[(c["cname"], c["shuffle"])] = taken.get((c["cname"], c["shuffle"]), 0) + 1
        else:
            assert g is None and c["cname"] in ("blosclz", "zlib")
    assert all(taken.get((cn, s), 0) >= 3 for cn in ("lz4", "lz4hc", "zstd") for s in (0, 1, 2)), taken
    assert _guards_untouched(host, out_off, nbytes)


@pytest.mark.parametrize("ts", [1, 2, 3, 4, 8])
def test_bitunshuffle_kernel_against_the_numpy_reference(torch_cuda, ts):
    """`afhip_bitunshuffle_blocks` alone, many blocks of different sizes in one call: element counts around a wave's step, a count
    that is 5 mod 8 (the copy path), trailing bytes, destinations at 16-byte, 4-byte-only and odd alignment, guards all around."""
    from aggfly_amd import hip
    W = WAVE_ELEMENTS
    rng = np.random.default_rng(100 + ts)
    shapes = [(n, 0) for n in (8, W - 8, W, W + 8, 3 * W + 40, 13, 8 * 1024 + 8)]          # (elements, trailing bytes)
    if ts > 1:
        shapes += [(W + 8, ts - 1), (24, 1)]
    blocks, tmp_parts, tmp_at, out_at = [], [], 0, GUARD
    want = []
    for i, (n, extra) in enumerate(shapes * 3):
        bsize = n * ts + extra
        align = (0, 4, 1 if ts in (1, 3) else 8)[i // len(shapes)]                        # residue of out_off mod 16
        out_at = (out_at + 15) // 16 * 16 + align
        src = rng.integers(0, 256, bsize, dtype=np.uint8)
        blocks.append((tmp_at, out_at, bsize, ts))
        want.append((out_at, bit_unshuffle_reference(src, ts)))
        tmp_parts.append(src)
        tmp_parts.append(np.zeros(-bsize % 16 + 16, dtype=np.uint8))
        tmp_at += bsize + len(tmp_parts[-1])
        out_at += bsize + GUARD
    assert any(b[1] % 16 == 4 for b in blocks) and any(b[1] % 2 == 1 for b in blocks) == (ts in (1, 3))
    assert len({b[2] for b in blocks}) > 2
    rec = np.array(blocks, dtype=codec.SHUFFLE_BLOCK)
    expect = np.full(out_at, 0xAB, dtype=np.uint8)
    for o, w in want:
        expect[o:o + len(w)] = w
    tmp = torch_cuda.from_numpy(np.concatenate(tmp_parts)).cuda()
    out = torch_cuda.full((out_at,), 0xAB, dtype=torch_cuda.uint8, device="cuda")
    hip.bitunshuffle_blocks(tmp, out, torch_cuda.from_numpy(rec.view(np.uint8).copy()).cuda(), len(rec), int(rec["bsize"].max()))
    torch_cuda.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, (ts, bad[:8], [b for b in blocks if b[1] <= bad[0] < b[1] + b[2] + GUARD][:1])


@pytest.mark.parametrize("flavour", ["lz4-bitshuffle", "zstd-shuffle", "zstd-bitshuffle"])
@pytest.mark.parametrize("dtype,n", ff.ENCODER_SHAPES)
def test_in_tree_encoder_chunks_of_the_new_flavours_decode_in_hbm(torch_cuda, flavour, dtype, n):
    """Multi-block chunks, a short last block whose element count is not a multiple of 8, a tiny chunk, int16; data of every
    compressibility: smooth, noisy, constant (Zstandard RLE blocks), random (stored streams).  One batch per case."""
    xs = [ff.flavour_input(kind, dtype, n) for kind in ("smooth", "noisy", "constant", "random")]
    encs = [codec.blosc_encode(x, x.dtype.itemsize, **ff.FLAVOURS[flavour]) for x in xs]
    nbytes = [x.nbytes for x in xs]
    base, out_off, lists, p = _plan(encs, nbytes)
    assert (p.results == nbytes).all()
    got, nerr, host = _run(torch_cuda, base, out_off, lists, p, nbytes)
    assert nerr == 0
    for kind, g, x in zip(("smooth", "noisy", "constant", "random"), got, xs):
        assert g.tobytes() == x.tobytes(), kind
    assert _guards_untouched(host, out_off, nbytes)


def test_damaged_zstandard_payloads_are_counted_not_followed(torch_cuda):
    """Garbage in the payload of a Blosc-Zstandard chunk (the block table is kept) between two good chunks: the passes count the
    damaged frames — as many as their host emulation finds, which runs first —, the neighbours are bit-exact and the guards around
    the outputs untouched.  Trials the planner refuses are skipped."""
    rng = np.random.default_rng(6)
    n = 150_000
    x = (280 + 10 * np.sin(np.arange(n) / 50) + np.round(rng.normal(0, 0.05, n), 3)).astype("<f4")
    good = codec.blosc_encode(x, 4, cname="zstd", blocksize=131072)
    nblocks = -(-x.nbytes // 131072)
    assert codec.blosc_info(good)["codec"] == "zstd" and nblocks == 5
    total_err = ran = 0
    for trial in range(6):
        bad = bytearray(good)
        lo = 16 + 4 * nblocks + 64
        for _ in range(40):                                          # overwrite runs of payload bytes
            q = int(rng.integers(lo, len(bad) - 16))
            bad[q:q + 8] = rng.bytes(8)
        nbytes = [x.nbytes] * 3
        try:
            base, out_off, lists, p = _plan([good, bytes(bad), good], nbytes)
        except codec.CodecError:
            continue                                                 # a length prefix or a header was hit: refused by the planner
        if (p.results < 0).any():
            continue
        emu = np.full(p.tmp_bytes + GUARD, 0xAB, dtype=np.uint8)
        want_err, _ = codec.zstd_emulate(base, lists[3], lists[4], p, emu)
        assert (emu[p.tmp_bytes:] == 0xAB).all()
        got, nerr, host = _run(torch_cuda, base, out_off, lists, p, nbytes)
        ran += 1
        total_err += nerr
        assert nerr == want_err
        assert got[0].tobytes() == x.tobytes() and got[2].tobytes() == x.tobytes()        # the neighbours are intact
        assert _guards_untouched(host, out_off, nbytes)
    assert ran > 0 and total_err > 0


def _store(tmp_path, name, cube, chunks, compress):
    T, ny, nx = cube.shape
    ds = af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                 {"time": pd.date_range("2001-01-01", periods=T, freq="h"),
                                  "latitude": 30 + 0.25 * np.arange(ny), "longitude": 250 + 0.25 * np.arange(nx)}), lon_is_360=True)
    path = str(tmp_path / name)
    af.dataset_to_zarr(ds, path, var="t2m", chunks=chunks, compress=compress)
    return path


def _spy(monkeypatch):
    kinds = []
    real, real_packed = codec.decode_ranges, codec.read_packed
    monkeypatch.setattr(codec, "decode_ranges", lambda kind, locs, outs, threads=8, exact=True: kinds.append(kind) or real(kind, locs, outs, threads, exact))
    monkeypatch.setattr(codec, "read_packed", lambda locs, dst, align=64, threads=8: kinds.append("files as they are") or real_packed(locs, dst, align, threads))
    return kinds


@pytest.fixture(scope="module")
def store_cube():
    return synth.temperature_cube(480, 40, 64, dtype=np.float32, seed=3, ocean_frac=0.1, scattered_nan=40) + np.float32(273.15)


@pytest.mark.parametrize("layout", ["time_contiguous", "space_tiled", "whole_series_tiles"])
@pytest.mark.parametrize("compress", ["blosc-zstd", "blosc-bitshuffle", "blosc-zstd-bitshuffle"])
def test_stores_of_the_new_flavours_read_the_same_on_both_routes(torch_cuda, tmp_path, monkeypatch, store_cube, compress, layout):
    cube = store_cube
    T, ny, nx = cube.shape
    chunks = {"time_contiguous": {"time": 48, "latitude": ny, "longitude": nx}, "space_tiled": {"time": 100, "latitude": 16, "longitude": 24},
              "whole_series_tiles": {"time": T, "latitude": 8, "longitude": 16}}[layout]
    path = _store(tmp_path, "s.zarr", cube, chunks, compress)
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE_BATCH_MB", "1")
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE_HOST_TAIL_MIN_MB", "0")
    kinds = _spy(monkeypatch)
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "1")
    dev = af.dataset_from_path(path, "t2m", lon_is_360=True, device="cuda").cube().cpu().numpy()
    assert "files as they are" in kinds, kinds                      # the route was really taken
    kinds.clear()
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "0")
    host = af.dataset_from_path(path, "t2m", lon_is_360=True, device="cuda").cube().cpu().numpy()
    assert set(kinds) == {"blosc"}, kinds
    np.testing.assert_array_equal(dev, host)
    np.testing.assert_array_equal(dev, cube)


def test_store_that_turns_blosclz_midway_finishes_on_the_host_route(torch_cuda, tmp_path, monkeypatch):
    """The first chunk is Blosc-Zstandard, the 10th a blosclz chunk the real c-blosc wrote: the request starts on the GPU route, whose
    planner hands that chunk back, and comes out right through the host route."""
    case = next(c for c in CASES if c["cname"] == "blosclz" and c["shuffle"] == 1 and c["dtype"] == "<f4" and c["n"] == 6000)
    T, ny, nx = 60 * 12, 10, 10
    cube = synth.temperature_cube(T, ny, nx, dtype=np.float32, seed=8, scattered_nan=5) + np.float32(273.15)
    cube[540:600] = recipe(case["recipe"], case["n"], case["dtype"], case["seed"]).reshape(60, ny, nx)
    path = _store(tmp_path, "mixed.zarr", cube, {"time": 60, "latitude": ny, "longitude": nx}, "blosc-zstd")
    odd = os.path.join(path, "t2m", "9.0.0")
    assert os.path.exists(odd) and codec.blosc_info(open(os.path.join(path, "t2m", "0.0.0"), "rb").read())["codec"] == "zstd"
    with open(odd, "wb") as f:
        f.write(base64.b64decode(case["chunk_b64"]))
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "1")
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE_BATCH_MB", "1")
    kinds = _spy(monkeypatch)
    got = af.dataset_from_path(path, "t2m", lon_is_360=True, device="cuda")
    assert "files as they are" in kinds and "blosc" in kinds, kinds   # started on the GPU route, finished on the host route
    np.testing.assert_array_equal(got.cube().cpu().numpy(), cube)
