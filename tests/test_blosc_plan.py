"""Blosc-1 chunks of every flavour the decode-in-HBM route takes, host side: `afcodec_blosc_plan` walks chunks the real c-blosc
1.21 wrote (tests/golden/blosc_fixtures.json, blosc_flavour_fixtures.json) — stored, LZ4, LZ4HC and Zstandard inside, shuffle none,
byte or bit — into its five record lists, which are then EXECUTED on the host: LZ4 streams by liblz4 (pyarrow's lz4_raw), Zstandard
frames by the GPU passes themselves (`afcodec_zstd_emulate`), the byte unshuffle by numpy and the bit unshuffle by a numpy
reference that does not call the library.  Mutated and truncated chunks never crash the planner nor yield a record outside the
batch; `afcodec_blosc_lz4_plan`, now a filter over the same walk, still gives the records it gave before; the in-tree encoder's new
flavours are what c-blosc was shown to read; `io._gpu_decodable` picks route and threshold by flavour; and `dataset_to_zarr` writes
the three new flavours in both Zarr formats.  CPU only."""
import base64
import hashlib
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
import make_blosc_lz4_plan_golden as lg         # noqa: E402

import aggfly_amd as af                          # noqa: E402
from aggfly_amd import codec, io as afio         # noqa: E402

OLD = json.load(open(os.path.join(HERE, "golden", "blosc_fixtures.json")))["cases"]
NEW = ff.load()
CASES = OLD + NEW["cases"]
GAP = 64


def _id(c):
    return f"{c['cname']}-s{c['shuffle']}-{c['dtype'][1:]}-{c['recipe']}-{c['n']}-b{c['blocksize']}-l{c['clevel']}"


def takes(case, chunk):
    """What the GPU route takes: stored chunks, and LZ4 / LZ4HC / Zstandard streams under any shuffle."""
    return bool(chunk[2] & 0x02) or case["cname"] in ("lz4", "lz4hc", "zstd")


def bit_unshuffle_reference(src: np.ndarray, ts: int) -> np.ndarray:
    """Blosc's bit shuffle undone for one block, in numpy alone."""
    bsize = len(src)
    n = bsize // ts
    out = src.copy()
    if n % 8 != 0 or n == 0:
        return out
    bits = np.unpackbits(src[:n * ts].reshape(ts * 8, n // 8), axis=1, bitorder="little")
    out[:n * ts] = np.packbits(bits.reshape(ts, 8, n).transpose(2, 0, 1), axis=2, bitorder="little").reshape(n * ts)
    return out


def pack(chunks, nbytes):
    """Chunks back to back at 64-byte steps, outputs with `GAP` bytes between them -> (base, comp_off, comp_size, out_off, n_out)."""
    co = np.concatenate([[0], np.cumsum([(len(c) + 63) // 64 * 64 for c in chunks])]).astype(np.int64)
    base = np.zeros(max(int(co[-1]), 1), dtype=np.uint8)
    for o, c in zip(co, chunks):
        base[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)
    oo = GAP + np.concatenate([[0], np.cumsum([n + GAP for n in nbytes])]).astype(np.int64)
    return base, co[:-1], np.array([len(c) for c in chunks], dtype=np.int64), oo[:-1], int(oo[-1])


class Lists:
    def __init__(self, n_streams=1 << 14, n_blocks=4096, n_zblocks=4096):
        self.streams = np.zeros(n_streams, dtype=codec.LZ4_STREAM)
        self.shuf, self.bits = np.zeros(n_blocks, dtype=codec.SHUFFLE_BLOCK), np.zeros(n_blocks, dtype=codec.SHUFFLE_BLOCK)
        self.frames, self.zblocks = np.zeros(n_blocks, dtype=codec.ZSTD_FRAME), np.zeros(n_zblocks, dtype=codec.ZSTD_BLOCK)

    def plan(self, base, co, cs, oo, nbytes, strict=True):
        return codec.blosc_plan(base, co, cs, oo, nbytes, self.streams, self.shuf, self.bits, self.frames, self.zblocks, strict=strict)


def check_records(L, p, co, cs, oo, nbytes, n_out):
    """Every record inside its chunk, the batch's buffers (shuffle scratch, literal / sequence buffers) and a chunk's destination."""
    ok = [i for i in range(len(co)) if p.results[i] >= 0]
    assert all(p.results[i] <= nbytes[i] for i in ok)
    src_lo, src_hi = np.asarray(co), np.asarray(co) + np.asarray(cs)
    dst_lo, dst_hi = np.asarray(oo), np.asarray(oo) + np.maximum(p.results, 0)

    def in_a_chunk(a, b):
        return any(src_lo[i] + 16 <= a and b <= src_hi[i] for i in ok)

    def in_a_destination(a, b):
        return any(dst_lo[i] <= a and b <= dst_hi[i] for i in ok)

    assert 0 <= p.tmp_bytes
    for s in L.streams[:p.n_streams]:
        assert s["csize"] >= 0 and s["dsize"] > 0 and in_a_chunk(int(s["src_off"]), int(s["src_off"] + s["csize"]))
        if s["to_out"]:
            assert in_a_destination(int(s["dst_off"]), int(s["dst_off"] + s["dsize"]))
        else:
            assert 0 <= s["dst_off"] and s["dst_off"] + s["dsize"] <= p.tmp_bytes
        assert s["csize"] != s["dsize"] or s["dsize"] <= max(65536, p.max_dsize)
    for rec in list(L.shuf[:p.n_shuf]) + list(L.bits[:p.n_bits]):
        assert rec["bsize"] > 0 and 1 <= rec["typesize"] <= 255
        assert 0 <= rec["tmp_off"] and rec["tmp_off"] + rec["bsize"] <= p.tmp_bytes
        assert in_a_destination(int(rec["out_off"]), int(rec["out_off"] + rec["bsize"]))
    assert p.max_shuf == (int(L.shuf["bsize"][:p.n_shuf].max()) if p.n_shuf else 0)
    fr, bl = L.frames[:p.n_frames], L.zblocks[:p.n_blocks]
    assert p.dec_bytes == int(fr["size"].sum()) and p.lit_bytes + 3 * p.n_seqs <= p.dec_bytes
    base_pos = lit = nsq = nb = 0
    for f, rec in enumerate(fr):
        assert rec["base"] == base_pos and 0 <= rec["dst_off"] and rec["dst_off"] + rec["size"] <= p.tmp_bytes
        base_pos += int(rec["size"])
        assert rec["first_block"] == nb and rec["n_blocks"] >= 1
        for b in range(nb, nb + int(rec["n_blocks"])):
            k = bl[b]
            assert k["frame"] == f and in_a_chunk(int(k["src"]), int(k["src"] + k["csize"]))
            assert k["lit_off"] == lit and k["seq_off"] == nsq and 0 <= k["lit_size"] <= 131072 and k["btype"] in (0, 1, 2)
            lit += int(k["lit_size"]); nsq += int(k["nseq"])
            if k["btype"] == 2:
                assert 0 < k["lit_src"] <= k["csize"] and k["lit_src"] + k["lit_csize"] <= k["csize"]
                if k["lit_type"] >= 2:
                    assert rec["first_block"] <= k["huf_block"] <= b
                if k["nseq"]:
                    assert k["lit_src"] <= k["seq_src"] < k["csize"]
                    assert all(k["mode"][t] != 2 or rec["first_block"] <= k["tab_block"][t] <= b for t in range(3))
        nb += int(rec["n_blocks"])
    assert nb == p.n_blocks and lit == p.lit_bytes and nsq == p.n_seqs


def execute(L, p, base, n_out, fill=0xAB):
    """The plan run on the host, in the order of the GPU route -> (out, Zstandard errors)."""
    import pyarrow as pa
    out = np.full(n_out, fill, dtype=np.uint8)
    tmp = np.full(p.tmp_bytes + 1, 0xCD, dtype=np.uint8)
    for s in L.streams[:p.n_streams]:
        src = base[s["src_off"]:s["src_off"] + s["csize"]].tobytes()
        dec = src if s["csize"] == s["dsize"] else pa.Codec("lz4_raw").decompress(src, decompressed_size=int(s["dsize"]), asbytes=True)
        assert len(dec) == s["dsize"]
        (out if s["to_out"] else tmp)[s["dst_off"]:s["dst_off"] + s["dsize"]] = np.frombuffer(dec, dtype=np.uint8)
    errors = 0
    if p.n_frames:
        errors, _ = codec.zstd_emulate(base, L.frames, L.zblocks, p, tmp)
    assert tmp[p.tmp_bytes] == 0xCD
    for b in L.shuf[:p.n_shuf]:
        ts, bs = int(b["typesize"]), int(b["bsize"])
        n = bs // ts
        src = tmp[b["tmp_off"]:b["tmp_off"] + bs]
        out[b["out_off"]:b["out_off"] + n * ts] = src[:n * ts].reshape(ts, n).T.reshape(-1)
        out[b["out_off"] + n * ts:b["out_off"] + bs] = src[n * ts:]
    for b in L.bits[:p.n_bits]:
        out[b["out_off"]:b["out_off"] + b["bsize"]] = bit_unshuffle_reference(tmp[b["tmp_off"]:b["tmp_off"] + b["bsize"]], int(b["typesize"]))
    return out, errors


def check_output(out, oo, raws, results, fill=0xAB):
    canary = np.ones(len(out), dtype=bool)
    for o, raw, r in zip(oo, raws, results):
        if r >= 0:
            assert out[o:o + len(raw)].tobytes() == raw
            canary[o:o + len(raw)] = False
    assert (out[canary] == fill).all()


def test_flavour_fixtures_hold_frames_of_several_zstandard_blocks():
    for c in NEW["cases"]:
        raw = recipe(c["recipe"], c["n"], c["dtype"], c["seed"])
        assert hashlib.sha256(raw.tobytes()).hexdigest() == c["sha256"] and c["nbytes"] >= 600000
        chunk = base64.b64decode(c["chunk_b64"])
        assert codec.blosc_decode(chunk).tobytes() == raw.tobytes()
        assert codec.blosc_info(chunk)["blocksize"] >= (256 << 10) or c["cname"] != "zstd"
    assert os.path.getsize(os.path.join(HERE, "golden", "blosc_flavour_fixtures.json")) < 1 << 20


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_plan_of_every_real_cblosc_chunk_executes_bit_exact(case):
    chunk = base64.b64decode(case["chunk_b64"])
    raw = recipe(case["recipe"], case["n"], case["dtype"], case["seed"]).tobytes()
    L = Lists()
    base, co, cs, oo, n_out = pack([chunk], [len(raw)])
    p = L.plan(base, co, cs, oo, [len(raw)])
    if not takes(case, chunk):
        assert case["cname"] in ("blosclz", "zlib") and p.results[0] == codec.E_UNSUPPORTED
        assert (p.n_streams, p.n_shuf, p.n_bits, p.n_frames, p.n_blocks, p.tmp_bytes) == (0,) * 6
        return
    assert p.results[0] == len(raw)
    check_records(L, p, co, cs, oo, [len(raw)], n_out)
    info = codec.blosc_info(chunk)
    if not info["stored"]:
        assert bool(p.n_frames) == (case["cname"] == "zstd" and p.n_frames > 0)
        assert bool(p.n_bits) == (case["shuffle"] == 2)
        if case["cname"] == "zstd" and case in NEW["cases"]:
            assert int(L.frames["n_blocks"][:p.n_frames].max()) > 1          # frames of more than one Zstandard block
    out, errors = execute(L, p, base, n_out)
    assert errors == 0
    check_output(out, oo, [raw], p.results)


def test_one_batch_of_every_flavour():
    chunks = [base64.b64decode(c["chunk_b64"]) for c in CASES]
    raws = [recipe(c["recipe"], c["n"], c["dtype"], c["seed"]).tobytes() for c in CASES]
    nbytes = [len(r) for r in raws]
    L = Lists(1 << 15, 1 << 13, 1 << 13)
    base, co, cs, oo, n_out = pack(chunks, nbytes)
    p = L.plan(base, co, cs, oo, nbytes)
    for c, ch, r, raw in zip(CASES, chunks, p.results, raws):
        assert r == (len(raw) if takes(c, ch) else codec.E_UNSUPPORTED), _id(c)
    assert p.n_streams and p.n_shuf and p.n_bits and p.n_frames
    check_records(L, p, co, cs, oo, nbytes, n_out)
    out, errors = execute(L, p, base, n_out)
    assert errors == 0
    check_output(out, oo, raws, p.results)
    # too few records of any list is a capacity error, not damage
    for small in (Lists(8), Lists(n_blocks=2), Lists(n_zblocks=2)):
        with pytest.raises(codec.PlanCapacityError):
            small.plan(base, co, cs, oo, nbytes)


def test_mutated_and_truncated_chunks_never_escape():
    """More than 10^4 damaged chunks: the planner never crashes and never emits a record outside the chunk, the batch's buffers or
    the destination; a plan it accepts runs through the host emulation of the Zstandard passes inside the scratch."""
    rng = np.random.default_rng(2025)
    small = [(c, base64.b64decode(c["chunk_b64"])) for c in OLD if c["cname"] in ("lz4", "lz4hc", "zstd") and c["cbytes"] < 40000]
    assert {c["cname"] for c, _ in small} == {"lz4", "lz4hc", "zstd"} and {c["shuffle"] for c, _ in small} == {0, 1, 2}
    L = Lists(1 << 12, 1 << 10, 1 << 10)
    accepted = emulated = with_frames = 0
    for it in range(12000):
        c, chunk = small[int(rng.integers(len(small)))]
        b = bytearray(chunk)
        kind = it % 4
        if kind == 0:
            b = b[:int(rng.integers(1, len(b)))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                # header, block table and first stream headers; anywhere; single bit flips
                j = int(rng.integers(0, min(len(b), 64))) if kind == 3 else int(rng.integers(0, len(b)))
                b[j] = b[j] ^ (1 << int(rng.integers(8))) if kind == 2 else int(rng.integers(256))
        nbytes = [c["nbytes"]]
        base, co, cs, oo, n_out = pack([bytes(b)], nbytes)
        p = L.plan(base, co, cs, oo, nbytes, strict=False)
        if p.results[0] < 0:
            assert (p.n_streams, p.n_shuf, p.n_bits, p.n_frames, p.n_blocks, p.tmp_bytes) == (0,) * 6
            continue
        accepted += 1
        check_records(L, p, co, cs, oo, nbytes, n_out)
        if p.n_frames:
            with_frames += 1
            if it % 3 == 0:
                tmp = np.full(p.tmp_bytes + 64, 0x5A, dtype=np.uint8)
                codec.zstd_emulate(base, L.frames, L.zblocks, p, tmp)
                assert (tmp[p.tmp_bytes:] == 0x5A).all()
                emulated += 1
    assert accepted > 1000 and with_frames > 100 and emulated > 30


def test_lz4_planner_gives_the_records_it_gave_before():
    """`afcodec_blosc_lz4_plan` is now a filter over the shared walk: for every fixture chunk its stream and block records are, byte
    for byte, those of the planner before that change (tests/golden/blosc_lz4_plan_golden.json), and it still refuses Zstandard
    and bit-shuffled chunks."""
    gold = json.load(open(os.path.join(HERE, "golden", "blosc_lz4_plan_golden.json")))
    assert len(gold["cases"]) == len(OLD)
    planned = 0
    for c, g in zip(OLD, gold["cases"]):
        res, d = lg.plan_digest(codec.load(), base64.b64decode(c["chunk_b64"]), c["nbytes"], gold["out_off"])
        assert res == g["result"] and d == g["records"], _id(c)
        stored = bool(base64.b64decode(c["chunk_b64"])[2] & 0x02)
        assert (res >= 0) == (stored or (c["cname"] in ("lz4", "lz4hc") and c["shuffle"] != 2))
        planned += d is not None
    assert planned >= 30
    for c in NEW["cases"]:
        assert lg.plan_digest(codec.load(), base64.b64decode(c["chunk_b64"]), c["nbytes"])[0] == codec.E_UNSUPPORTED


def test_bit_shuffle_of_the_encoder_is_the_inverse_of_the_reference():
    rng = np.random.default_rng(5)
    for ts, n, extra in ((1, 4096, 0), (2, 800, 0), (3, 264, 0), (4, 1000, 0), (8, 520, 0), (4, 133, 0), (4, 64, 3)):
        raw = rng.integers(0, 256, n * ts + extra, dtype=np.uint8)
        enc = codec.blosc_encode(raw, ts, cname="lz4", bitshuffle=True, blocksize=n * ts + extra)
        info = codec.blosc_info(enc)
        assert info["shuffle"] == 2 and codec.blosc_decode(enc).tobytes() == raw.tobytes()
        L = Lists()
        base, co, cs, oo, n_out = pack([enc], [len(raw)])
        p = L.plan(base, co, cs, oo, [len(raw)])
        assert p.n_bits == 1 and p.n_shuf == 0
        out, _ = execute(L, p, base, n_out)
        check_output(out, oo, [raw.tobytes()], p.results)


@pytest.mark.parametrize("flavour", sorted(ff.FLAVOURS))
@pytest.mark.parametrize("dtype,n", ff.ENCODER_SHAPES)
def test_encoder_flavours_round_trip_and_are_what_cblosc_read(flavour, dtype, n):
    kw = ff.FLAVOURS[flavour]
    x = ff.flavour_input("smooth", dtype, n)
    enc = codec.blosc_encode(x, x.dtype.itemsize, **kw)
    info = codec.blosc_info(enc)
    assert codec.blosc_decode(enc).tobytes() == x.tobytes()
    if n >= 128:
        assert info["codec"] == kw["cname"] and info["shuffle"] == (2 if kw.get("bitshuffle") else int(kw.get("shuffle", True)))
        assert info["split"] == (kw["cname"] == "lz4")                      # Zstandard blocks are never split, as c-blosc writes them
        assert info["blocksize"] == (min(256 << 10, x.nbytes) if kw["cname"] == "zstd" else min(65536 * x.dtype.itemsize, x.nbytes))
    if n > 1000:
        assert len(enc) < x.nbytes
    case = NEW["encoder"][ff.encoder_case_id(flavour, dtype, n)]
    assert hashlib.sha256(x.tobytes()).hexdigest() == case["input_sha256"]
    if kw["cname"] == "lz4" or ff.zstd_version() == NEW["zstd_version"]:
        # the very chunk the real c-blosc decoded back to x when the fixture was made (Zstandard bytes: by the same libzstd only)
        assert hashlib.sha256(enc).hexdigest() == case["chunk_sha256"] and len(enc) == case["chunk_bytes"]
    L = Lists()
    base, co, cs, oo, n_out = pack([enc], [x.nbytes])
    p = L.plan(base, co, cs, oo, [x.nbytes])
    check_records(L, p, co, cs, oo, [x.nbytes], n_out)
    out, errors = execute(L, p, base, n_out)
    assert errors == 0
    check_output(out, oo, [x.tobytes()], p.results)


def test_encoder_with_the_old_arguments_writes_the_old_bytes():
    lib = codec.load()
    for dtype, n, shuffle, blocksize in (("<f4", 100000, True, 0), ("<f8", 33333, True, 65536), ("<i2", 5000, False, 4096), ("<f4", 17, True, 0)):
        x = ff.flavour_input("smooth", dtype, n)
        dst = np.empty(lib.afcodec_blosc_bound(x.nbytes, blocksize), dtype=np.uint8)
        r = lib.afcodec_blosc_encode_lz4(x.ctypes.data, x.nbytes, x.dtype.itemsize, int(shuffle), blocksize, dst.ctypes.data, dst.nbytes)
        assert r > 0 and codec.blosc_encode(x, x.dtype.itemsize, shuffle, blocksize) == dst[:r].tobytes()
    with pytest.raises(KeyError):
        codec.blosc_encode(np.zeros(8, np.uint8), 1, cname="zlib")


def _store(tmp_path, name, fmt, chunks, compress, T=240, ny=6, nx=8):
    from aggfly_amd import synth
    cube = synth.temperature_cube(T, ny, nx, dtype=np.float32, seed=3, scattered_nan=5)
    time = pd.date_range("2001-01-01", periods=T, freq="h")
    ds = af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                 {"time": time, "latitude": 30 + 0.5 * np.arange(ny), "longitude": 200 + 0.5 * np.arange(nx)}))
    path = str(tmp_path / name)
    af.dataset_to_zarr(ds, path, var="t2m", chunks=chunks, compress=compress, zarr_format=fmt)
    return cube, path


FLAVOUR_OF = {"blosc": (1, 1), "blosc-bitshuffle": (1, 2), "blosc-zstd": (4, 1), "blosc-zstd-bitshuffle": (4, 2)}


@pytest.mark.parametrize("fmt", [2, 3])
@pytest.mark.parametrize("compress", ["blosc-zstd", "blosc-bitshuffle", "blosc-zstd-bitshuffle"])
def test_writer_flavours_read_back_on_the_host_route(tmp_path, monkeypatch, compress, fmt):
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "0")
    cube, path = _store(tmp_path, "s.zarr", fmt, {"time": 48, "latitude": 6, "longitude": 4}, compress)
    za = afio.ZarrArray(os.path.join(path, "t2m"))
    assert za.native_kind == "blosc"
    assert np.array_equal(za.read(), cube, equal_nan=True)
    loc = za.chunk_locator((0, 0, 0))
    info = codec.blosc_info(open(loc[0], "rb").read())
    assert (4 if info["codec"] == "zstd" else 1, info["shuffle"]) == FLAVOUR_OF[compress] and info["typesize"] == 4
    meta = json.load(open(os.path.join(path, "t2m", ".zarray" if fmt == 2 else "zarr.json")))
    if fmt == 2:
        assert meta["compressor"]["cname"] == ("zstd" if "zstd" in compress else "lz4")
        assert meta["compressor"]["shuffle"] == (2 if "bitshuffle" in compress else 1)
    else:
        conf = meta["codecs"][-1]["configuration"]
        assert meta["codecs"][-1]["name"] == "blosc" and conf["cname"] == ("zstd" if "zstd" in compress else "lz4")
        assert conf["shuffle"] == ("bitshuffle" if "bitshuffle" in compress else "shuffle")
    with pytest.raises(ValueError, match="compress must be"):
        _store(tmp_path, "bad.zarr", fmt, {"time": 48, "latitude": 6, "longitude": 4}, "blosc-snappy")


def test_route_choice_by_flavour(tmp_path, monkeypatch):
    """`_gpu_decodable` by flavour and mode: the two new constants (an int, or None = opt-in) rule the new flavours; LZ4 + byte
    shuffle keeps its two thresholds and `_Lz4Route`."""
    for name in ("GPU_DECODE_AUTO_BYTES_BLOSC_BITSHUFFLE", "GPU_DECODE_AUTO_BYTES_BLOSC_ZSTD"):
        v = getattr(afio, name)
        assert v is None or (isinstance(v, int) and v >= 64 << 20), name      # (the small stores of the suite stay on the host under auto)
    assert (afio.GPU_DECODE_AUTO_BYTES, afio.GPU_DECODE_AUTO_BYTES_WHOLE_ROWS) == (96 << 20, 256 << 20)
    huge = 1 << 40
    for compress, flavour in FLAVOUR_OF.items():
        for chunks, whole in (({"time": 48, "latitude": 6, "longitude": 8}, True), ({"time": 240, "latitude": 3, "longitude": 4}, False)):
            _, path = _store(tmp_path, f"{compress}-{int(whole)}.zarr", 2, chunks, compress)
            za = afio.ZarrArray(os.path.join(path, "t2m"))
            const = (afio.GPU_DECODE_AUTO_BYTES_BLOSC_ZSTD if flavour[0] == 4 else afio.GPU_DECODE_AUTO_BYTES_BLOSC_BITSHUFFLE if flavour[1] == 2
                     else afio.GPU_DECODE_AUTO_BYTES_WHOLE_ROWS if whole else afio.GPU_DECODE_AUTO_BYTES)
            assert afio._blosc_auto_bytes(flavour, whole) == const
            want = [("0", huge, False), ("1", 1, True), ("auto", 1, False), ("auto", huge, const is not None)]
            if const is not None:
                want += [("auto", const - 1, False), ("auto", const, True)]
            for mode, nbytes, expect in want:
                monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
                if hasattr(za, "_gpu_decodable"):
                    del za._gpu_decodable
                assert afio._gpu_decodable(za, nbytes) is expect, (compress, whole, mode, nbytes)
            assert za._blosc_flavour == flavour and za._blosc_geometry[1] == 4
    # another inner codec is not taken, whatever the mode
    case = next(c for c in OLD if c["cname"] == "blosclz" and c["shuffle"] == 1 and c["dtype"] == "<f4" and c["n"] == 6000)
    d = tmp_path / "lz" / "t2m"
    os.makedirs(d)
    json.dump({"zarr_format": 2, "shape": [60, 10, 10], "chunks": [60, 10, 10], "dtype": "<f4", "fill_value": "NaN", "order": "C", "filters": None,
               "compressor": {"id": "blosc", "cname": "blosclz", "clevel": 5, "shuffle": 1, "blocksize": 0}}, open(d / ".zarray", "w"))
    json.dump({"_ARRAY_DIMENSIONS": ["time", "latitude", "longitude"]}, open(d / ".zattrs", "w"))
    open(d / "0.0.0", "wb").write(base64.b64decode(case["chunk_b64"]))
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "1")
    assert afio._gpu_decodable(afio.ZarrArray(str(d)), huge) is False
