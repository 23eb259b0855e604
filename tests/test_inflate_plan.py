"""zlib (deflate) chunks on the decode-in-HBM route, host side: `afcodec_inflate_plan` reads the zlib wrapper of streams that the
real zlib wrote at test time (and of edge streams assembled by tests/inflate_cases.py's bit writer) into stream records that stay
inside their buffers; the GPU passes (aggfly_amd/csrc/inflate_passes.h), run on the host by `afcodec_inflate_emulate`, rebuild every
stream bit-exact and verify its Adler-32; malformed streams are refused without a byte outside their destination; 10^4 cut or
mutated streams never escape and never decode to anything zlib would not; and `io._gpu_decodable` picks the route for HDF5 /
netCDF-4 deflate chunks and Zarr v2 zlib stores by format, `GPU_DECODE_AUTO_BYTES_DEFLATE` and AGGFLY_HIP_GPU_DECODE."""
import os
import sys
import zlib

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inflate_cases as ic                       # noqa: E402

import aggfly_amd as af                          # noqa: E402
from aggfly_amd import codec, hdf5, io as afio   # noqa: E402

GOOD = ic.good_streams()
FIX = os.path.join(HERE, "golden", "hdf5")


def _check_records(base, co, cs, oo, nout, st, sh, p, sizes, typesize=1):
    """Every record inside its chunk, the batch's buffers and the destination."""
    st, sh = st[:p.n_streams], sh[:p.n_shuf]
    taken = np.nonzero(p.results >= 0)[0]
    assert len(taken) == p.n_streams and p.dec_bytes == int(st["dsize"].sum()) < 2 ** 31
    dec = nsq = nb = npc = tmp = nsh = 0
    for rec, i in zip(st, taken):
        assert rec["src"] == co[i] and rec["csize"] == cs[i] and rec["src"] + rec["csize"] <= base.size
        assert rec["dsize"] == sizes[i] == p.results[i]
        assert rec["base"] == dec and rec["seq_off"] == nsq and rec["first_block"] == nb and rec["first_piece"] == npc
        assert rec["n_blocks"] == rec["dsize"] // (131072 - 257) + 1
        if rec["to_out"]:
            assert rec["dst_off"] == oo[i] and rec["dst_off"] + rec["dsize"] <= nout
        else:
            k = sh[nsh]
            assert rec["dst_off"] == tmp == k["tmp_off"] and k["out_off"] == oo[i] and k["bsize"] == rec["dsize"] and k["typesize"] == typesize
            assert k["out_off"] + k["bsize"] <= nout
            tmp += (int(rec["dsize"]) + 15) // 16 * 16
            nsh += 1
        dec += int(rec["dsize"]); nsq += int(rec["dsize"]) // 3 + 1; nb += int(rec["n_blocks"]); npc += -(-int(rec["dsize"]) // 65536)
    assert (nb, nsq, npc, tmp, nsh) == (p.n_pblocks, p.n_seqs, p.n_pieces, p.tmp_bytes, p.n_shuf)
    assert p.scratch_bytes() >= p.dec_bytes * 5 + p.n_seqs * 12 + p.tmp_bytes


def _emulate(streams, sizes, typesize=1, strict=True):
    base, co, cs, oo, nout, st, sh, p = ic.plan(streams, sizes, typesize, strict)
    _check_records(base, co, cs, oo, nout, st, sh, p, np.asarray(sizes), typesize)
    out = np.full(nout, 0xA5, dtype=np.uint8)
    errors, rounds = codec.inflate_emulate(base, st, sh, p, out)
    assert (out[ic.canary_mask(nout, oo, sizes)] == 0xA5).all()
    return p, out, oo, errors


def test_the_cube_streams_hold_many_dynamic_blocks():
    """A guard on the generators of tests/inflate_cases.py, not on the decoder (it passes without it): the streams are what zlib
    reads, and they hold the block kinds the other tests rely on — per cube stream 10 blocks and more, 3 to 10 of them dynamic."""
    assert len(ic.SHUF) == 199680
    for name, s, raw in GOOD:
        assert zlib.decompress(s) == raw, name
        if name.startswith("cube level"):
            assert 140000 < len(s) < 170000, (name, len(s))
    # two of the four byte planes are noise (stored blocks), the others compress: every stream holds 10 blocks or more, several of
    # them dynamic — 40 and more dynamic blocks over the set, all three kinds in it
    types = {n: ic.block_types(s_) for n, s_, _ in GOOD}
    for n, t in types.items():
        if n.startswith("cube") and n != "cube Z_FIXED":
            assert len(t) >= 10 and t.count(2) >= 3, (n, t)
    assert types["cube wbits 9"].count(2) >= 10 and types["cube Z_FIXED"].count(1) >= 4
    assert sum(t.count(2) for t in types.values()) >= 40
    assert types["noise level 0"] == [0, 0] and types["far match"] == [0, 1]


@pytest.mark.parametrize("one_per_call", [False, True])
def test_gpu_passes_on_the_host_match_zlib(one_per_call):
    groups = [[x] for x in GOOD] if one_per_call else [GOOD]
    for g in groups:
        p, out, oo, errors = _emulate([s for _, s, _ in g], [len(r) for _, _, r in g])
        assert errors == 0 and (p.results >= 0).all()
        for (name, _, raw), o in zip(g, oo):
            assert out[o:o + len(raw)].tobytes() == raw, name


@pytest.mark.parametrize("typesize", [2, 4, 8])
def test_shuffled_chunks_come_out_unshuffled(typesize):
    raws = [ic.CUBE.tobytes(), ic.CUBE.tobytes()[:50001], b"abc", b""]      # (a tail that is no whole element; less than one element)
    streams = [zlib.compress(ic.shuffle(r, typesize), 4) for r in raws]
    p, out, oo, errors = _emulate(streams, [len(r) for r in raws], typesize)
    assert errors == 0 and p.n_shuf == sum(len(r) >= typesize for r in raws)
    for raw, o in zip(raws, oo):
        assert out[o:o + len(raw)].tobytes() == raw


def test_far_match_is_what_zlib_never_writes():
    s, raw = ic.far_match_stream()
    assert zlib.decompress(s) == raw
    p, out, oo, errors = _emulate([s], [len(raw)])
    assert errors == 0 and out[oo[0]:oo[0] + len(raw)].tobytes() == raw


@pytest.mark.parametrize("case", ic.refused_streams(), ids=lambda c: c[0])
def test_malformed_streams_are_refused_inside_their_destination(case):
    name, s, n = case
    if "plan" not in name:                       # (those two are valid streams of another size)
        with pytest.raises(zlib.error):
            zlib.decompress(s)
    p, out, oo, errors = _emulate([s], [n])
    assert p.results[0] == n and errors == 1, name
    good = GOOD[1]                               # between two good streams: they decode, the bad one counts once
    p, out, oo, errors = _emulate([good[1], s, good[1]], [1, n, 1])
    assert errors == 1 and out[oo[0]] == out[oo[2]] == good[2][0]


def test_preset_dictionary_gzip_and_foreign_headers_leave_no_record():
    c = zlib.compressobj(zdict=b"temperature")
    fdict = c.compress(b"temperature field") + c.flush()
    import gzip
    for s, want in ((fdict, codec.E_UNSUPPORTED), (gzip.compress(b"abc"), codec.E_UNSUPPORTED), (b"\x79\x9c" + b"\0" * 8, -1),
                    (b"\x78\x9d" + b"\0" * 8, -1), (b"\x88\x1c" + b"\0" * 8, -1), (b"\x78", -1)):
        *_, st, sh, p = ic.plan([s], [17], strict=False)
        assert p.results[0] == want and p.n_streams == 0 and p.n_pblocks == 0 and p.dec_bytes == 0
    with pytest.raises(codec.CodecError):
        ic.plan([b"\x79\x9c" + b"\0" * 8], [17])


def test_mutated_and_truncated_streams_never_escape():
    """10^4 damaged streams: every record stays inside its buffers, the emulated passes leave the canaries around the destination
    alone, and whatever they accept is what zlib decodes from the same bytes."""
    rng = np.random.default_rng(2025)
    small = [(s, r) for _, s, r in GOOD if len(s) < 65536]
    assert len(small) >= 8
    emulated = clean = 0
    for it in range(10000):
        s, raw = small[int(rng.integers(len(small)))]
        m = ic.mutate(rng, it, s)
        base, co, cs, oo, nout, st, sh, p = ic.plan([m], [len(raw)], strict=False)
        if p.results[0] < 0:
            assert p.n_streams == 0
            continue
        _check_records(base, co, cs, oo, nout, st, sh, p, np.array([len(raw)]))
        out = np.full(nout, 0x5A, dtype=np.uint8)
        errors, _ = codec.inflate_emulate(base, st, sh, p, out)
        emulated += 1
        assert errors in (0, 1)
        assert (out[:oo[0]] == 0x5A).all() and (out[oo[0] + len(raw):] == 0x5A).all()
        if errors == 0:
            clean += 1
            assert out[oo[0]:oo[0] + len(raw)].tobytes() == zlib.decompress(m)
    assert emulated >= 2000
    print("emulated", emulated, "decoded clean", clean)


def _zarr(tmp_path, name, fmt, compress):
    from aggfly_amd import synth
    T, ny, nx = 240, 6, 8
    cube = synth.temperature_cube(T, ny, nx, dtype=np.float32, seed=3)
    time = pd.date_range("2001-01-01", periods=T, freq="h")
    ds = af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                 {"time": time, "latitude": 30 + 0.5 * np.arange(ny), "longitude": 200 + 0.5 * np.arange(nx)}))
    path = str(tmp_path / name)
    af.dataset_to_zarr(ds, path, var="t2m", chunks={"time": 48, "latitude": ny, "longitude": nx}, compress=compress, zarr_format=fmt)
    return afio.ZarrArray(os.path.join(path, "t2m"))


def test_route_choice_for_deflate_sources(tmp_path, monkeypatch):
    files = [hdf5.H5File(os.path.join(FIX, fn)) for fn in ("nc4_like.nc", "old_style.h5")]
    try:
        srcs = [hdf5.ChunkSource(f.datasets["t2m"]) for f in files]
        assert srcs[0].native_kind == ("zlib", 4) and srcs[1]._trailer == 4
        assert srcs[0].chunk_locator((0, 0, 0), probe=False) == srcs[0].chunk_locator((0, 0, 0))
        srcs.append(_zarr(tmp_path, "v2.zarr", 2, "zlib"))
        assert srcs[2].native_kind == "zlib"
        auto = afio.GPU_DECODE_AUTO_BYTES_DEFLATE
        assert auto is None or auto >= 64 << 20          # the small files of the existing tests stay on the host route under auto
        cases = [("0", 1 << 40, False), ("1", 1, True)]
        cases += [("auto", 1 << 40, False)] if auto is None else [("auto", auto - 1, False), ("auto", auto, True)]
        for za in srcs:
            for mode, nbytes, want in cases:
                monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
                if hasattr(za, "_gpu_decodable"):
                    delattr(za, "_gpu_decodable")
                assert afio._gpu_decodable(za, nbytes) is want, (za.path, mode, nbytes)
        monkeypatch.delenv("AGGFLY_HIP_GPU_DECODE")
        assert afio._gpu_decodable(srcs[0], 1 << 20) is False
        for za in (_zarr(tmp_path, "v3.zarr", 3, "zlib"), _zarr(tmp_path, "raw.zarr", 2, False)):
            assert za.native_kind in ("gzip", "raw")
            for mode in ("0", "1", "auto"):
                monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
                assert afio._gpu_decodable(za, 1 << 40) is False
    finally:
        for f in files:
            f.close()
    assert afio._zlib_header_taken(b"\x78\x9c") and afio._zlib_header_taken(b"\x18\x19")
    assert not afio._zlib_header_taken(b"\x78\xbb") and not afio._zlib_header_taken(b"\x1f\x8b") and not afio._zlib_header_taken(b"\x78")
