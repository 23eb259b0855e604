"""Zstandard frames on the decode-in-HBM route, host side: `afcodec_zstd_plan` walks the headers of frames the real libzstd
wrote (tests/golden/zstd_fixtures.json) into block records that stay inside their buffers; the GPU passes
(aggfly_amd/csrc/zstd_passes.h), run on the host by `afcodec_zstd_emulate`, rebuild every frame bit-exact; mutated and
truncated frames never crash the planner nor yield a record outside the batch; and `io._gpu_decodable` picks the route for
zstd stores by format, size threshold and AGGFLY_HIP_GPU_DECODE."""
import hashlib
import os
import sys

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_zstd_fixtures as zf                  # noqa: E402

import aggfly_amd as af                          # noqa: E402
from aggfly_amd import codec, io as afio         # noqa: E402

FIX = zf.load()
TAKEN = [(e, f, r) for e, f, r in FIX if e["taken"]]


def _plan(frames, sizes, strict=True, cap_blocks=4096):
    base, co, cs, oo, nout = zf.pack(frames, sizes)
    fr, bl = np.zeros(len(frames) + 1, dtype=codec.ZSTD_FRAME), np.zeros(cap_blocks, dtype=codec.ZSTD_BLOCK)
    p = codec.zstd_plan(base, co, cs, oo, sizes, fr, bl, strict=strict)
    return base, co, cs, oo, nout, fr, bl, p


def _check_records(base, co, cs, oo, nout, fr, bl, p, sizes):
    """Every record inside its chunk, the batch's literal / sequence buffers and the output."""
    fr, bl = fr[:p.n_frames], bl[:p.n_blocks]
    assert p.lit_bytes >= 0 and p.n_seqs >= 0 and p.dec_bytes == int(fr["size"].sum())
    assert p.lit_bytes + 3 * p.n_seqs <= p.dec_bytes
    chunk_of = {}
    for i in np.nonzero(p.results >= 0)[0]:
        chunk_of[len(chunk_of)] = int(i)
    base_pos, lit, nsq = 0, 0, 0
    for f, rec in enumerate(fr):
        i = chunk_of[f]
        assert rec["size"] == p.results[i] == sizes[i] and rec["dst_off"] == oo[i] and rec["base"] == base_pos
        assert rec["dst_off"] + rec["size"] <= nout
        base_pos += int(rec["size"])
        lo, hi = int(co[i]), int(co[i] + cs[i])
        for b in range(int(rec["first_block"]), int(rec["first_block"] + rec["n_blocks"])):
            k = bl[b]
            assert k["frame"] == f and lo <= k["src"] and k["src"] + k["csize"] <= hi
            assert k["lit_off"] == lit and k["seq_off"] == nsq
            lit += int(k["lit_size"]); nsq += int(k["nseq"])
            assert 0 <= k["lit_size"] <= 131072 and k["btype"] in (0, 1, 2)
            if k["btype"] == 2:
                assert 0 < k["lit_src"] <= k["csize"] and k["lit_src"] + k["lit_csize"] <= k["csize"]
                assert k["lit_type"] in (0, 1, 2, 3) and k["n_streams"] in (1, 4)
                if k["lit_type"] >= 2:
                    assert rec["first_block"] <= k["huf_block"] <= b and bl[k["huf_block"]]["lit_type"] == 2
                if k["nseq"]:
                    assert k["lit_src"] <= k["seq_src"] < k["csize"]
                    for t in range(3):
                        assert k["mode"][t] in (0, 1, 2)
                        if k["mode"][t] == 2:
                            tb = int(k["tab_block"][t])
                            assert rec["first_block"] <= tb <= b
                            assert 0 < bl[tb]["tab_desc"][t] < bl[tb]["csize"] and bl[tb]["mode"][t] == 2 and bl[tb]["tab_block"][t] == tb
    assert lit == p.lit_bytes and nsq == p.n_seqs


def test_fixtures_are_what_their_recipes_give_and_cover_every_mode():
    for e, _, raw in FIX:
        assert hashlib.sha256(raw).hexdigest() == e["raw_sha256"] and len(raw) == e["raw_bytes"]
    union = set(m for e, _, _ in FIX for m in e["modes"])
    assert zf.REQUIRED_MODES <= union, sorted(zf.REQUIRED_MODES - union)
    for lvl in (-5, 1, 3, 9, 19):
        assert any(e["level"] == lvl for e, _, _ in TAKEN)
    assert any(e["raw_bytes"] == 0 for e, _, _ in TAKEN) and any(0 < e["raw_bytes"] < 16 for e, _, _ in TAKEN)
    assert {e["why"] for e, _, _ in FIX if not e["taken"]} == {"checksum", "no content size", "two frames"}


def test_planner_on_every_fixture():
    frames, sizes = [f for _, f, _ in FIX], np.array([len(r) for _, _, r in FIX], dtype=np.int64)
    base, co, cs, oo, nout, fr, bl, p = _plan(frames, sizes)
    for (e, _, raw), r in zip(FIX, p.results):
        assert r == (len(raw) if e["taken"] else codec.E_UNSUPPORTED), e
    _check_records(base, co, cs, oo, nout, fr, bl, p, sizes)
    # records hold what the headers say: modes seen by the fixture generator's walk appear in the records
    multi = [e for e, _, _ in TAKEN if "frame:multi-block" in e["modes"]]
    assert p.n_blocks > len(TAKEN) and multi


def test_frame_with_a_different_content_size_is_not_taken():
    e, f, raw = TAKEN[0]
    *_, p = _plan([f], np.array([len(raw) + 4], dtype=np.int64))
    assert p.results[0] == codec.E_UNSUPPORTED and p.n_blocks == 0


@pytest.mark.parametrize("one_per_call", [False, True])
def test_gpu_passes_on_the_host_rebuild_every_frame_bit_exact(one_per_call):
    groups = [[x] for x in TAKEN] if one_per_call else [TAKEN]
    for g in groups:
        frames, raws = [f for _, f, _ in g], [r for _, _, r in g]
        sizes = np.array([len(r) for r in raws], dtype=np.int64)
        base, co, cs, oo, nout, fr, bl, p = _plan(frames, sizes)
        out = np.full(nout, 0xA5, dtype=np.uint8)
        errors, rounds = codec.zstd_emulate(base, fr, bl, p, out)
        assert errors == 0
        canary = np.ones(nout, dtype=bool)
        for (e, _, raw), o in zip(g, oo):
            assert out[o:o + len(raw)].tobytes() == raw, (e["recipe"], e["level"], e["n"])
            canary[o:o + len(raw)] = False
        assert (out[canary] == 0xA5).all()


def test_mutated_and_truncated_frames_never_escape():
    """10^4 damaged frames: the planner never crashes and never emits a record outside its buffers; a plan it accepts runs
    through the host emulation of the GPU passes without touching the canaries around the destination."""
    rng = np.random.default_rng(2024)
    small = [(e, f, r) for e, f, r in TAKEN if len(f) < 20000 and len(r) > 0]
    accepted = emulated = 0
    for it in range(10000):
        e, f, raw = small[int(rng.integers(len(small)))]
        b = bytearray(f)
        kind = it % 4
        if kind == 0:
            b = b[:int(rng.integers(1, len(b)))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                j = int(rng.integers(4, len(b))) if kind < 3 else int(rng.integers(4, min(len(b), 40)))
                b[j] = int(rng.integers(256)) if kind != 2 else b[j] ^ (1 << int(rng.integers(8)))
        sizes = np.array([len(raw)], dtype=np.int64)
        base, co, cs, oo, nout, fr, bl, p = _plan([bytes(b)], sizes, strict=False)
        assert p.results[0] < 0 or p.results[0] == len(raw)
        if p.results[0] < 0:
            assert p.n_blocks == 0 and p.n_frames == 0
            continue
        accepted += 1
        _check_records(base, co, cs, oo, nout, fr, bl, p, sizes)
        if it % 5 == 0:
            out = np.full(nout, 0x5A, dtype=np.uint8)
            errors, _ = codec.zstd_emulate(base, fr, bl, p, out)
            canary = np.ones(nout, dtype=bool)
            canary[oo[0]:oo[0] + len(raw)] = False
            assert (out[canary] == 0x5A).all()
            if errors == 0:
                emulated += 1
    assert accepted > 1000


def _store(tmp_path, name, fmt, chunks, shards=None, T=240, ny=6, nx=8, dtype=np.float32):
    from aggfly_amd import synth
    cube = synth.temperature_cube(T, ny, nx, dtype=dtype, seed=3)
    time = pd.date_range("2001-01-01", periods=T, freq="h")
    ds = af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                 {"time": time, "latitude": 30 + 0.5 * np.arange(ny), "longitude": 200 + 0.5 * np.arange(nx)}))
    path = str(tmp_path / name)
    af.dataset_to_zarr(ds, path, var="t2m", chunks=chunks, shards=shards, compress="zstd", zarr_format=fmt)
    return afio.ZarrArray(os.path.join(path, "t2m"))


def test_route_choice_for_zstd_stores(tmp_path, monkeypatch):
    stores = [_store(tmp_path, "v2.zarr", 2, {"time": 48, "latitude": 6, "longitude": 8}),
              _store(tmp_path, "v3.zarr", 3, {"time": 240, "latitude": 3, "longitude": 4}),
              _store(tmp_path, "v3s.zarr", 3, {"time": 24, "latitude": 6, "longitude": 8}, shards={"time": 120, "latitude": 6, "longitude": 8})]
    for za in stores:
        assert za.native_kind == "zstd"
        for mode, nbytes, want in (("0", 1 << 40, False), ("1", 1, True), ("auto", afio.GPU_DECODE_AUTO_BYTES_ZSTD - 1, False),
                                   ("auto", afio.GPU_DECODE_AUTO_BYTES_ZSTD, True)):
            monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
            for attr in ("_gpu_decodable",):
                if hasattr(za, attr):
                    delattr(za, attr)
            assert afio._gpu_decodable(za, nbytes) is want, (za.path, mode, nbytes)
    # the small stores of the existing tests stay on the host route under auto
    assert afio.GPU_DECODE_AUTO_BYTES_ZSTD >= 64 << 20
    # a store whose first chunk carries a checksum is judged not decodable
    za = stores[0]
    first = za.chunk_locator((0, 0, 0))[0]
    h = bytearray(open(first, "rb").read(18))
    assert afio._zstd_frame_taken(bytes(h), za.chunk_nbytes)
    h[4] |= 0x04
    assert not afio._zstd_frame_taken(bytes(h), za.chunk_nbytes)
    assert not afio._zstd_frame_taken(bytes(h[:4]) + b"\x00" * 14, za.chunk_nbytes)
