"""The Zstandard block encoder of aggfly_amd/csrc/zstd_encode_pass.h as the host runs it (`afcodec_zstd_encode_block_emulate`: the
kernel's text, its 64 lanes in loops) over the catalogue of tests/zstd_encode_cases.py: every block, behind a frame header, means its
input to libzstd and to the strict RFC 8878 decoder of tests/zstd_frames.py, keeps the limits the encoder promises, and is taken by
the planner and the passes of the decode-in-HBM route; `codec.BloscZstdEncodePlan` assembles containers that `codec.blosc_decode`
reads and whose headers are the host encoder's; and the host route of `dataset_to_zarr` writes what the commit before wrote.

The issue behind this encoder also asks the census for RLE literals.  They cannot arise: the first occurrence of every byte value in
a block is a literal, so literals of one value mean a block of one value, which is an RLE block — `test_rle_literals_cannot_arise`
holds the catalogue to that argument instead."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import zstd_encode_cases as zc                  # noqa: E402
import zstd_frames as zf                        # noqa: E402

import aggfly_amd as af                         # noqa: E402
from aggfly_amd import codec                    # noqa: E402


@pytest.fixture(scope="module")
def encoded():
    """[(name, input, expectation, block, census, records)] once for the module: the emulation's block and the strict decoder's view."""
    out = []
    for name, data, expect in zc.catalogue():
        block = codec.zstd_encode_block_emulate(data)
        census, records = set(), []
        back = zf.decode(codec.zstd_frame_header(len(data)) + block, census, records)
        assert back == data, name
        out.append((name, data, expect, block, census, records))
    return out


def test_the_catalogue_holds_what_the_issue_names():
    names = [n for n, _, _ in zc.catalogue()]
    assert len(names) == len(set(names)) and sum(n.startswith("mix_") for n in names) == 100
    for n in (1, 2, 3, 4, 7, 8, 63, 64, 65, 255, 256, 257, 131071, 131072):
        assert f"len_{n}_run" in names and f"len_{n}_noise" in names
    assert all(len(d) % 64 for n, d, _ in zc.catalogue() if n.startswith("mix_"))
    assert all(1 <= len(d) <= zc.BLOCK for _, d, _ in zc.catalogue())


def test_every_block_decodes_with_libzstd(encoded):
    for name, data, _, block, _, _ in encoded:
        assert codec.zstd_decode(codec.zstd_frame_header(len(data)) + block, len(data)).tobytes() == data, name


def test_block_limits(encoded):
    """At most n + 3 bytes; codes of at most 11 bits; predefined sequence codes, no repeat code, never treeless; the last-block bit is the
    caller's.  (An offset beyond its position is refused by the strict decoder, which decoded every block in the fixture.)"""
    for name, data, _, block, census, records in encoded:
        assert len(block) <= len(data) + 3, name
        assert len(records) == 1 and block[0] & 1 == 1, name
        assert all(c[1] <= 11 for c in census if c[0] == "huf_depth"), name
        assert not [c for c in census if c[0] == "rep"], name
        assert all(c[2] == "pre" for c in census if c[0] == "mode"), name
        assert not [c for c in census if c[0] == "lit" and c[1] == "treeless"], name
        assert codec.zstd_encode_block_emulate(data, last=False)[0] & 1 == 0
    name, data, _, block, _, _ = encoded[-1]
    assert codec.zstd_encode_block_emulate(data, last=False)[1:] == block[1:]


def test_expectations_of_the_named_cases(encoded):
    for name, data, expect, block, census, records in encoded:
        if "block" in expect:
            assert ("block", expect["block"]) in census, (name, census)
        if expect.get("block") == "raw":
            assert len(block) == len(data) + 3, name
        if expect.get("shorter"):
            assert len(block) < len(data), (name, len(block))
        for entry in expect.get("census", ()):
            assert tuple(entry) in census, (name, entry, sorted(census, key=str))
        if "nseq" in expect:
            assert records[0]["nseq"] == expect["nseq"], (name, records)
        if "lit_size" in expect:
            assert records[0]["lit_size"] == expect["lit_size"], (name, records)


def test_census_over_the_catalogue(encoded):
    census = set().union(*[c for *_, c, _ in encoded])
    for want in [("lit", "raw", 1), ("lit", "huf", 1), ("lit", "huf", 4), ("block", "raw"), ("block", "rle"), ("block", "comp"),
                 ("huf_desc", "fse", 6), ("nseq_form", 0), ("nseq_form", 1), ("nseq_form", 2), ("mode", "LL", "pre"), ("mode", "OF", "pre"),
                 ("mode", "ML", "pre"), ("lit_hdr", "coded", 3), ("lit_hdr", "coded", 4), ("lit_hdr", "coded", 5), ("lit_hdr", "plain", 1),
                 ("lit_hdr", "plain", 2), ("lit_hdr", "plain", 3), ("code", "LL", 35), ("code", "ML", 52), ("code", "OF", 16), ("huf_depth", 11)]:
        assert want in census, want
    assert {c[2] for c in census if c[:2] == ("huf_desc", "direct")} == {"odd", "even"}
    assert max(r[0]["nseq"] for *_, r in encoded) == 16384                      # (the cap on sequences: the rest became literals)


def test_rle_literals_cannot_arise(encoded):
    """No compressed block of the catalogue has literals of one byte value, and the encoder has no line for them (see the module's text)."""
    assert ("lit", "rle", 1) not in set().union(*[c for *_, c, _ in encoded])
    for name, data, _, block, census, _ in encoded:
        if ("block", "comp") in census:
            assert len(set(data)) > 1, name
        if len(set(data)) == 1:
            assert ("block", "rle") in census and len(block) == 4, name


def test_the_decode_route_takes_every_frame(encoded):
    """`codec.zstd_plan(strict=True)` accepts every frame and `codec.zstd_emulate` (the passes of the decode-in-HBM route) rebuilds it."""
    frames = [codec.zstd_frame_header(len(d)) + b for _, d, _, b, _, _ in encoded]
    sizes = np.array([len(d) for _, d, *_ in encoded], dtype=np.int64)
    cs = np.array([len(f) for f in frames], dtype=np.int64)
    co, oo = np.cumsum(cs) - cs, np.cumsum(sizes) - sizes
    base = np.frombuffer(b"".join(frames), dtype=np.uint8).copy()
    fr, bl = np.zeros(len(frames) + 1, dtype=codec.ZSTD_FRAME), np.zeros(len(frames) + 8, dtype=codec.ZSTD_BLOCK)
    p = codec.zstd_plan(base, co, cs, oo, sizes, fr, bl, strict=True)
    assert (p.results == sizes).all()
    out = np.zeros(int(sizes.sum()), dtype=np.uint8)
    errors, _ = codec.zstd_emulate(base, fr, bl, p, out)
    assert errors == 0 and out.tobytes() == b"".join(d for _, d, *_ in encoded)


# ---- containers -------------------------------------------------------------------------------------------------------------------
def _field(nbytes, seed):
    rng = np.random.default_rng(seed)
    m = nbytes // 4 + 1
    return (280 + 10 * np.sin(np.arange(m) * 0.01) + rng.normal(0, 0.5, m)).astype("<f4").tobytes()[:nbytes]


def _containers(n, nbytes, typesize, data):
    """The containers of n chunks of ``data`` assembled by the plan from emulated blocks: what the GPU route does, on the host."""
    pl = codec.BloscZstdEncodePlan(n, nbytes, typesize)
    work = np.zeros(pl.work_bytes, dtype=np.uint8)
    src = np.frombuffer(data, dtype=np.uint8)
    for b in pl.blocks:
        blk = src[b["out_off"]:b["out_off"] + b["bsize"]].tobytes()
        work[b["tmp_off"]:b["tmp_off"] + b["bsize"]] = np.frombuffer(zc.shuffle(blk, int(b["typesize"])), dtype=np.uint8)
    cs = np.zeros(len(pl.streams), dtype=np.int64)
    for i, s in enumerate(pl.streams):
        blk = codec.zstd_encode_block_emulate(work[s["src_off"]:s["src_off"] + s["n"]], bool(s["last"]))
        cs[i] = len(blk)
        assert len(blk) <= s["n"] + 3
        work[pl.slot_base + s["dst_off"]:pl.slot_base + s["dst_off"] + len(blk)] = np.frombuffer(blk, dtype=np.uint8)
    return pl, pl.assemble_host(work, cs)


@pytest.mark.parametrize("nbytes,typesize", [(100, 4), (127, 4), (128, 4), (262143, 4), (262144, 4), (262148, 4), (3 * 262144 + 20, 4),
                                             (300000, 2), (300000, 8)])
def test_containers_decode_and_carry_the_host_encoders_headers(nbytes, typesize):
    n = 2
    data = _field(n * nbytes, nbytes)
    pl, conts = _containers(n, nbytes, typesize, data)
    for i, c in enumerate(conts):
        raw = data[i * nbytes:(i + 1) * nbytes]
        assert codec.blosc_decode(c).tobytes() == raw
        host = codec.blosc_encode(raw, typesize, cname="zstd")
        gi, hi = codec.blosc_info(c), codec.blosc_info(host)
        assert (c[2], c[3], c[4:12]) == (host[2], host[3], host[4:12])               # flags, typesize, nbytes, blocksize
        assert (gi["nbytes"], gi["blocksize"]) == (hi["nbytes"], hi["blocksize"]) == (nbytes, pl.blocksize)
        first = lambda b: int.from_bytes(b[16:20], "little") if nbytes >= 128 else 16
        assert first(c) == first(host) == 16 + 4 * pl.n_bstarts                      # the same number of bstarts
        assert int.from_bytes(c[12:16], "little") == len(c)
        if nbytes >= 262144:
            assert len(c) < nbytes                                                   # (the field compresses)


def test_a_frame_is_cut_at_the_byte_planes():
    pl = codec.BloscZstdEncodePlan(1, 262144 + 40, 4)
    assert [int(s["n"]) for s in pl.streams] == [65536] * 4 + [10] * 4 and [int(s["last"]) for s in pl.streams] == [0, 0, 0, 1] * 2
    assert [int(s["n"]) for s in codec.BloscZstdEncodePlan(1, 262144, 2).streams] == [131072] * 2
    assert [int(s["n"]) for s in codec.BloscZstdEncodePlan(1, 262144 + 5, 1).streams] == [131072] * 2 + [5]
    assert [int(s["n"]) for s in codec.BloscZstdEncodePlan(1, 262143, 4).streams] == [65535] * 4 + [3]
    st = codec.BloscZstdEncodePlan(3, 300000, 8).streams
    assert (np.diff(st["dst_off"]) == st["n"][:-1] + 3).all() and (st["scratch_off"] % 256 == 0).all() and st["scratch_off"][0] > 0


def test_incompressible_containers_are_stored_frames_of_the_host_encoders_size():
    nbytes = 262144 + 4000
    data = np.random.default_rng(5).integers(0, 256, 2 * nbytes, dtype=np.uint8).tobytes()
    pl, conts = _containers(2, nbytes, 4, data)
    for i, c in enumerate(conts):
        raw = data[i * nbytes:(i + 1) * nbytes]
        assert codec.blosc_decode(c).tobytes() == raw
        assert len(c) == len(codec.blosc_encode(raw, 4, cname="zstd")) == 16 + 2 * 4 + 2 * 4 + nbytes
        assert int.from_bytes(c[24:28], "little") == 262144                          # the first frame's length: its block's size = stored


# ---- the host route is the parent commit's ----------------------------------------------------------------------------------------
def test_the_host_route_writes_what_the_parent_commit_wrote(tmp_path):
    gold = json.load(open(os.path.join(HERE, "golden", "zstd_encode_parent.json")))
    assert [{k: s[k] for k in ("compress", "zarr_format", "shards")} for s in gold["stores"]] == zc.HOST_ROUTE_STORES
    for i, s in enumerate(gold["stores"]):
        p = str(tmp_path / f"s{i}.zarr")
        af.dataset_to_zarr(zc.small_dataset(), p, chunks=zc.SMALL_CHUNKS, compress=s["compress"], zarr_format=s["zarr_format"],
                           shards=s["shards"], encode="host")
        assert zc.tree_hashes(p) == s["files"], (s["compress"], s["zarr_format"], s["shards"])
