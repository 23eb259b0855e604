"""The hand-built LZ4 streams of tests/lz4_streams.py on the host, no GPU: every catalogue and fuzz stream decodes — by the
module's own strict decoder and by the real liblz4 (`codec.lz4_decode`) — to what its sequence list means; every damaged one
is refused; the census (a restatement of `k_lz4_streams_vec`'s parse decisions) shows that the cases reach the kernel paths
they are named after; and streams wrapped into Blosc-1 chunks come back through the host route and the planner as they went in.

liblz4 1.9.3's LZ4_decompress_safe does not check for a match offset of 0 (it copies the destination onto itself and reports
the recorded size): the host route finds it with a walk over the sequence headers first (`lz4_has_zero_offset` in blosc1.c), so
that all 22 damaged streams are refused by the strict decoder, the host route and the GPU kernel alike."""
import os
import struct
import sys
from collections import Counter

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lz4_streams as lz                        # noqa: E402

from aggfly_amd import codec                    # noqa: E402

FUZZ_SEED, FUZZ_N = 2024, 400


@pytest.fixture(scope="module")
def catalogue():
    return lz.catalogue()


@pytest.fixture(scope="module")
def fuzzed():
    return lz.fuzz(FUZZ_SEED, FUZZ_N)


def _liblz4(stream, dsize):
    return codec.lz4_decode(struct.pack("<i", dsize) + stream, dsize).tobytes()


def _check_positive(cases):
    for name, seqs, tail in cases:
        assert lz.conformant(seqs, tail), name
        stream, want = lz.build(seqs, tail), lz.expand(seqs, tail)
        assert len(stream) != len(want), name                       # (csize == dsize reads as "stored")
        assert lz.decode(stream, len(want)) == want, name
        assert _liblz4(stream, len(want)) == want, name


def test_catalogue_streams_decode_to_their_sequence_lists(catalogue):
    assert len(catalogue) > 200
    _check_positive(catalogue)
    sizes = [len(lz.expand(q, t)) for _, q, t in catalogue]
    assert max(sizes) < 200_000 and sum(sizes) < 4 << 20


def test_fuzz_streams_decode_to_their_sequence_lists(fuzzed):
    assert len(fuzzed) == FUZZ_N and all(len(q) <= 60 for _, q, _ in fuzzed)
    _check_positive(fuzzed)
    assert sum(len(lz.expand(q, t)) for _, q, t in fuzzed) <= lz.FUZZ_MAX_BYTES
    assert [lz.build(q, t) for _, q, t in lz.fuzz(FUZZ_SEED, 5)] == [lz.build(q, t) for _, q, t in fuzzed[:5]]     # the seed decides


def test_the_end_rule_is_liblz4s():
    """Streams that break only the end-of-block rule — a tail of 0 or 4 literals, a 4-byte last match before a 5-byte tail — are
    what `conformant` says liblz4 refuses (they are in no list that runs on the GPU)."""
    rng = np.random.default_rng(1)
    head = (rng.bytes(8), 8, 8)
    for seqs, tail in (([head], b""), ([head], rng.bytes(4)), ([head, (rng.bytes(2), 3, 4)], rng.bytes(5))):
        assert not lz.conformant(seqs, tail)
        want = lz.expand(seqs, tail)
        with pytest.raises(codec.CodecError):
            _liblz4(lz.build(seqs, tail), len(want))
    seqs, tail = [head, (rng.bytes(2), 3, 7)], rng.bytes(5)
    assert lz.conformant(seqs, tail) and _liblz4(lz.build(seqs, tail), 30) == lz.expand(seqs, tail)


DAMAGED = lz.damaged()


def test_damaged_streams_cover_the_list():
    names = [d[0] for d in DAMAGED]
    assert len(set(names)) == len(names) == 22


@pytest.mark.parametrize("name,stream,dsize", DAMAGED, ids=[d[0] for d in DAMAGED])
def test_strict_decoder_refuses_the_damaged_stream(name, stream, dsize):
    with pytest.raises(lz.StreamError):
        lz.decode(stream, dsize)


@pytest.mark.parametrize("name,stream,dsize", DAMAGED, ids=[d[0] for d in DAMAGED])
def test_liblz4_refuses_the_damaged_stream(name, stream, dsize):
    """The host route's decoder: `afcodec_lz4_decode` -> `lz4_has_zero_offset`, LZ4_decompress_safe."""
    codec.load()                                                     # (a missing library raises CodecError too: not what is meant)
    with pytest.raises(codec.CodecError, match="failed to decode to its recorded size"):
        _liblz4(stream, dsize)


@pytest.mark.parametrize("literals", [2, 70], ids=["window", "generic"])
@pytest.mark.parametrize("shuffle", [True, False], ids=["shuffled", "plain"])
def test_blosc_host_route_refuses_an_offset_zero_plane(literals, shuffle):
    """The same defect inside a Blosc-1 chunk (`decode_stream` in blosc1.c): a chunk whose second plane holds a match of offset 0
    is refused by `codec.blosc_decode`, and decodes once that offset is 3."""
    plane = 256
    rng = np.random.default_rng(78)
    head, tail = (rng.bytes(8), 8, 8), rng.bytes(plane - 16 - (literals + 6) - 6)
    first = lz.padded([head, (rng.bytes(2), 3, 6)], rng.bytes(12), plane, seed=1)
    lits = rng.bytes(literals)
    streams = {off: [lz.build(*first), lz.build([head, (lits, off, 6), (b"ab", 3, 4)], tail)] for off in (0, 3)}
    assert len(streams[0][1]) == len(streams[3][1]) != plane
    with pytest.raises(lz.StreamError, match="offset 0"):
        lz.decode(streams[0][1], plane)
    good, _ = lz.blosc_wrap(streams[3], 2, shuffle, 2 * plane)
    planes = [lz.decode(s, plane) for s in streams[3]]
    assert codec.blosc_decode(good).tobytes() == (lz.weave(planes, 2) if shuffle else b"".join(planes))
    bad, _ = lz.blosc_wrap(streams[0], 2, shuffle, 2 * plane)
    with pytest.raises(codec.CodecError, match="block failed to decompress to its recorded size"):
        codec.blosc_decode(bad, out=np.full(2 * plane, 0xAB, dtype=np.uint8))


def _census(cases):
    total, per_case = Counter(), {}
    for name, seqs, tail in cases:
        c = lz.census(lz.build(seqs, tail), len(lz.expand(seqs, tail)))
        per_case[name] = c
        total.update(c)
    return total, per_case


def test_census_of_the_catalogue_reaches_every_class(catalogue):
    """Printed with -s: how often the catalogue takes each path of the kernel."""
    total, per = _census(catalogue)
    for k in lz.CLASSES + ("windows", "fast_sequences", "generic_sequences", "line_shift_twice"):
        print(f"{k:32s} {total[k]}")
    print("window_tokens", [total[f"window_tokens={k}"] for k in range(1, 22)])
    assert [k for k in lz.CLASSES if total[k] == 0] == []
    assert [k for k in range(1, 22) if total[f"window_tokens={k}"] == 0] == []
    assert not any(total[f"window_tokens={k}"] for k in range(22, 65))                # three bytes a sequence: 21 fit
    # the cases reach the paths they are named after
    for k in range(1, 22):
        assert per[f"pack_{k}"][f"window_tokens={k}"] == 3, k
    assert per["pack_21x3"]["window_tokens=21"] == 4
    assert per["pack_16x273"]["window_tokens=16"] == 2 and per["pack_16x273"]["rounds>1"] == 2
    assert per["edge_nx64"]["window_tokens=21"] == 2 and per["edge_nx65"]["window_tokens=20"] >= 1 and not per["edge_nx65"]["window_tokens=21"]
    for L in (15 + 255 * 64, 16 + 255 * 64):
        assert per[f"lit_{L}"]["generic_ext_scan_two_passes"] == 1
    for M in (19 + 255 * 64, 20 + 255 * 64, 70_000):
        assert per[f"match_{M}"]["generic_ext_scan_two_passes"] == 1
    assert per["match_273"]["generic_sequences"] == 1 and per["match_274"]["generic_sequences"] == 3     # (254 | 255, 0; + the final one)
    assert per["lit_269"]["literal_copy_from_stream"] and per["lit_14"]["generic_sequences"] == 1
    for k in range(64):                                              # the read position at every residue of a 64-byte line
        seqs = [q for n, q, _ in catalogue if n == f"residue_{k}"][0]
        assert len(lz.build(seqs[:1], None)) % 64 == k and per[f"residue_{k}"][f"window_residue={k}"] >= 1, k
        assert per[f"residue_{k}"]["generic_near_short_period"] >= 1 and per[f"residue_{k}"]["windows"] >= 5
    assert per["run_128"]["line_shift_twice"] and per["run_192"]["literal_jump_3_lines"] and per["run_1000"]["literal_jump_3_lines"]
    for off in (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 63):
        assert per[f"off_{off}_generic"]["generic_near_short_period"] == 3 and per[f"off_{off}_fast"]["fast_overlap"] >= 3
    assert per["off_64_generic"]["generic_near"] == 4 and per["off_sweep_273"]["fast_overlap"] == 272
    for off in (4, 1):
        assert per[f"chain_{off}_4"]["fast_same_round_source"] >= 80
    for off in (4031, 4032):
        assert not per[f"far_{off}_fast"]["fast_far"] and per[f"far_{off}_generic_M274"]["generic_near"] >= 2
    for off in (4033, 4095, 4096, 4097, 8192, 65535):
        assert per[f"far_{off}_fast"]["fast_far"] >= 10, off
        assert per[f"far_{off}_generic_M274"]["generic_far_plain"] >= 3
        assert per[f"far_{off}_generic_M{off + 1}"]["generic_far_overlap"] == 1 and per[f"far_{off}_generic_M{2 * off + 17}"]["generic_far_overlap"] == 1
    assert per["far_8192_generic_M20000"]["generic_far_overlap"] == 1 and per["far_65535_generic_M20000"]["generic_far_plain"] == 2
    assert per["far_unacked_after_fast_rounds"]["fast_far_unacked"] == 3 and per["far_unacked_after_fast_rounds"]["fast_far"] >= 6
    assert per["far_long_stored"]["fast_far_unacked"] == 0 and per["far_long_stored"]["fast_far"] >= 8
    assert per["far_residues"]["fast_far"] >= 2 and per["far_residues"]["generic_far_plain"] == 17
    assert per["ring_wrap_match"]["ring_wrap_inside_match"] >= 2
    for t in (5, 12, 14, 15, 16, 59, 60, 61, 62):
        assert per[f"tail_{t}"]["final_in_window"] == 1 or t >= 15, t
    assert per["tail_14"]["final_in_window"] == 1 and per["tail_15"]["final_generic"] == 1 and per["tail_300"]["final_generic"] == 1
    assert per["litonly_14"]["final_in_window"] == 1 and per["litonly_300"]["final_generic"] == 1


def test_census_of_the_fuzz_reaches_both_paths_and_the_far_ones(fuzzed):
    """Measured for seed 2024, n = 400: fast_sequences 8,995, generic_sequences 3,492, fast_far 3,141, generic_far_overlap 67."""
    total, _ = _census(fuzzed)
    print({k: total[k] for k in ("fast_sequences", "generic_sequences", "fast_far", "generic_far_overlap")})
    assert total["fast_sequences"] >= 4000 and total["generic_sequences"] >= 1500
    assert total["fast_far"] >= 1000 and total["generic_far_overlap"] >= 30


def test_wrapped_streams_come_back_through_the_host_route_and_the_planner():
    chunks = lz.wrapped_chunks()
    assert [(c[0], c[1]) for c in chunks] == list(lz.WRAP_SHAPES)
    for ts, shuffle, chunk, recs, want in chunks:
        info = codec.blosc_info(chunk)
        assert info["codec"] == "lz4" and info["split"] and info["typesize"] == ts and info["shuffle"] == int(shuffle)
        assert info["nbytes"] == len(want) == 2 * ts * lz.WRAP_PLANE
        assert codec.blosc_decode(chunk).tobytes() == want, (ts, shuffle)
        base = np.zeros(64 + len(chunk), dtype=np.uint8)
        base[64:] = np.frombuffer(chunk, dtype=np.uint8)
        streams, blocks = np.zeros(64, dtype=codec.LZ4_STREAM), np.zeros(8, dtype=codec.SHUFFLE_BLOCK)
        ns, nb, tmpb, maxd, res = codec.blosc_lz4_plan(base, [64], [len(chunk)], [128], [len(want)], streams, blocks)
        assert ns == len(recs) == 2 * ts and res[0] == len(want) and maxd == lz.WRAP_PLANE and nb == (2 if shuffle else 0)
        for j, (s, (off, csize, dsize)) in enumerate(zip(streams[:ns], recs)):
            assert (s["src_off"], s["csize"], s["dsize"], s["to_out"]) == (64 + off, csize, dsize, 0 if shuffle else 1), (ts, shuffle, j)
            assert s["dst_off"] == (0 if shuffle else 128) + j * lz.WRAP_PLANE


def test_layout_places_every_record_between_guards(catalogue):
    """The launch layout the GPU tests use, replayed on the host: every record decoded by `lz.decode` into buffers of 0xAB gives the
    expected image; sources and destinations are apart, inside their buffers, at residues 0 .. 15 mod 16."""
    items = [(lz.build(q, t), len(lz.expand(q, t)), lz.expand(q, t)) for _, q, t in catalogue[:40]]
    name, stream, dsize = DAMAGED[0]
    items.insert(3, (stream, dsize, None))
    stored = [(bytes(range(17)), True, True), (bytes(range(33)), False, True), (bytes(range(16)), True, False)]
    comp, recs, image, mask = lz.layout(items, stored)
    assert recs.dtype == codec.LZ4_STREAM and len(recs) == len(items) + 3
    buf = {k: np.full(len(image[k]), 0xAB, dtype=np.uint8) for k in (0, 1)}
    spans = {0: [], 1: []}
    for r in recs:
        src = comp[r["src_off"]:r["src_off"] + r["csize"]].tobytes()
        assert len(src) == r["csize"] and r["dst_off"] >= lz.GUARD and r["dst_off"] + r["dsize"] + lz.GUARD <= len(buf[int(r["to_out"])])
        spans[int(r["to_out"])].append((int(r["dst_off"]), int(r["dst_off"] + r["dsize"])))
        if r["csize"] == r["dsize"]:
            dec = src
        else:
            try:
                dec = lz.decode(src, int(r["dsize"]))
            except lz.StreamError:
                assert not mask[int(r["to_out"])][r["dst_off"]:r["dst_off"] + r["dsize"]].any()
                continue
        buf[int(r["to_out"])][r["dst_off"]:r["dst_off"] + r["dsize"]] = np.frombuffer(dec, dtype=np.uint8)
    for k in (0, 1):
        assert (buf[k] == image[k])[mask[k]].all() and (~mask[k]).sum() == (dsize if k == 1 else 0)
        ordered = sorted(spans[k])
        assert all(b[0] - a[1] >= lz.GUARD for a, b in zip(ordered, ordered[1:]))
    assert set(recs["src_off"][:len(items)] % 16) == set(range(16)) == set(recs["dst_off"][:len(items)] % 16) and [int(x) for x in recs["src_off"][-3:] % 16] == [0, 5, 0]
    assert [int(x) for x in recs["dst_off"][-3:] % 16] == [0, 0, 9]
