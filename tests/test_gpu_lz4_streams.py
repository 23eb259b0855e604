"""`k_lz4_streams_vec` and `k_unshuffle_blocks` (aggfly_amd/csrc/afhip_lz4_kernels.h) held to hand-built input: the catalogue,
the sequence-level fuzz and the damaged streams of tests/lz4_streams.py through `hip.lz4_decode_streams` as bare records —
every destination between 64-byte guards in buffers filled with 0xAB, both whole buffers compared with an expected image —,
catalogue streams wrapped into Blosc-1 chunks through the planner, and the byte unshuffle alone against numpy at every size and
alignment where it takes another path.  tests/test_lz4_streams.py shows on the host which kernel path every case reaches."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lz4_streams as lz                        # noqa: E402

from aggfly_amd import codec                    # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = lz.GUARD
FUZZ_SEED, FUZZ_N, FUZZ_LAUNCHES = 2024, 400, 4  # (the seed tests/test_lz4_streams.py takes its census of)


def _launch(torch, comp, recs, image):
    """One `hip.lz4_decode_streams` call -> ({0: tmp, 1: out} on the host, error count)."""
    from aggfly_amd import hip
    assert recs.dtype == codec.LZ4_STREAM
    dev = {k: torch.full((len(image[k]),), 0xAB, dtype=torch.uint8, device="cuda") for k in (0, 1)}
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.lz4_decode_streams(torch.from_numpy(comp).cuda(), torch.from_numpy(recs.view(np.uint8).copy()).cuda(), len(recs),
                           int(recs["dsize"].max()), dev[0], dev[1], errors)
    torch.cuda.synchronize()
    return {k: dev[k].cpu().numpy() for k in (0, 1)}, int(errors.item())


def _first_difference(names, recs, got, image, mask=None):
    """None, or (buffer, position, name of the record whose destination or guards hold it, got, expected)."""
    for k in (0, 1):
        ne = got[k] != image[k]
        if mask is not None:
            ne &= mask[k]
        bad = np.nonzero(ne)[0]
        if bad.size:
            at = int(bad[0])
            who = [n for n, r in zip(names, recs) if r["to_out"] == k and r["dst_off"] - GUARD <= at < r["dst_off"] + r["dsize"] + GUARD]
            return ("out" if k else "tmp", at, who[:2], int(got[k][at]), int(image[k][at]), int(bad.size))
    return None


def _positive(cases):
    items, names = [], []
    for name, seqs, tail in cases:
        want = lz.expand(seqs, tail)
        stream = lz.build(seqs, tail)
        assert lz.conformant(seqs, tail) and len(stream) != len(want), name
        items.append((stream, len(want), want))
        names.append(name)
    return items, names


def test_catalogue_streams_decode_bit_exact(torch_cuda):
    """The whole catalogue and the stored records in one launch, src_off / dst_off at the residues 0 .. 15 mod 16, to_out 0 and 1;
    then the same records in reverse order: nothing may depend on which workgroup gets which stream."""
    items, names = _positive(lz.catalogue())
    rng = np.random.default_rng(9)
    stored = [(rng.bytes(n), sa, da) for n in lz.STORED_SIZES for sa, da in ((True, True), (False, True), (True, False))]
    names += [f"stored_{len(b)}_{'a' if sa else 'u'}{'a' if da else 'u'}" for b, sa, da in stored]
    comp, recs, image, _ = lz.layout(items, stored)
    assert {int(r) for r in recs["src_off"][:len(items)] % 16} == set(range(16)) == {int(r) for r in recs["dst_off"][:len(items)] % 16}
    assert set(recs["to_out"]) == {0, 1} and ((recs["csize"] == recs["dsize"]).sum() == len(stored))
    for order in (slice(None), slice(None, None, -1)):
        got, nerr = _launch(torch_cuda, comp, recs[order].copy(), image)
        assert nerr == 0
        assert _first_difference(names, recs, got, image) is None


def test_sequence_fuzz(torch_cuda):
    cases = lz.fuzz(FUZZ_SEED, FUZZ_N)
    assert len(cases) == FUZZ_N
    step = -(-len(cases) // FUZZ_LAUNCHES)
    for at in range(0, len(cases), step):
        items, names = _positive(cases[at:at + step])
        comp, recs, image, _ = lz.layout(items)
        got, nerr = _launch(torch_cuda, comp, recs, image)
        assert nerr == 0
        assert _first_difference(names, recs, got, image) is None


def test_damaged_streams_count_once_and_stay_inside(torch_cuda):
    """Every damaged stream of `lz4_streams.damaged` (the line of the kernel that refuses each is named beside it there) between
    two good ones, one launch: as many errors as damaged streams, the neighbours bit-exact, every byte outside the damaged
    streams' own destinations as it was."""
    good, good_names = _positive([c for c in lz.catalogue() if c[0] in ("pack_21x3", "chain_4_4", "off_7_fast", "lit_16", "far_4097_fast")])
    damaged = lz.damaged()
    items, names = [good[0]], [good_names[0]]
    for j, (name, stream, dsize) in enumerate(damaged):
        items += [(stream, dsize, None), good[(j + 1) % len(good)]]
        names += [name, good_names[(j + 1) % len(good)]]
    comp, recs, image, mask = lz.layout(items)
    got, nerr = _launch(torch_cuda, comp, recs, image)
    assert _first_difference(names, recs, got, image, mask) is None
    assert nerr == len(damaged)


def test_wrapped_streams_through_the_planner(torch_cuda):
    """Catalogue streams as the byte planes of Blosc-1 chunks (typesize 2, 4 and 8; shuffled and not): planner, LZ4 kernel and
    unshuffle give what the host route gives."""
    from test_gpu_decode import _gpu_decode
    chunks = lz.wrapped_chunks()
    assert {c[0] for c in chunks} == {2, 4, 8} and {c[1] for c in chunks} == {True, False}
    want = [codec.blosc_decode(c[2]).tobytes() for c in chunks]
    assert want == [c[4] for c in chunks]
    got, nerr, host, out_off = _gpu_decode(torch_cuda, [c[2] for c in chunks], [len(w) for w in want])
    assert nerr == 0
    for c, g, w in zip(chunks, got, want):
        assert g is not None and g.tobytes() == w, c[:2]


TILE_EDGE = 64 * 256                                                 # k_unshuffle_blocks: at most 64 tiles of 256 threads, then the grid-stride loop


@pytest.mark.parametrize("ts", [1, 2, 3, 4, 8, 16])
def test_unshuffle_kernel_against_the_numpy_reference(torch_cuda, ts):
    """`afhip_unshuffle_blocks` alone, many blocks of different sizes in one call (`max_bsize` from the largest: small blocks see idle
    tiles): element counts around a tile and around the 64 tiles where the grid-stride loop starts, trailing bytes, destinations at
    the residues 0, 8, 4, 2 and 1 mod 16 (the qword, dword and byte-wise stores of the ts = 8 and ts = 4 branches), sources
    unaligned, guards all round, the whole buffer compared."""
    from aggfly_amd import hip
    rng = np.random.default_rng(200 + ts)
    shapes = [(n, 0) for n in (1, 255, 256, 257, TILE_EDGE - 1, TILE_EDGE, TILE_EDGE + 1, 40_000)]           # (elements, trailing bytes)
    if ts > 1:
        shapes += [(257, 1), (257, ts - 1), (TILE_EDGE + 1, ts - 1), (1, 1)]
    blocks, tmp_parts, tmp_at, out_at, want = [], [], 0, GUARD, []
    for res in (0, 8, 4, 2, 1):
        for n, extra in shapes:
            bsize = n * ts + extra
            out_at = (out_at + 15) // 16 * 16 + res
            pad = 1 + (len(blocks) * 5) % 7                        # sources at odd places
            tmp_parts.append(np.zeros(pad, dtype=np.uint8))
            tmp_at += pad
            src = rng.integers(0, 256, bsize, dtype=np.uint8)
            ref = src.copy()
            ref[:n * ts] = src[:n * ts].reshape(ts, n).T.reshape(-1)
            blocks.append((tmp_at, out_at, bsize, ts))
            want.append((out_at, ref))
            tmp_parts.append(src)
            tmp_at += bsize
            out_at += bsize + GUARD
    rec = np.array(blocks, dtype=codec.SHUFFLE_BLOCK)
    assert {int(r) for r in rec["out_off"] % 16} == {0, 8, 4, 2, 1} and (rec["tmp_off"] % 4 != 0).any()
    expect = np.full(out_at + 16, 0xAB, dtype=np.uint8)
    for o, w in want:
        expect[o:o + len(w)] = w
    tmp = torch_cuda.from_numpy(np.concatenate(tmp_parts + [np.zeros(16, dtype=np.uint8)])).cuda()
    out = torch_cuda.full((len(expect),), 0xAB, dtype=torch_cuda.uint8, device="cuda")
    hip.unshuffle_blocks(tmp, out, torch_cuda.from_numpy(rec.view(np.uint8).copy()).cuda(), len(rec), int(rec["bsize"].max()))
    torch_cuda.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, (ts, bad[:8], [b for b in blocks if b[1] - GUARD <= bad[0] < b[1] + b[2] + GUARD][:1])
