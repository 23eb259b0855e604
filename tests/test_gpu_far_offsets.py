"""The placement, decode and encode entries writing beyond element 2^31 and byte 2^32 of their destination.

The cube is (2051, 1021, 1031), one per element size (2.2, 4.3, 8.6 and 17.3 GB), every element a recognisable integer.  Its element
index passes 2^31 between t = 2040 and t = 2041 (2040 * 1 052 651 = 2 147 408 040 < 2^31 < 2 148 460 691 = 2041 * 1 052 651); the
2-byte cube passes byte 2^32 at the same place, the 4- and 8-byte cubes pass both limits earlier.  Every entry runs twice, into a box
that straddles the limit (t in [2039, 2044)) and into one wholly beyond it, both near the far corner in y and x, with the small inputs
and the expectation of its existing test; then the box is overwritten with the fill on the device and the whole cube must equal the
fill again (one reduction on the device, nothing copied to the host): a store that went anywhere else is seen.  The record family
(`dst_off`, `out_off`, `src_off`, `tmp_off`) writes into one buffer of 2^32 + 2^20 bytes: one record near 0 as a control, one whose
destination straddles byte 2^32, one beyond it.

The index arithmetic of every kernel named here is 64-bit (read before this file was written); these tests guard that.
They need up to about 40 GB of free HBM and skip below that, as tests/test_gpu_fullsize.py does."""
import zlib

import numpy as np
import pytest

from aggfly_amd import codec

pytestmark = pytest.mark.gpu

SHAPE = (2051, 1021, 1031)
PLANE = SHAPE[1] * SHAPE[2]
assert 2040 * PLANE < 2 ** 31 < 2041 * PLANE
FILL = {1: 0x5A, 2: 0x5A5B, 4: 0x5A5B5C5D, 8: 0x5A5B5C5D5E5F6061}
INT = {1: "int8", 2: "int16", 4: "int32", 8: "int64"}
STRADDLE, BEYOND = 2039, 2045                    # first time step of the two boxes (5 steps each where the input has as many)
BIG = 2 ** 32 + 2 ** 20
BYTE = 0xAB

# every entry of include/aggfly_hip.h that places into or takes from a cube, or reads records with a destination offset -> where it
# is held to far offsets here (tests/test_entry_catalogue_host.py keeps the table level with the header)
FAR_ENTRIES = {
    "afhip_place_box": "cube", "afhip_place_box_swapped": "cube", "afhip_place_box_tlast": "cube", "afhip_take_box": "cube (reading)",
    "afhip_grib_unpack": "cube", "afhip_grib_unpack_complex": "cube", "afhip_grib_unpack_ccsds": "cube",
    "afhip_tiff_place": "cube", "afhip_tiff_place_bands": "cube",
    "afhip_lz4_decode_streams": "records: dst_off with to_out", "afhip_unshuffle_blocks": "records: out_off",
    "afhip_bitunshuffle_blocks": "records: out_off", "afhip_zstd_decode": "records: frame dst_off",
    "afhip_inflate_decode": "records: dst_off, and out_off of the shuffled chunk", "afhip_copy_ranges": "records: dst_off and src_off",
    "afhip_shuffle_blocks": "records: tmp_off and out_off", "afhip_lz4_encode_streams": "records: dst_off of the slots, src_off",
    "afhip_zstd_encode_blocks": "records: dst_off of the slots, src_off",
}


def _need(torch, gb):
    free, _ = torch.cuda.mem_get_info()
    if free < gb * 2 ** 30:
        pytest.skip(f"needs {gb} GB of free HBM")


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Cube:
    """The cube of one element size, full of FILL; `check(box)` overwrites the box with the fill and reduces the whole cube."""

    def __init__(self, torch, elem):
        self.torch, self.elem = torch, elem
        self.fill = int(np.array([FILL[elem]], dtype=f"u{elem}").view(INT[elem])[0])
        self.t = torch.empty(SHAPE, dtype=getattr(torch, INT[elem]), device="cuda")
        self.t.fill_(self.fill)

    def corner(self, ny, nx, k=0):
        return SHAPE[1] - ny - 1 - k, SHAPE[2] - nx - 2 - k

    def box(self, t0, nt, y, ny, x, nx):
        return self.t[t0:t0 + nt, y:y + ny, x:x + nx]

    def check(self, what, t0, nt, y, ny, x, nx, want):
        """The box holds ``want`` (numpy, any dtype of the element size, compared bit for bit); everything else the fill."""
        assert (t0 + nt) * PLANE > 2 ** 31 and t0 + nt <= SHAPE[0]
        got = self.box(t0, nt, y, ny, x, nx).cpu().numpy()
        want = np.ascontiguousarray(want).view(INT[self.elem]).reshape(got.shape)
        assert np.array_equal(got, want), f"{what}: the box at t0={t0} differs"
        self.box(t0, nt, y, ny, x, nx).fill_(self.fill)
        assert bool((self.t == self.fill).all()), f"{what}: a store landed outside the box at t0={t0}"


def _cube(torch, elem):
    _need(torch, 8 + 2.3 * elem * 1.6)            # the cube, the reduction's mask (one byte per element) and some air
    return Cube(torch, elem)


# ---------------------------------------------------------------------------------------
# place_box, place_box_swapped, place_box_tlast, take_box, tiff_place, tiff_place_bands
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem", [2, 4, 8])
def test_place_and_take_boxes_far_into_the_cube(torch_cuda, elem):
    from aggfly_amd import hip
    torch = torch_cuda
    c = _cube(torch, elem)
    rng = np.random.default_rng(elem)
    bt, by, bx = 7, 11, 70                        # the chunk; its part (1.., 2.., 3..) of 5 x 7 x 65 goes to the cube
    nt, ny, nx = 5, 7, 65
    chunk = rng.integers(1, 2 ** 15, size=(bt, by, bx)).astype(INT[elem])
    part = chunk[1:1 + nt, 2:2 + ny, 3:3 + nx]
    tlast = np.ascontiguousarray(chunk.transpose(1, 2, 0))                    # [by, bx, bt], time fastest
    d, dl = torch.from_numpy(chunk).cuda(), torch.from_numpy(tlast).cuda()
    for k, t0 in enumerate((STRADDLE, BEYOND)):
        y, x = c.corner(ny, nx, k)
        hip.place_box(d, c.t, (1, 2, 3, nt, ny, nx), (t0, y, x))
        c.check("place_box", t0, nt, y, ny, x, nx, part)
        hip.place_box_swapped(d, c.t, (1, 2, 3, nt, ny, nx), (t0, y, x))
        c.check("place_box_swapped", t0, nt, y, ny, x, nx, part.byteswap())
        hip.place_box_tlast(dl, c.t, (2, 3, 1, ny, nx, nt), (t0, y, x))
        c.check("place_box_tlast", t0, nt, y, ny, x, nx, part)
        # take_box reads there: the box holds the part, the chunk buffer is larger than the box and padded with 7
        c.box(t0, nt, y, ny, x, nx).copy_(torch.from_numpy(np.ascontiguousarray(part)).cuda())
        got = torch.zeros((nt + 1, ny + 2, nx + 3), dtype=c.t.dtype, device="cuda")
        hip.take_box(c.t, got, (t0, y, x), (nt, ny, nx), 7)
        want = np.full((nt + 1, ny + 2, nx + 3), 7, dtype=INT[elem])
        want[:nt, :ny, :nx] = part
        assert np.array_equal(got.cpu().numpy(), want), ("take_box", t0)
        c.check("take_box (the cube is only read)", t0, nt, y, ny, x, nx, part)


@pytest.mark.parametrize("elem,dt,predictor,byteorder", [(1, "u1", 2, "<"), (2, "u2", 2, ">"), (4, "f4", 3, "<"), (8, "f8", 3, ">")])
def test_tiff_place_far_into_the_cube(torch_cuda, elem, dt, predictor, byteorder):
    """The decoded segments of tests/test_gpu_tiff.py (3 pages of 37 x 70 in 16 x 16 tiles, junk in the padding) and of
    tests/test_gpu_tiff_bands.py (one chunky page of 3 bands), placed whole."""
    import tiff_cases as TC
    import test_gpu_tiff as T1
    import test_gpu_tiff_bands as TB
    from aggfly_amd import hip
    torch = torch_cuda
    c = _cube(torch, elem)
    swap = byteorder == ">" and elem > 1
    pages = TC.field(dt, 3, seed=5)
    blob1, rec1 = T1._segments(pages, (16, 16), None, predictor, byteorder)
    bands = TB._field(dt, 3)
    blob3, rec3 = TB._segments(bands, (16, 16), None, predictor, byteorder)
    H, W = pages.shape[1:]
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k, t0 in enumerate((STRADDLE + 1, BEYOND)):
        y, x = c.corner(H, W, k)
        hip.tiff_place(_dev(torch, blob1), _dev(torch, rec1), len(rec1), int(rec1["rows"].max()), predictor, swap, c.t, (0, 0, H, W), (t0, y, x), errors)
        c.check("tiff_place", t0, 3, y, H, x, W, pages)
        hip.tiff_place_bands(_dev(torch, blob3), _dev(torch, rec3), len(rec3), int(rec3["rows"].max()), 3, predictor, swap, c.t, (0, 0, H, W), (t0, y, x), errors)
        c.check("tiff_place_bands", t0, 3, y, H, x, W, bands)
    assert int(errors.item()) == 0


# ---------------------------------------------------------------------------------------
# the three GRIB unpackers (float32 cubes)
# ---------------------------------------------------------------------------------------
def test_grib_unpackers_far_into_the_cube(torch_cuda):
    """Three 12-bit fields with a bitmap (simple packing), two second-order fields with a bitmap (complex packing) and the 19 x 23
    fields with a bitmap (CCSDS) of the existing kernel tests, a box of each at an offset."""
    import test_gpu_grib as G
    import test_gpu_grib_complex as K
    import test_gpu_grib_ccsds as A
    from aggfly_amd import hip
    torch = torch_cuda
    c = _cube(torch, 4)
    cube = c.t.view(torch.float32)
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")

    def simple(t0, k):
        steps, want = G._fields(12, True)
        stage, rec = G._stage(steps, G.NY * G.NX)
        box = (2, 3, 29, 124)
        y, x = c.corner(box[2], box[3], k)
        hip.grib_unpack(_dev(torch, stage), _dev(torch, rec), len(rec), (G.NY, G.NX), box, cube, (t0, y, x), scratch(hip.grib_rank_bytes(len(rec), G.NY * G.NX)), errors)
        c.check("grib_unpack", t0, len(rec), y, box[2], x, box[3], want[:, 2:31, 3:127])

    def complex_(t0, k):
        ny, nx = 37, 111
        steps, wants = zip(*[K._field("order2", True, ny, nx, seed) for seed in range(2)])
        stage, rec = K._stage(steps)
        box = (2, 3, ny - 4, nx - 6)
        y, x = c.corner(box[2], box[3], k)
        mg = int(rec["n_groups"].max())
        hip.grib_unpack_complex(_dev(torch, stage), _dev(torch, rec), len(rec), 2, mg, (ny, nx), box, cube, (t0, y, x),
                                scratch(hip.grib_complex_scratch_bytes(len(rec), ny * nx, mg)), errors)
        c.check("grib_unpack_complex", t0, len(rec), y, box[2], x, box[3], np.stack(wants)[:, 2:ny - 2, 3:nx - 3])

    def ccsds(t0, k):
        steps, ny, nx = A._grid_steps("19x23", True)
        want = np.stack([s.expected(ny, nx) for s in steps])
        stage, rec = A._stage(steps)
        box = (2, 3, ny - 4, nx - 6)
        y, x = c.corner(box[2], box[3], k)
        mr = A._max_rsis(rec)
        hip.grib_unpack_ccsds(_dev(torch, stage), _dev(torch, rec), len(rec), mr, (ny, nx), box, cube, (t0, y, x),
                              scratch(hip.grib_ccsds_scratch_bytes(len(rec), ny * nx, mr)), errors)
        c.check("grib_unpack_ccsds", t0, len(rec), y, box[2], x, box[3], want[:, 2:ny - 2, 3:nx - 3])

    for k, t0 in enumerate((STRADDLE + 1, BEYOND)):               # (two or three steps: 2040 .. 2042 straddles the limit)
        simple(t0, k)
        complex_(t0, k)
        ccsds(t0, k)
    torch.cuda.synchronize()
    assert int(errors.item()) == 0


# ---------------------------------------------------------------------------------------
# the record family: one buffer of 2^32 + 2^20 bytes
# ---------------------------------------------------------------------------------------
def _places(n):
    """Three destinations of n bytes: a control near 0, one that straddles byte 2^32 at an odd address, one beyond it."""
    return [4096 + 3, 2 ** 32 - n // 2 - 1, 2 ** 32 + 2 ** 19 + 5]


class Big:
    def __init__(self, torch):
        _need(torch, 14)
        self.torch = torch
        self.t = torch.full((BIG,), BYTE, dtype=torch.uint8, device="cuda")

    def check(self, what, offs, wants):
        for o, w in zip(offs, wants):
            assert o + len(w) <= BIG
            assert self.t[o:o + len(w)].cpu().numpy().tobytes() == bytes(w), f"{what}: the destination at byte {o} differs"
            self.t[o:o + len(w)] = BYTE
        assert offs[1] < 2 ** 32 < offs[1] + len(wants[1]) and offs[2] > 2 ** 32
        assert bool((self.t == BYTE).all()), f"{what}: a byte outside the destinations was written"


def test_records_with_far_destination_offsets(torch_cuda):
    import inflate_cases as ic
    import lz4_streams as lz
    import zstd_frames as zs
    from test_gpu_blosc_flavours import bit_unshuffle_reference
    from aggfly_amd import hip
    torch = torch_cuda
    big = Big(torch)
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(32)

    # lz4_decode_streams, to_out
    name, seqs, tail = next(x for x in lz.catalogue() if x[0] == "far_4097_fast")
    stream, want = lz.build(seqs, tail), lz.expand(seqs, tail)
    offs = _places(len(want))
    rec = np.array([(0, o, len(stream), len(want), 1, 0) for o in offs], dtype=codec.LZ4_STREAM)
    hip.lz4_decode_streams(_dev(torch, np.frombuffer(stream + b"\0" * 64, np.uint8)), _dev(torch, rec), 3, len(want), None, big.t, errors)
    big.check("lz4_decode_streams", offs, [want] * 3)

    # unshuffle_blocks, bitunshuffle_blocks: tmp small, out far; shuffle_blocks: out small, tmp far
    ts, n = 4, 40_000
    raw = rng.integers(0, 256, n * ts + 3, dtype=np.uint8)
    unshuffled = raw.copy()
    unshuffled[:n * ts] = raw[:n * ts].reshape(ts, n).T.reshape(-1)
    offs = _places(len(raw))
    rec = np.array([(0, o, len(raw), ts) for o in offs], dtype=codec.SHUFFLE_BLOCK)
    small = _dev(torch, raw)
    hip.unshuffle_blocks(small, big.t, _dev(torch, rec), 3, len(raw))
    big.check("unshuffle_blocks", offs, [unshuffled.tobytes()] * 3)
    hip.bitunshuffle_blocks(small, big.t, _dev(torch, rec), 3, len(raw))
    big.check("bitunshuffle_blocks", offs, [bit_unshuffle_reference(raw, ts).tobytes()] * 3)
    rec = np.array([(o, 0, len(raw), ts) for o in offs], dtype=codec.SHUFFLE_BLOCK)          # tmp_off far, out_off = the small input
    hip.shuffle_blocks(_dev(torch, unshuffled), big.t, _dev(torch, rec), 3, len(raw))
    big.check("shuffle_blocks", offs, [raw.tobytes()] * 3)

    # zstd_decode: frame dst_off
    cat = {nm: fd for nm, _, fd in zs.catalogue()}
    frame, want = zs.build(cat["rep0-minus-1-three-times"]), zs.expand(cat["rep0-minus-1-three-times"])
    offs = _places(len(want))
    base = np.frombuffer(frame * 3, dtype=np.uint8).copy()
    fr, bl = np.zeros(4, dtype=codec.ZSTD_FRAME), np.zeros(64, dtype=codec.ZSTD_BLOCK)
    p = codec.zstd_plan(base, [0, len(frame), 2 * len(frame)], [len(frame)] * 3, offs, [len(want)] * 3, fr, bl)
    assert list(fr["dst_off"][:3]) == offs
    hip.zstd_decode(_dev(torch, base), base.nbytes, _dev(torch, fr[:3]), _dev(torch, bl[:p.n_blocks]), p,
                    torch.full((hip.zstd_scratch_bytes(p),), 0xFF, dtype=torch.uint8, device="cuda"), big.t, errors)
    big.check("zstd_decode", offs, [want] * 3)

    # inflate_decode: dst_off of plain streams, out_off of a shuffled chunk
    part = ic.SHUF[100000:120000]
    streams = [zlib.compress(part, 6), zlib.compress(ic.shuffle(part, 4), 4), zlib.compress(part, 1)]
    offs = _places(len(part))
    co = np.concatenate([[0], np.cumsum([(len(s) + 63) // 64 * 64 for s in streams])]).astype(np.int64)
    base = np.zeros(int(co[-1]), dtype=np.uint8)
    for o, s in zip(co, streams):
        base[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    st, sh = np.zeros(4, dtype=codec.INFLATE_STREAM), np.zeros(4, dtype=codec.SHUFFLE_BLOCK)
    p = codec.inflate_plan(base, co[:-1], [len(s) for s in streams], offs, [len(part)] * 3, st, sh, typesize=np.array([1, 4, 1], dtype=np.int32))
    assert p.n_shuf == 1 and sh[0]["out_off"] == offs[1] and list(st["dst_off"][[0, 2]]) == [offs[0], offs[2]]
    hip.inflate_decode(_dev(torch, base), base.nbytes, _dev(torch, st[:3]), _dev(torch, sh[:1]), p,
                       torch.full((hip.inflate_scratch_bytes(p),), 0xFF, dtype=torch.uint8, device="cuda"), big.t, errors)
    big.check("inflate_decode", offs, [part] * 3)

    # copy_ranges: dst_off far, then src_off far
    data = rng.integers(0, 256, 70_001, dtype=np.uint8)
    offs = _places(len(data))
    rec = np.array([(5, o, len(data)) for o in offs], dtype=codec.COPY_RANGE)
    hip.copy_ranges(_dev(torch, np.concatenate([np.zeros(5, np.uint8), data])), big.t, _dev(torch, rec), 3)
    big.check("copy_ranges (dst_off)", offs, [data.tobytes()] * 3)
    for o in offs:
        big.t[o:o + len(data)] = torch.from_numpy(data).cuda()
    dst = torch.full((3 * len(data) + 64,), BYTE, dtype=torch.uint8, device="cuda")
    rec = np.array([(o, 16 + i * len(data), len(data)) for i, o in enumerate(offs)], dtype=codec.COPY_RANGE)
    hip.copy_ranges(big.t, dst, _dev(torch, rec), 3)
    want = np.full(len(dst), BYTE, dtype=np.uint8)
    want[16:16 + 3 * len(data)] = np.tile(data, 3)
    assert np.array_equal(dst.cpu().numpy(), want), "copy_ranges (src_off)"
    big.check("copy_ranges (the source is only read)", offs, [data.tobytes()] * 3)

    # lz4_encode_streams, zstd_encode_blocks: the slots far (dst_off), the input far (src_off)
    text = (b"far offsets " * 900 + bytes(rng.integers(0, 256, 500, dtype=np.uint8)))[:9000]
    offs = _places(len(text) + 3)
    for o in offs:                                                            # the input lies in the big buffer as well, behind each slot
        big.t[o + 16384:o + 16384 + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    csize = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    want = codec.lz4_encode_emulate(text)
    rec = np.array([(o + 16384, o, 0, len(text), 0, 0) for o in offs], dtype=codec.LZ4_STREAM)
    hip.lz4_encode_streams(big.t, _dev(torch, rec), 3, big.t, csize)
    assert csize.tolist() == [len(want)] * 3
    spans = [want + bytes([BYTE]) * (16384 - len(want)) + text for _ in offs]
    big.check("lz4_encode_streams", offs, spans)
    for o in offs:
        big.t[o + 16384:o + 16384 + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    want = codec.zstd_encode_block_emulate(text, last=True)
    s0, s1 = (int(hip.load().afhip_zstd_encode_scratch_bytes(v)) for v in (0, len(text)))
    rec = np.array([(o + 16384, o, s0 + i * s1, len(text), 1) for i, o in enumerate(offs)], dtype=codec.ZSTD_ENCODE_BLOCK)
    hip.zstd_encode_blocks(big.t, _dev(torch, rec), 3, torch.full((s0 + 3 * s1,), 0xFF, dtype=torch.uint8, device="cuda"), big.t, csize)
    assert csize.tolist() == [len(want)] * 3
    big.check("zstd_encode_blocks", offs, [want + bytes([BYTE]) * (16384 - len(want)) + text for _ in offs])
    torch.cuda.synchronize()
    assert int(errors.item()) == 0
