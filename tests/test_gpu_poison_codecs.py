"""Every decode and encode entry with caller-owned scratch, `tmp` or slots, run with that buffer holding each fill of tests/poison.py
and, for the entries with a scratch proper, in the scratch an earlier, different batch left: the outputs (data, `errors`, `rounds`,
`csize`) are the same bits every time, and they are what the entry's existing test expects — the case writers' bytes, or the existing
test function itself, which runs here unchanged with `torch.empty` poisoned under it.  The kernels use no float atomics on global
memory, so one fill run twice must already agree bit for bit; that is checked first.

zstd_decode / inflate_decode: the batches of tests/poison_batches.py (catalogue, fuzz and every damaged case in one launch).
grib_unpack / _complex / _ccsds: the existing tests of their modules (good fields with and without a bitmap, every refused record,
the damaged CCSDS streams), every call of their `_run` recorded and compared across fills.  delta_decode, lz4_decode_streams +
unshuffle_blocks + bitunshuffle_blocks (`tmp`; the real c-blosc chunks of every flavour in one batch, Zstandard frames decoded into the
poisoned `tmp`), lzw_decode + tiff_place / tiff_place_bands (the decoded buffer), lz4_encode_streams (slots), zstd_encode_blocks
(scratch and slots): runners of their own over the existing catalogues."""
import numpy as np
import pytest

import poison
import poison_batches as pb

from aggfly_amd import codec

pytestmark = pytest.mark.gpu
FILLS = list(poison.FILLS)
_CACHE = {}


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _same(a, b):
    """Two recorded results — arrays, numbers, tuples of them — hold the same bits."""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))
    return a == b


# ---------------------------------------------------------------------------------------
# zstd_decode, inflate_decode
# ---------------------------------------------------------------------------------------
KINDS = {"zstd": pb.zstd_batches, "inflate": pb.inflate_batches}


def _scratch_bytes(kind, b):
    from aggfly_amd import hip
    return hip.zstd_scratch_bytes(b.plan) if kind == "zstd" else hip.inflate_scratch_bytes(b.plan)


def _decode(torch, kind, b, scratch):
    """One launch of ``b`` in ``scratch`` (a uint8 HBM tensor, used as it is) -> (output image, errors, rounds)."""
    from aggfly_amd import hip
    key = (kind, b.name)
    if key not in _CACHE:
        r0, r1 = b.records
        n0, n1 = (b.plan.n_frames, b.plan.n_blocks) if kind == "zstd" else (b.plan.n_streams, b.plan.n_shuf)
        _CACHE[key] = (_dev(torch, b.base), _dev(torch, r0[:max(n0, 1)]), _dev(torch, r1[:max(n1, 1)]))
    comp, d0, d1 = _CACHE[key]
    out = torch.full((b.nout,), pb.FILL, dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    rounds = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    (hip.zstd_decode if kind == "zstd" else hip.inflate_decode)(comp, b.base.nbytes, d0, d1, b.plan, scratch, out, errors, rounds)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(errors.item()), int(rounds.item())


@pytest.mark.parametrize("kind", list(KINDS))
def test_decode_is_a_function_of_its_inputs_under_every_fill(torch_cuda, kind):
    torch = torch_cuda
    b = KINDS[kind]()["A"]
    n = _scratch_bytes(kind, b)
    assert n == b.plan.scratch_bytes()
    first = _decode(torch, kind, b, poison.filled(torch, n, "random"))
    assert _same(first, _decode(torch, kind, b, poison.filled(torch, n, "random"))), "two runs of one fill differ"
    assert first[1] == b.errors and np.array_equal(first[0], b.want) and 1 <= first[2] <= 40
    for fill in ("zero", "ones", "plausible"):
        canary = 4096
        whole = poison.filled(torch, n + canary, fill)
        assert _same(first, _decode(torch, kind, b, whole[:n])), fill
        assert bool((whole[n:] == poison.filled(torch, n + canary, fill)[n:]).all()), "the bytes behind the scratch were written"
    assert _same(first, _decode(torch, kind, b, poison.filled(torch, n + 65536, "plausible"))), "a scratch larger than needed"


@pytest.mark.parametrize("kind", list(KINDS))
def test_decode_in_the_scratch_another_batch_left(torch_cuda, kind):
    """A (catalogue, fuzz, every damaged case: bad flags and half-built tables stay behind), then B in the same scratch with nothing
    refilled: B alone.  Then A, and A again: A."""
    torch = torch_cuda
    A, B = KINDS[kind]()["A"], KINDS[kind]()["B"]
    na, nb = _scratch_bytes(kind, A), _scratch_bytes(kind, B)
    assert A.errors >= 20 and B.errors == 0 and nb < na
    alone = {b.name: _decode(torch, kind, b, poison.filled(torch, n, "zero")) for b, n in ((A, na), (B, nb))}
    assert all(np.array_equal(alone[b.name][0], b.want) and alone[b.name][1] == b.errors for b in (A, B))
    scratch = poison.filled(torch, na, "random")
    for b, n in ((A, na), (B, nb), (A, na), (A, na)):
        assert _same(alone[b.name], _decode(torch, kind, b, scratch[:n])), b.name


# ---------------------------------------------------------------------------------------
# the three GRIB unpackers: their existing tests, with what `torch.empty` gives them poisoned or stale
# ---------------------------------------------------------------------------------------
def _params(fn):
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    return list(mark.args[1])


def _grib_simple(torch):
    import test_gpu_grib as G
    refused = _params(G.test_a_refused_record_writes_nothing_and_is_counted)
    for with_map, what in refused:                                   # batch A: good fields and every refused record
        G.test_a_refused_record_writes_nothing_and_is_counted(torch, with_map, what)
    for nbits, with_map in ((12, True), (16, False), (7, True), (0, False), (31, True)):      # whole grid, and a box in a larger cube
        G.test_unpack_against_the_case_writer(torch, nbits, with_map)
    G.test_three_widths_in_one_batch(torch)                          # batch B: another, smaller selection
    G.test_a_step_staged_from_the_middle_of_its_data(torch)
    for with_map, what in refused[::-4]:
        G.test_a_refused_record_writes_nothing_and_is_counted(torch, with_map, what)


def _grib_complex(torch):
    import test_gpu_grib_complex as G
    refused = _params(G.test_a_refused_record_writes_nothing_and_is_counted)
    for with_map, what in refused:
        G.test_a_refused_record_writes_nothing_and_is_counted(torch, with_map, what)
    for form, with_map, ny, nx in (("5.2", True, 37, 111), ("order1", False, 33, 130), ("order2", True, 1, 2 * G.TILE + 3), ("order2", False, 37, 111)):
        G.test_unpack_against_the_case_writer(torch, form, with_map, ny, nx)
    G.test_group_counts_257_1_and_0(torch)
    for with_map, what in refused[::-4]:
        G.test_a_refused_record_writes_nothing_and_is_counted(torch, with_map, what)


def _grib_ccsds(torch):
    import test_gpu_grib_ccsds as G
    refused = _params(G.test_a_refused_record_writes_nothing_and_is_counted)
    for with_map, what in refused:
        G.test_a_refused_record_writes_nothing_and_is_counted(torch, with_map, what)
    G.test_damaged_streams_are_counted_and_leave_the_cube_untouched(torch)
    for name, with_map in (("19x23", True), ("37x53", False), ("70x61", True)):
        G.test_unpack_against_the_case_writer(torch, name, with_map)
    G.test_nbits_0_and_differing_parameters_in_one_call(torch)
    G.test_damaged_streams_are_counted_and_leave_the_cube_untouched(torch)
    for with_map, what in refused[::-4]:
        G.test_a_refused_record_writes_nothing_and_is_counted(torch, with_map, what)


GRIB = {"grib_unpack": ("test_gpu_grib", _grib_simple), "grib_unpack_complex": ("test_gpu_grib_complex", _grib_complex),
        "grib_unpack_ccsds": ("test_gpu_grib_ccsds", _grib_ccsds)}


def _recorded(torch, module, scenario, arrange):
    """The results of every `_run` call of ``scenario`` (the existing tests' own assertions hold on the way), with ``arrange(mp)``
    deciding what `torch.empty` hands out meanwhile."""
    import importlib
    mod = importlib.import_module(module)
    log = []
    real = mod._run
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(mod, "_run", lambda *a, **k: (log.append(real(*a, **k)), log[-1])[1])
        handed = arrange(mp)
        scenario(torch)
    assert handed and len(log) >= 20, "the scenario's scratch did not come from torch.empty"
    return log


@pytest.mark.parametrize("entry", list(GRIB))
def test_grib_unpackers_under_every_fill_and_in_stale_scratch(torch_cuda, entry):
    torch = torch_cuda
    module, scenario = GRIB[entry]
    first = _recorded(torch, module, scenario, lambda mp: poison.poisoned_empty(mp, torch, "random"))
    assert _same(first, _recorded(torch, module, scenario, lambda mp: poison.poisoned_empty(mp, torch, "random"))), "two runs of one fill differ"
    for fill in ("zero", "ones", "plausible"):
        assert _same(first, _recorded(torch, module, scenario, lambda mp: poison.poisoned_empty(mp, torch, fill))), fill
    # one block for every call of the scenario, never refilled: each batch runs in what the batch before it left
    block = poison.filled(torch, 64 << 20, "random")
    assert _same(first, _recorded(torch, module, scenario, lambda mp: poison.stale_empty(mp, torch, block)))


# ---------------------------------------------------------------------------------------
# delta_decode
# ---------------------------------------------------------------------------------------
def _delta(torch, enc, scratch):
    from aggfly_amd import hip
    stage = _dev(torch, enc)
    hip.delta_decode(stage, enc.shape[0], enc.shape[1], enc.dtype.itemsize, scratch)
    torch.cuda.synchronize()
    return stage.cpu().numpy().view(enc.dtype).reshape(enc.shape)


@pytest.mark.parametrize("es", [1, 2, 4, 8])
def test_delta_decode_under_every_fill_and_in_stale_scratch(torch_cuda, es):
    import zarr_filter_cases as Z
    from aggfly_amd import hip
    from test_gpu_zarr_filters import TILE_BYTES, WG
    torch = torch_cuda
    dt = np.dtype(f"i{es}")
    tile = TILE_BYTES // es
    rng = np.random.default_rng(40 + es)
    batches = {}
    for name, (n_chunks, n) in {"A": (3, (WG + 1) * tile + 5), "B": (7, 3 * tile + 17), "one tile": (2, tile - 1)}.items():
        enc = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, size=(n_chunks, n), endpoint=True, dtype=np.int64).astype(dt)
        batches[name] = (enc, np.stack([Z.delta_decode_fast(row, dt) for row in enc]), hip.delta_scratch_bytes(n_chunks, n, es))
    for name, (enc, want, sbytes) in batches.items():
        for fill in FILLS:
            assert np.array_equal(_delta(torch, enc, poison.filled(torch, sbytes + 64, fill)[:sbytes]), want), (name, fill)
    scratch = poison.filled(torch, max(s for _, _, s in batches.values()) + 256, "random")
    for name in ("A", "B", "one tile", "A", "A"):
        enc, want, sbytes = batches[name]
        assert np.array_equal(_delta(torch, enc, scratch[:sbytes]), want), name


# ---------------------------------------------------------------------------------------
# lz4_decode_streams (tmp) + unshuffle_blocks + bitunshuffle_blocks, zstd_decode into the poisoned tmp
# ---------------------------------------------------------------------------------------
def _flavours(torch, base, out_off, lists, p, fill):
    """`_run` of test_gpu_blosc_flavours.py with `tmp` and the Zstandard scratch holding ``fill`` -> (out on the host, errors)."""
    from aggfly_amd import hip
    counts = (p.n_streams, p.n_shuf, p.n_bits, p.n_frames, p.n_blocks)
    comp = torch.from_numpy(base).cuda()
    st, sh, bt, fr, zb = (_dev(torch, a[:max(n, 1)]) for a, n in zip(lists, counts))
    out = torch.full((max(int(out_off[-1]), 64),), 0xAB, dtype=torch.uint8, device="cuda")
    tmp = poison.filled(torch, max(p.tmp_bytes, 64), fill)
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.lz4_decode_streams(comp, st, p.n_streams, p.max_dsize, tmp, out, errors)
    hip.zstd_decode(comp, base.nbytes, fr, zb, p, poison.filled(torch, hip.zstd_scratch_bytes(p), fill), tmp, errors)
    hip.unshuffle_blocks(tmp, out, sh, p.n_shuf, p.max_shuf)
    hip.bitunshuffle_blocks(tmp, out, bt, p.n_bits, p.max_bits)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(errors.item())


def test_blosc_flavours_with_a_poisoned_tmp(torch_cuda):
    """The real c-blosc chunks of every flavour in one batch (test_real_cblosc_chunks_of_every_flavour_decode_in_one_batch), and the
    catalogue streams of tests/lz4_streams.py wrapped as byte planes."""
    import base64
    import lz4_streams as lz
    import test_gpu_blosc_flavours as F
    cases = [c for c in F.CASES if c["cname"] in ("lz4", "lz4hc", "zstd")]
    chunks = [base64.b64decode(c["chunk_b64"]) for c in cases] + [c[2] for c in lz.wrapped_chunks()]
    raws = [F.recipe(c["recipe"], c["n"], c["dtype"], c["seed"]).tobytes() for c in cases] + [c[4] for c in lz.wrapped_chunks()]
    nbytes = [len(r) for r in raws]
    base, out_off, lists, p = F._plan(chunks, nbytes)
    assert p.n_streams and p.n_shuf and p.n_bits and p.n_frames and (p.results == nbytes).all()
    want = np.full(max(int(out_off[-1]), 64), 0xAB, dtype=np.uint8)
    for o, r in zip(out_off, raws):
        want[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    for fill in ["random"] + FILLS:
        host, errors = _flavours(torch_cuda, base, out_off, lists, p, fill)
        assert errors == 0 and np.array_equal(host, want), fill


def test_lz4_decode_streams_into_a_poisoned_tmp_and_out(torch_cuda):
    """The catalogue and the stored records of test_catalogue_streams_decode_bit_exact, and the damaged streams between good ones:
    every destination holds what the case writer says, every other byte of `tmp` and `out` what it held before."""
    import lz4_streams as lz
    from test_gpu_lz4_streams import _positive
    from aggfly_amd import hip
    torch = torch_cuda
    items, _ = _positive(lz.catalogue())
    rng = np.random.default_rng(9)
    stored = [(rng.bytes(n), sa, da) for n in lz.STORED_SIZES for sa, da in ((True, True), (False, True), (True, False))]
    good, _ = _positive([c for c in lz.catalogue() if c[0] in ("pack_21x3", "chain_4_4", "off_7_fast", "lit_16", "far_4097_fast")])
    mixed = [good[0]]
    for j, (_, stream, dsize) in enumerate(lz.damaged()):
        mixed += [(stream, dsize, None), good[(j + 1) % len(good)]]
    for what, (comp, recs, image, mask), want_err in (("catalogue", lz.layout(items, stored), 0), ("damaged", lz.layout(mixed), len(lz.damaged()))):
        written = {k: image[k] != 0xAB for k in (0, 1)}              # (a lower bound of the bytes a good stream owns; the rest is compared below)
        owned = {k: np.zeros(len(image[k]), dtype=bool) for k in (0, 1)}
        for r in recs:
            owned[int(r["to_out"] != 0)][r["dst_off"]:r["dst_off"] + r["dsize"]] = True
        assert all((owned[k] | ~written[k]).all() for k in (0, 1))
        cd, rd = torch.from_numpy(comp).cuda(), _dev(torch, recs)
        for fill in ["random"] + FILLS:
            dev = {k: poison.filled(torch, len(image[k]), fill) for k in (0, 1)}
            before = {k: dev[k].cpu().numpy() for k in (0, 1)}
            errors = torch.zeros(1, dtype=torch.int32, device="cuda")
            hip.lz4_decode_streams(cd, rd, len(recs), int(recs["dsize"].max()), dev[0], dev[1], errors)
            torch.cuda.synchronize()
            assert int(errors.item()) == want_err, (what, fill)
            for k in (0, 1):
                got = dev[k].cpu().numpy()
                keep = owned[k] if mask is None else owned[k] & mask[k]          # (mask: all but the damaged streams' own destinations)
                assert np.array_equal(got[keep], image[k][keep]), (what, fill, k)
                assert np.array_equal(got[~owned[k]], before[k][~owned[k]]), (what, fill, k, "a byte outside every destination was written")


# ---------------------------------------------------------------------------------------
# lz4_encode_streams (slots), zstd_encode_blocks (scratch, slots)
# ---------------------------------------------------------------------------------------
GUARD = 64


def _encode(torch, kind, items, fill, scratch=None):
    """One launch over ``items`` = [(input, the emulation's bytes)], slots between guards, slots (and scratch) holding ``fill`` ->
    (csize, the bytes of every slot up to its csize); nothing else of the slots image may have changed."""
    from aggfly_amd import hip
    zstd = kind == "zstd"
    rec = np.zeros(len(items), dtype=codec.ZSTD_ENCODE_BLOCK if zstd else codec.LZ4_STREAM)
    src_off = dst_off = 0
    scratch_off = hip.load().afhip_zstd_encode_scratch_bytes(0) if zstd else 0
    for i, (data, _) in enumerate(items):
        dst_off += GUARD
        rec[i] = (src_off, dst_off, scratch_off, len(data), i & 1) if zstd else (src_off, dst_off, 0, len(data), 0, 0)
        src_off += len(data)
        dst_off += len(data) + (3 if zstd else 0)
        scratch_off += hip.load().afhip_zstd_encode_scratch_bytes(len(data)) if zstd else 0
    inp = np.frombuffer(b"".join(d for d, _ in items) + b"\0", dtype=np.uint8)
    slots = poison.filled(torch, dst_off + GUARD, fill)
    before = slots.cpu().numpy()
    csize = torch.full((len(items),), -1, dtype=torch.int32, device="cuda")
    if zstd:
        scratch = poison.filled(torch, scratch_off, fill) if scratch is None else scratch[:scratch_off]
        hip.zstd_encode_blocks(_dev(torch, inp), _dev(torch, rec), len(rec), scratch, slots, csize)
    else:
        hip.lz4_encode_streams(_dev(torch, inp), _dev(torch, rec), len(rec), slots, csize)
    torch.cuda.synchronize()
    got, csize = slots.cpu().numpy(), csize.cpu().numpy()
    want_csize = np.array([len(w) for _, w in items], dtype=np.int32)
    assert np.array_equal(csize, want_csize), [(i, int(csize[i]), int(want_csize[i])) for i in np.nonzero(csize != want_csize)[0][:5]]
    mine = np.zeros(len(got), dtype=bool)
    for r, (_, want) in zip(rec, items):
        assert got[r["dst_off"]:r["dst_off"] + len(want)].tobytes() == want, int(r["dst_off"])
        mine[r["dst_off"]:r["dst_off"] + len(want)] = True
    assert np.array_equal(got[~mine], before[~mine]), "a byte outside the streams was written"
    return scratch_off


def _encode_items(kind):
    if kind not in _CACHE:
        if kind == "zstd":
            import zstd_encode_cases as zc
            _CACHE[kind] = [(data, codec.zstd_encode_block_emulate(data, last=bool(i & 1))) for i, (_, data, _) in enumerate(zc.catalogue())]
        else:
            import lz4_encode_cases as lc
            _CACHE[kind] = [(data, codec.lz4_encode_emulate(data)) for _, data, _ in lc.catalogue()]
    return _CACHE[kind]


@pytest.mark.parametrize("kind", ["lz4", "zstd"])
def test_encoders_with_poisoned_slots_and_scratch(torch_cuda, kind):
    items = _encode_items(kind)
    for fill in ["random"] + FILLS:
        _encode(torch_cuda, kind, items, fill)


def test_zstd_encode_blocks_in_the_scratch_another_batch_left(torch_cuda):
    """The blocks' Last_Block bits follow their position in the batch, so B's expectation is the emulation's for B's own order."""
    torch = torch_cuda
    datas = [d for d, _ in _encode_items("zstd")]
    A = _encode_items("zstd")
    B = [(d, codec.zstd_encode_block_emulate(d, last=bool(i & 1))) for i, d in enumerate(datas[::-3])]
    scratch = poison.filled(torch, _encode(torch, "zstd", A, "zero"), "random")
    for batch in (A, B, A, A):
        _encode(torch, "zstd", batch, "plausible", scratch=scratch)


# ---------------------------------------------------------------------------------------
# lzw_decode + tiff_place / tiff_place_bands: the decoded buffer
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bands", [1, 3])
def test_lzw_decode_and_tiff_place_with_a_poisoned_decoded_buffer(torch_cuda, bands):
    """The decoded segments of the existing placement tests (37 x 70 in 16 x 16 tiles with junk in the padding, and in strips of 5
    rows; float32 under predictor 3, big-endian uint16 under predictor 2), each written as a TIFF LZW stream by the case writer, with
    the damaged streams of the stream catalogue between them: decoded into a buffer that held each fill and placed from there.  The
    cube is the writer's array bit for bit, a box of it lands in a larger cube whose other bytes stay, the damaged streams are
    counted and skipped, and the decoded buffer is the same under every fill outside their destinations."""
    import tiff_cases as TC
    import test_gpu_tiff as T1
    import test_gpu_tiff_bands as TB
    from aggfly_amd import hip
    torch = torch_cuda
    broken = [s for s in TC.stream_catalogue() if s[3] is None][:6]
    assert len(broken) >= 4
    for dt, predictor, byteorder, tile, rps in (("f4", 3, "<", (16, 16), None), ("u2", 2, ">", None, 5)):
        if bands == 1:
            values = TC.field(dt, 2, seed=5)
            blob, rec = T1._segments(values, tile, rps, predictor, byteorder)
        else:
            values = TB._field(dt, bands)
            blob, rec = TB._segments(values, tile, rps, predictor, byteorder)
        swap = byteorder == ">"
        NT, H, W = values.shape
        rec = np.concatenate([rec, np.zeros(len(broken), dtype=hip.TIFF_SEG)])
        rec[-len(broken):]["rows"], rec[-len(broken):]["pitch"] = 1, 1
        stage, dec_at = bytearray(), 0
        for i, r in enumerate(rec):
            if i < len(rec) - len(broken):
                comp = TC.lzw_encode(blob[int(r["dec_off"]):int(r["dec_off"] + r["dec_bytes"])].tobytes())
            else:
                comp, r["dec_bytes"] = broken[i - len(rec)][1], broken[i - len(rec)][2]
            r["src_off"], r["src_bytes"], r["dec_off"] = len(stage), len(comp), dec_at
            stage += comp + b"\xee"
            dec_at += (int(r["dec_bytes"]) + 15) // 16 * 16
        rec = rec[np.random.default_rng(2).permutation(len(rec))]
        good = np.zeros(dec_at, dtype=bool)
        for r in rec:
            if r["rows"] != 1 or r["pitch"] != 1:
                good[int(r["dec_off"]):int(r["dec_off"] + r["dec_bytes"])] = True
        sd = _dev(torch, np.frombuffer(bytes(stage), np.uint8))
        tdt = {2: torch.int16, 4: torch.int32}[values.dtype.itemsize]
        box, at, shape = (3, 9, 20, 41), (1, 2, 3), (NT + 2, 24, 46)
        first = None
        for fill in ["random"] + FILLS:
            decoded = poison.filled(torch, dec_at, fill)
            before = decoded.cpu().numpy()
            recs = _dev(torch, rec)
            errors = torch.zeros(1, dtype=torch.int32, device="cuda")
            hip.lzw_decode(sd, recs, len(rec), decoded, errors)
            cube = poison.filled(torch, values.nbytes, fill).view(tdt).view(values.shape)
            larger = poison.filled(torch, int(np.prod(shape)) * values.dtype.itemsize, fill).view(tdt).view(shape)
            was = larger.cpu().numpy().view(values.dtype).copy()
            for c, b, a in ((cube, (0, 0, H, W), (0, 0, 0)), (larger, box, at)):
                if bands == 1:
                    hip.tiff_place(decoded, recs, len(rec), int(rec["rows"].max()), predictor, swap, c, b, a, errors)
                else:
                    hip.tiff_place_bands(decoded, recs, len(rec), int(rec["rows"].max()), bands, predictor, swap, c, b, a, errors)
            torch.cuda.synchronize()
            assert int(errors.item()) == len(broken), (dt, fill)
            after = recs.cpu().numpy().view(hip.TIFF_SEG)
            assert np.array_equal(after["bad"] != 0, (rec["rows"] == 1) & (rec["pitch"] == 1))
            T1._same_bits(cube.cpu().numpy().view(values.dtype), values)
            was[at[0]:at[0] + NT, at[1]:at[1] + box[2], at[2]:at[2] + box[3]] = values[:, box[0]:box[0] + box[2], box[1]:box[1] + box[3]]
            T1._same_bits(larger.cpu().numpy().view(values.dtype), was)
            dec = decoded.cpu().numpy()
            assert np.array_equal(dec[~good], before[~good]), "a damaged stream's output, or the padding, was written"
            first = dec[good] if first is None else first
            assert np.array_equal(dec[good], first), (dt, fill)
