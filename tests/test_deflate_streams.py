"""The deflate route (`afcodec_inflate_plan` in blosc1.c, the passes of inflate_passes.h run on the host by `afcodec_inflate_emulate`)
held to the hand-built streams of tests/deflate_streams.py: every stream of the catalogue and 300 fuzzed ones mean to zlib and to
the strict RFC 1951 decoder what their descriptions say, the planner takes them with records inside their buffers, and the passes
rebuild them bit for bit, cut into the pseudo-blocks that the rule of inflate_passes.h gives; every damaged stream is refused by
zlib, by the strict decoder and by the passes, exactly once and inside its destination; the census proves that the catalogue
reaches every class it claims and that the zlib-written streams of tests/inflate_cases.py do not; and
tests/deflate_streams_check.c, compiled and run, does the same on exactly sized buffers with 2,000 mutated copies on top."""
import ctypes as C
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import deflate_streams as ds
import inflate_cases as ic
from test_inflate_plan import _check_records

from aggfly_amd import codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aggfly_amd", "csrc")
FILL = ds.FILL
PBLOCK = np.dtype([("out_pos", "<i8"), ("lit_off", "<i8"), ("seq_off", "<i8"), ("stream", "<i4"), ("nseq", "<i4"), ("lit_size", "<i4"),
                   ("dsize", "<i4")])                        # afi_pblock of inflate_passes.h


@pytest.fixture(scope="module")
def valid():
    """[(name, stream, the bytes its description means)] of the catalogue and the 300 fuzzed streams, built once."""
    cat = ds.catalogue()
    fz = ds.fuzz(ds.FUZZ_COUNT, ds.FUZZ_SEED)
    assert len(fz) == 300
    streams = [(n, ds.build(d), ds.expand(d)) for n, d in [(n, d) for n, _, d in cat] + fz]
    return streams, len(cat)


def _plan(streams, sizes, typesize=1):
    base, co, cs, oo, nout = ds.layout(streams, sizes)
    st = np.zeros(len(streams) + 1, dtype=codec.INFLATE_STREAM)
    sh = np.zeros(len(streams) + 1, dtype=codec.SHUFFLE_BLOCK)
    p = codec.inflate_plan(base, co, cs, oo, np.asarray(sizes, dtype=np.int64), st, sh, typesize=typesize, strict=False)
    return base, co, cs, oo, nout, st, sh, p


def _pblock_offset(p):
    """afi_layout of inflate_passes.h: where the pseudo-block records lie in the scratch."""
    al = lambda v: (v + 255) & ~255                          # noqa: E731
    at = al(p.n_streams * 5376)
    at = al(at + p.dec_bytes)
    return al(at + p.n_seqs * 12)


def _emulate(streams, sizes, typesize=1):
    """-> (plan, the whole output buffer, out_off, errors, the pseudo-block records the front end wrote)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    base, co, cs, oo, nout, st, sh, p = _plan(streams, sizes, typesize)
    assert (p.results == sizes).all()
    assert co[0] == 0 and co[-1] + cs[-1] == base.size and (len(streams) < 20 or (co % 2 == 1).any())      # flush at both ends, odd addresses
    _check_records(base, co, cs, oo, nout, st, sh, p, sizes, typesize)
    out = np.full(nout, FILL, dtype=np.uint8)
    scratch = np.zeros(p.scratch_bytes(), dtype=np.uint8)
    err, rounds = C.c_int32(0), C.c_int32(0)
    codec.load().afcodec_inflate_emulate(base.ctypes.data, base.nbytes, st.ctypes.data, p.n_streams, sh.ctypes.data, p.n_shuf, p.n_pblocks,
                                         p.n_seqs, p.n_pieces, p.dec_bytes, p.tmp_bytes, scratch.ctypes.data, out.ctypes.data,
                                         C.byref(err), C.byref(rounds))
    o = _pblock_offset(p)
    pb = scratch[o:o + p.n_pblocks * PBLOCK.itemsize].view(PBLOCK).copy()
    return p, out, oo, int(err.value), pb, st


def _expected(nout, oo, raws):
    want = np.full(nout, FILL, dtype=np.uint8)
    for o, r in zip(oo, raws):
        want[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    return want


def test_catalogue_names_every_case():
    cat = ds.catalogue()
    names = [n for n, _, _ in cat]
    assert len(set(names)) == len(names) >= 85 and all(why for _, why, _ in cat)
    assert set(ds.LAUNCH_GEOMETRY + ds.JUMP_BOUND + ds.MULTI_PBLOCK) <= set(names)
    total = sum(len(ds.expand(d)) for _, _, d in cat)
    assert total < 4 << 20, total                            # a few MB decoded


def test_zlib_and_the_strict_decoder_read_what_the_descriptions_mean(valid):
    """zlib is the reference; `expand` never decodes; the strict decoder agrees with both."""
    streams, _ = valid
    for name, s, want in streams:
        assert zlib.decompress(s) == want, name
        info = {}
        got, _ = ds.strict_decode(s, info)
        assert got == want, name
        d = zlib.decompressobj()                             # what lies behind the trailer is left over, as the passes leave it
        assert d.decompress(s) == want and d.eof and d.unused_data == info["unused"], name
    tails = [n for n, s, _ in streams if ("trailing-bytes",) in ds.strict_decode(s)[1]]
    assert len(tails) >= 2


def test_strict_decoder_refuses_what_zlib_refuses(valid):
    """On the 2,000 mutated copies that the stand-alone checker gets: the strict decoder takes exactly the streams zlib takes, to the
    same bytes."""
    streams, _ = valid
    taken = 0
    for i, (s, _) in enumerate(ds.mutated([(s, len(r)) for _, s, r in streams], ds.MUTATED_COUNT, 4)):
        try:
            want = zlib.decompress(s)
        except zlib.error:
            want = None
        try:
            got = ds.strict_decode(s)[0]
        except ds.Invalid:
            got = None
        assert got == want, i
        taken += want is not None
    assert 0 < taken < ds.MUTATED_COUNT // 4


@pytest.mark.parametrize("which", ["catalogue", "fuzz"])
def test_planner_takes_every_stream_and_the_passes_rebuild_the_whole_buffer(valid, which):
    streams, ncat = valid
    streams = streams[:ncat] if which == "catalogue" else streams[ncat:]
    raws = [r for _, _, r in streams]
    p, out, oo, errors, pb, st = _emulate([s for _, s, _ in streams], [len(r) for r in raws])
    assert errors == 0
    want = _expected(out.size, oo, raws)
    if not np.array_equal(out, want):
        bad = [n for (n, _, r), o in zip(streams, oo) if out[o:o + len(r)].tobytes() != r]
        raise AssertionError(("streams that differ", bad[:10], "canaries intact", bool((out[want == FILL] == FILL).all())))
    # the pseudo-blocks: what the rule of inflate_passes.h gives, none above AFZ_BLOCK_MAX, none but a stream's last below AFI_PBLOCK_MIN
    for (name, s, _), rec in zip(streams, st[:p.n_streams]):
        info = {}
        ds.strict_decode(s, info)
        got = [int(x) for x in pb[int(rec["first_block"]):int(rec["first_block"] + rec["n_blocks"])]["dsize"]]
        model = info["pblocks"]
        assert len(model) <= len(got), name
        assert got == model + [0] * (len(got) - len(model)), (name, got, model)
        assert max(got) <= ds.BLOCK_MAX and all(x >= ds.PBLOCK_MIN for x in model[:-1]), (name, got)


def test_every_stream_alone_in_its_batch(valid):
    streams, _ = valid
    for name, s, want in streams:
        p, out, oo, errors, _, _ = _emulate([s], [len(want)])
        assert errors == 0, name
        assert np.array_equal(out, _expected(out.size, oo, [want])), name


@pytest.mark.parametrize("typesize", [2, 4])
def test_multi_pseudo_block_streams_through_the_shuffle_scratch(valid, typesize):
    streams, _ = valid
    raws = [next(r for n, _, r in streams if n == name) for name in ds.MULTI_PBLOCK]
    again = [ds.build(ds.restore(ic.shuffle(r, typesize))) for r in raws]
    for s, r in zip(again, raws):
        assert zlib.decompress(s) == ic.shuffle(r, typesize)
    p, out, oo, errors, _, _ = _emulate(again, [len(r) for r in raws], typesize)
    assert errors == 0 and p.n_shuf == 2 and p.n_pblocks >= 4
    assert np.array_equal(out, _expected(out.size, oo, raws))


def test_census_reaches_every_class_and_the_zlib_written_streams_do_not(valid):
    streams, ncat = valid
    seen = set()
    for name, s, _ in streams[:ncat]:
        seen |= ds.strict_decode(s)[1]
    missing = set(ds.CLASSES) - seen
    assert not missing, sorted(map(str, missing))
    assert len(set(ds.CLASSES)) == len(ds.CLASSES)
    # "distances below the length, several of them"
    overlapping = [n for n, s, _ in streams[:ncat] if ("match", "overlap") in ds.strict_decode(s)[1]]
    assert len(overlapping) >= 5
    old = set()
    for name, s, raw in ic.good_streams():
        got, cls = ds.strict_decode(s)
        assert got == raw, name
        old |= cls
    old_missing = set(ds.CLASSES) - old
    print("census: %d classes; the catalogue (%d streams) misses %d, the zlib-written streams miss %d" % (len(ds.CLASSES), ncat, len(missing), len(old_missing)))
    print("not reached by the zlib-written streams:", sorted(map(str, old_missing)))
    assert old_missing
    # what the census of the zlib-written set found missing, named
    assert {("ll_len", 15), ("d_len", 12), ("d_len", 15), ("hdist", 1), ("dtable", "none-literals-only"), ("dtable", "one-1bit-used"),
            ("ltable", "eob-only"), ("len258", 284), ("tables", "fixed-after-dynamic-after-fixed"), ("stored_pad", 1), ("stored_pad", 7),
            ("stored_len", 65535), ("cut", "match-closes-at", ds.PBLOCK_MIN), ("hclen", 5), ("hclen", 13), ("hclen", 19)} <= old_missing


def test_damaged_streams_are_refused_once_and_inside_their_destination(valid):
    streams, _ = valid
    before = next((s, r) for n, s, r in streams if n == "stored-len-1")
    after = next((s, r) for n, s, r in streams if n == "one-distance-code-of-one-bit")
    dam = ds.damaged()
    assert len({d[0] for d in dam}) == len(dam) >= 40 and sum(d[5] is not None for d in dam) == 4
    src = open(os.path.join(CSRC, "inflate_passes.h")).read()
    for name, text, s, n, zlib_refuses, left in dam:
        assert text in src, (name, "the text that refuses it is no longer in inflate_passes.h")
        if zlib_refuses:
            with pytest.raises(zlib.error):
                zlib.decompress(s)
            with pytest.raises(ds.Invalid):
                ds.strict_decode(s)
        else:                                                # a valid stream of another size than planned
            assert len(zlib.decompress(s)) in (n - 1, n + 1) and len(ds.strict_decode(s)[0]) in (n - 1, n + 1), name
        p, out, oo, errors, _, _ = _emulate([s], [n])       # alone (the planner takes it: `_emulate` asserts the results)
        assert errors == 1, name
        assert np.array_equal(out, _expected(out.size, oo, [left or b""])), name
        # between two valid streams: a wrong accept of a distance past the stream's first byte would copy the neighbour's bytes
        sizes = [len(before[1]), n, len(after[1])]
        p, out, oo, errors, _, _ = _emulate([before[0], s, after[0]], sizes)
        assert errors == 1, name
        assert np.array_equal(out, _expected(out.size, oo, [before[1], left or b"", after[1]])), name


def test_the_stand_alone_checker_passes(valid, tmp_path):
    """tests/deflate_streams_check.c with blosc1.c, compiled plainly: catalogue, fuzz, damaged and 2,000 mutated streams, each alone
    in buffers of exactly its size."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    streams, _ = valid
    data = str(tmp_path / "streams.bin")
    n = ds.write_check_file(data, streams)
    assert n == len(streams) + len(ds.damaged()) + ds.MUTATED_COUNT
    exe = str(tmp_path / "deflate_streams_check")
    subprocess.run([cc, "-O1", "-fopenmp", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "deflate_streams_check.c"),
                    os.path.join(CSRC, "blosc1.c"), "-o", exe, "-lz", "-ldl"], check=True)
    out = subprocess.run([exe, data], capture_output=True, text=True)
    assert out.returncode == 0 and "deflate_streams_check: 0 failures" in out.stdout, out.stdout + out.stderr
