"""The Zstandard route (`afcodec_zstd_plan` in blosc1.c, the seven passes of zstd_passes.h run on the host by `afcodec_zstd_emulate`)
held to the hand-built frames of tests/zstd_frames.py: every frame of the catalogue and 300 fuzzed ones mean to the strict RFC 8878
decoder and to libzstd what their descriptions say, the planner takes them with records that match the decoder's view, and the
passes rebuild them bit for bit; every damaged frame is refused by the strict decoder and by the planner or the passes; the
census proves that catalogue and fuzz reach every class they claim; and tests/zstd_frames_check.c, compiled and run, does the
same on exactly sized buffers with 2,000 byte-mutated copies on top."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import zstd_frames as zs
from test_zstd_plan import _check_records

from aggfly_amd import codec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aggfly_amd", "csrc")
FILL = 0xAB

# Damaged frames that libzstd decodes although RFC 8878 does not allow them, each with the libzstd behaviour that explains it
# (lib/decompress/zstd_decompress_block.c).  This is no tolerance: the strict decoder and the route under test refuse every one.
LIBZSTD_LENIENT = {
    "rep0-minus-1-is-0-concrete": "ZSTD_decodeSequence: `offset = temp + !temp; /* 0 is not valid; input is corrupted; force offset to 1 */`",
    "rep0-minus-1-is-0-symbolic": "the same line of ZSTD_decodeSequence",
    "rep0-minus-1-is-0-symbolic-later-block": "the same line of ZSTD_decodeSequence",
    "match-overruns-128KiB": "ZSTD_execSequence bounds a match by the destination's capacity, not by Block_Maximum_Size",
    "left-over-bits-sequences": "ZSTD_decompressSequences_body checks only that the stream was not overrun (BIT_reloadDStream), not that it is used up",
    "left-over-byte-sequences": "the same check of ZSTD_decompressSequences_body",
    "reserved-bits-modes": "ZSTD_decodeSeqHeaders reads the three 2-bit modes and never looks at the two reserved bits",
}


@pytest.fixture(scope="module")
def valid():
    """[(name, frame bytes, the bytes its description means)] of the catalogue and the 300 fuzzed frames, built once."""
    cat = zs.catalogue()
    fz = zs.fuzz(zs.FUZZ_COUNT, zs.FUZZ_SEED)
    assert len(fz) == 300
    frames = [(n, zs.build(fd), zs.expand(fd)) for n, fd in [(n, fd) for n, _, fd in cat] + fz]
    return frames, len(cat)


def _plan(frames, sizes, cap_blocks=8192):
    base, co, cs, oo, nout = zs.layout(frames, sizes)
    fr, bl = np.zeros(len(frames) + 1, dtype=codec.ZSTD_FRAME), np.zeros(cap_blocks, dtype=codec.ZSTD_BLOCK)
    p = codec.zstd_plan(base, co, cs, oo, sizes, fr, bl, strict=False)
    return base, co, cs, oo, nout, fr, bl, p


def _canaries(out, oo, sizes):
    mask = np.ones(out.size, dtype=bool)
    for o, n in zip(oo, sizes):
        mask[o:o + n] = False
    return out[mask]


def test_catalogue_names_every_case_and_its_branch():
    cat = zs.catalogue()
    names = [n for n, _, _ in cat]
    assert len(set(names)) == len(names) >= 190 and all(why for _, why, _ in cat)
    assert set(zs.LAUNCH_GEOMETRY + zs.JUMP_BOUND) <= set(names)
    assert sum(n.startswith("modes-") for n in names) == 64


def test_strict_decoder_and_libzstd_read_what_the_descriptions_mean(valid):
    frames, _ = valid
    for name, fb, want in frames:
        assert zs.decode(fb) == want, name
        assert codec.zstd_decode(fb, len(want) + 8).tobytes() == want, name


@pytest.mark.parametrize("which", ["catalogue", "fuzz"])
def test_planner_takes_every_frame_and_the_passes_rebuild_it(valid, which):
    frames, ncat = valid
    frames = frames[:ncat] if which == "catalogue" else frames[ncat:]
    sizes = np.array([len(r) for _, _, r in frames], dtype=np.int64)
    base, co, cs, oo, nout, fr, bl, p = _plan([f for _, f, _ in frames], sizes)
    assert (p.results == sizes).all(), [frames[i][0] for i in np.nonzero(p.results != sizes)[0]]
    assert co[0] == 0 and co[-1] + cs[-1] == base.size                 # first frame at byte 0, last flush with the end
    _check_records(base, co, cs, oo, nout, fr, bl, p, sizes)
    for (name, fb, _), rec in zip(frames, fr[:p.n_frames]):            # the records against the strict decoder's view
        view = []
        zs.decode(fb, records=view)
        got = bl[int(rec["first_block"]):int(rec["first_block"] + rec["n_blocks"])]
        assert len(view) == len(got), name
        for v, k in zip(view, got):
            assert all(int(k[key]) == v[key] for key in ("btype", "lit_type", "lit_size", "n_streams", "nseq")), (name, v)
    out = np.full(nout, FILL, dtype=np.uint8)
    errors, rounds = codec.zstd_emulate(base, fr, bl, p, out)
    assert errors == 0
    for (name, _, want), o in zip(frames, oo):
        assert out[o:o + len(want)].tobytes() == want, name
    assert (_canaries(out, oo, sizes) == FILL).all()


@pytest.mark.parametrize("name", zs.LAUNCH_GEOMETRY + zs.JUMP_BOUND)
def test_frames_of_a_launch_geometry_alone_in_their_batch(valid, name):
    frames, _ = valid
    _, fb, want = next(x for x in frames if x[0] == name)
    base, co, cs, oo, nout, fr, bl, p = _plan([fb], [len(want)])
    out = np.full(nout, FILL, dtype=np.uint8)
    errors, rounds = codec.zstd_emulate(base, fr, bl, p, out)
    assert errors == 0 and out[oo[0]:oo[0] + len(want)].tobytes() == want and (_canaries(out, oo, [len(want)]) == FILL).all()
    if name == "workgroup-of-16-tables":
        assert (bl[:16]["lit_type"] == 2).all() and (bl[:16]["n_streams"] == 4).all() and bl[16]["huf_block"] == 15
    if name == "treeless-across-workgroups":
        assert bl[15]["lit_type"] == 2 and bl[16]["lit_type"] == 3 and bl[16]["huf_block"] == 15
    if name == "blocks-300-small":
        assert p.n_blocks == 300


def test_damaged_frames_are_refused(valid):
    frames, _ = valid
    neighbour = next((fb, want) for n, fb, want in frames if n == "block-raw")
    lenient = set()
    dam = zs.damaged()
    assert len({n for n, _, _, _ in dam}) == len(dam) >= 30
    for name, (src, text), fb, n in dam:
        assert text in open(os.path.join(CSRC, src)).read(), (name, "the text that refuses it is no longer in " + src)
        with pytest.raises(zs.Invalid):
            zs.decode(fb)
        try:
            codec.zstd_decode(fb, n + 64)
            lenient.add(name)
        except codec.CodecError:
            pass
        # a valid neighbour lies directly before it in the batch: a wrong accept of an offset past the frame's first byte
        # would copy the neighbour's bytes
        sizes = [len(neighbour[1]), n]
        base, co, cs, oo, nout, fr, bl, p = _plan([neighbour[0], fb], sizes)
        assert p.results[0] == sizes[0]
        out = np.full(nout, FILL, dtype=np.uint8)
        errors, _ = codec.zstd_emulate(base, fr, bl, p, out)
        assert out[oo[0]:oo[0] + sizes[0]].tobytes() == neighbour[1]
        assert (_canaries(out, oo, sizes) == FILL).all()
        if p.results[1] >= 0:
            assert errors == 1, name
        else:
            assert p.results[1] == -1, name                             # AFCODEC_E_FORMAT: malformed, not "decode on the host"
            assert errors == 0 and p.n_frames == 1
            assert (out[oo[1]:oo[1] + n] == FILL).all()
    print("libzstd", _libzstd_version(), "decodes these damaged frames:", sorted(lenient))
    assert lenient <= set(LIBZSTD_LENIENT), sorted(lenient - set(LIBZSTD_LENIENT))
    assert set(LIBZSTD_LENIENT) <= {n for n, _, _, _ in dam}


def _libzstd_version():
    import ctypes as C
    lib = C.CDLL("libzstd.so.1")
    lib.ZSTD_versionString.restype = C.c_char_p
    return lib.ZSTD_versionString().decode()


def test_census_reaches_every_class(valid):
    """By the strict decoder; the literal classes once more from the planner's block records."""
    frames, ncat = valid
    seen = {"catalogue": set(), "fuzz": set()}
    for i, (name, fb, _) in enumerate(frames):
        zs.decode(fb, census=seen["catalogue" if i < ncat else "fuzz"])
    assert not set(zs.CLASSES) - seen["catalogue"], sorted(map(str, set(zs.CLASSES) - seen["catalogue"]))
    missing = set(zs.CLASSES) - zs.NOT_BY_FUZZ - seen["fuzz"]
    assert not missing, sorted(map(str, missing))
    cat = seen["catalogue"]
    # the shapes named in the issue beyond the classes
    assert {("huf_symbols", 2), ("huf_symbols", 256), ("huf_depth", 11), ("huf_desc", "direct", "odd"), ("huf_desc", "direct", "even"),
            ("huf_desc", "fse", 5), ("huf_desc", "fse", 6)} <= cat
    assert {("code", "LL", c) for c in range(36)} | {("code", "ML", c) for c in range(53)} | {("code", "OF", c) for c in range(21)} <= cat
    assert {("fse_log", "LL", 5), ("fse_log", "OF", 5), ("fse_log", "ML", 5), ("fse_log", "LL", 9), ("fse_log", "OF", 8), ("fse_log", "ML", 9)} <= cat
    assert {("fse_less_than_one", t) for t in zs.TABLES} <= cat
    assert {("repeat_of", t, k) for t in zs.TABLES for k in ("pre", "rle", "fse")} <= cat
    assert {("frame", "single", 0, k) for k in (1, 2, 4, 8)} | {("frame", "window", 0, k) for k in (2, 4, 8)} | {("frame", "single", k, 1) for k in (1, 2, 4)} <= cat
    for part, lo, hi in (("catalogue", 0, ncat), ("fuzz", ncat, len(frames))):
        sub = frames[lo:hi]
        sizes = np.array([len(r) for _, _, r in sub], dtype=np.int64)
        *_, bl, p = _plan([f for _, f, _ in sub], sizes)
        k = bl[:p.n_blocks]
        k = k[k["btype"] == 2]
        got = {("lit", ("raw", "rle", "huf", "treeless")[int(t)], int(n)) for t, n in zip(k["lit_type"], k["n_streams"])}
        assert got == {c for c in seen[part] if c[0] == "lit"}
    print("census: %d classes; catalogue %d frames, fuzz %d frames" % (len(zs.CLASSES), ncat, len(frames) - ncat))


def test_ncount_writer_and_reader_agree():
    rng = np.random.default_rng(3)
    for _ in range(300):
        log = int(rng.integers(5, 10))
        hist = [int(x) for x in rng.integers(0, 6, size=int(rng.integers(2, 30))) * (rng.random(1) < 0.9)]
        if sum(1 for h in hist if h) < 2:
            continue
        norm = zs.normalise(hist, log)
        for j in rng.choice(len(norm), size=min(3, len(norm)), replace=False):   # some "less than 1" probabilities
            if norm[j] == 1:
                norm[j] = -1
        got, lg, used = zs.ncount_read(zs.ncount_write(norm, log) + b"\xff", 255, 9)
        assert (got, lg) == (norm, log) and used == len(zs.ncount_write(norm, log))


def test_the_stand_alone_checker_passes(valid, tmp_path):
    """tests/zstd_frames_check.c with blosc1.c, compiled plainly: catalogue, fuzz, damaged and 2,000 byte-mutated frames, each alone
    in buffers of exactly its size."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    frames, _ = valid
    data = str(tmp_path / "frames.bin")
    n = zs.write_check_file(data, frames)
    assert n == len(frames) + len(zs.damaged()) + zs.MUTATED_COUNT
    exe = str(tmp_path / "zstd_frames_check")
    subprocess.run([cc, "-O1", "-fopenmp", "-I", os.path.join(ROOT, "include"), "-I", CSRC, os.path.join(ROOT, "tests", "zstd_frames_check.c"),
                    os.path.join(CSRC, "blosc1.c"), "-o", exe, "-lz", "-ldl"], check=True)
    out = subprocess.run([exe, data], capture_output=True, text=True)
    assert out.returncode == 0 and "zstd_frames_check: 0 failures" in out.stdout, out.stdout + out.stderr
