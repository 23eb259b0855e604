"""The batches the poisoned- and stale-scratch tests run, built once from the existing case writers (tests/zstd_frames.py,
tests/deflate_streams.py, tests/inflate_cases.py) and shared by the host half (tests/test_poison_host.py: the emulations) and the
GPU half (tests/test_gpu_poison_codecs.py: the kernels).  A batch knows its planned records and the image its output buffer must
hold afterwards: the fill byte 0xAB, the bytes every good item means by its description, and what a damaged item leaves — nothing,
or for the four deflate streams with a wrong Adler-32 the decoded bytes (`deflate_streams.damaged`).  Batch "A" is the whole catalogue,
the fuzz and every damaged case of the writer between good ones; batch "B" a smaller selection of good items in another order."""
import functools
import zlib

import numpy as np

import deflate_streams as ds
import inflate_cases as ic
import zstd_frames as zs

from aggfly_amd import codec

FILL = 0xAB


class Batch:
    """base: the compressed bytes; records: the planner's two record arrays; plan; nout / want: the output buffer's size and the
    image it must hold; errors: the items the passes must count."""

    def __init__(self, name, base, records, plan, nout, want, errors):
        self.name, self.base, self.records, self.plan, self.nout, self.want, self.errors = name, base, records, plan, nout, want, errors
        self.want.setflags(write=False)


def _image(nout, oo, left):
    want = np.full(nout, FILL, dtype=np.uint8)
    for o, b in zip(oo, left):
        if b:
            want[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    return want


def _interleave(good, damaged):
    """good, damaged, good, damaged, ..., then the good ones that are left: -> [(item, is damaged)]."""
    out = []
    for i, g in enumerate(good):
        out.append((g, False))
        if i < len(damaged):
            out.append((damaged[i], True))
    assert len(good) > len(damaged)
    return out


@functools.lru_cache(maxsize=None)
def zstd_batches():
    cat = zs.catalogue()
    good = [(n, zs.build(fd), zs.expand(fd)) for n, fd in [(n, fd) for n, _, fd in cat] + zs.fuzz(zs.FUZZ_COUNT, zs.FUZZ_SEED)]
    dam = [(n, fb, size) for n, _, fb, size in zs.damaged()]
    a = [(f, len(r), r, False) for _, f, r in good]
    a = [x if not bad else (x[1], x[2], b"", True) for x, bad in _interleave(a, dam)]
    small = [(f, len(r), r, False) for _, f, r in good if len(r) < 70000]
    b = small[::-3]
    assert len(b) >= 100 and len(dam) >= 30
    return {"A": _zstd_batch("A", a), "B": _zstd_batch("B", b)}


def _zstd_batch(name, items):
    frames, sizes = [x[0] for x in items], np.array([x[1] for x in items], dtype=np.int64)
    base, co, cs, oo, nout = zs.layout(frames, sizes)
    fr, bl = np.zeros(len(frames) + 1, dtype=codec.ZSTD_FRAME), np.zeros(16384, dtype=codec.ZSTD_BLOCK)
    p = codec.zstd_plan(base, co, cs, oo, sizes, fr, bl, strict=False)
    bad = np.array([x[3] for x in items])
    assert (p.results[~bad] == sizes[~bad]).all()
    return Batch("zstd-" + name, base, (fr, bl), p, nout, _image(nout, oo, [x[2] for x in items]), int((p.results[bad] >= 0).sum()))


@functools.lru_cache(maxsize=None)
def inflate_batches():
    """The catalogue and the fuzz of deflate_streams.py, `inflate_cases.good_streams`, four chunks written through the shuffle filter
    (element sizes 2, 4, 4, 8: they decode into the scratch and are unshuffled from there, n_shuf > 0) and every damaged stream."""
    cat = ds.catalogue()
    good = [(ds.build(d), r, 1) for d, r in [(d, ds.expand(d)) for _, _, d in cat] + [(d, ds.expand(d)) for _, d in ds.fuzz(ds.FUZZ_COUNT, ds.FUZZ_SEED)]]
    good += [(s, r, 1) for _, s, r in ic.good_streams()]
    cube = ic.CUBE.tobytes()
    good += [(zlib.compress(ic.shuffle(r, ts), 4), r, ts) for r, ts in ((cube[:50002], 2), (cube, 4), (cube[:50001], 4), (cube[:120008], 8))]
    dam = [(s, n, left) for _, _, s, n, _, left in ds.damaged()]
    a = [(s, len(r), r, ts, False) for s, r, ts in good]
    a = [x if not bad else (x[0], x[1], x[2] or b"", 1, True) for x, bad in _interleave(a, dam)]
    small = [(s, len(r), r, ts, False) for s, r, ts in good if len(r) < 70000 or ts > 1]
    b = small[::-3]
    assert len(b) >= 100 and len(dam) >= 40 and sum(x[3] > 1 for x in b) >= 1
    return {"A": _inflate_batch("A", a), "B": _inflate_batch("B", b)}


def _inflate_batch(name, items):
    streams, sizes = [x[0] for x in items], np.array([x[1] for x in items], dtype=np.int64)
    base, co, cs, oo, nout = ds.layout(streams, sizes)
    st = np.zeros(len(streams) + 1, dtype=codec.INFLATE_STREAM)
    sh = np.zeros(len(streams) + 1, dtype=codec.SHUFFLE_BLOCK)
    p = codec.inflate_plan(base, co, cs, oo, sizes, st, sh, typesize=np.array([x[3] for x in items], dtype=np.int32), strict=False)
    bad = np.array([x[4] for x in items])
    assert (p.results[~bad] == sizes[~bad]).all() and p.n_shuf > 0
    return Batch("inflate-" + name, base, (st, sh), p, nout, _image(nout, oo, [x[2] for x in items]), int((p.results[bad] >= 0).sum()))


def emulate(kind, batch, scratch=None):
    """-> (output image, errors, rounds) of the host emulation of ``kind`` ("zstd" / "inflate") over ``batch``."""
    out = np.full(batch.nout, FILL, dtype=np.uint8)
    fn = codec.zstd_emulate if kind == "zstd" else codec.inflate_emulate
    errors, rounds = fn(batch.base, *batch.records, batch.plan, out, scratch=scratch)
    return out, errors, rounds
