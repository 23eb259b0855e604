"""ctypes binding of ``libaggfly_codec.so`` (aggfly_amd/csrc/blosc1.c): the host-side chunk codecs
of the ingestion path — Blosc-1 containers (blosclz / lz4 / lz4hc / zlib / zstd, byte- and
bit-shuffle), plain Zstandard frames, the planners of the decode-in-HBM routes, and a Blosc-1 encoder (LZ4 / Zstandard) for the writer
side.

The reference decodes chunks through numcodecs inside its dask graph
(`aggfly/dataset/dataset.py:697-728`); here every chunk is decoded by native code on a host thread
(ctypes drops the GIL), or a whole slab of chunks at once on an OpenMP team.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libaggfly_codec.so")
_lib = None

CODEC_NAMES = {0: "blosclz", 1: "lz4", 2: "snappy", 3: "zlib", 4: "zstd"}


class CodecError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CodecError(f"{LIB_PATH} is missing: build it with `make -C aggfly_amd/csrc codec` "
                             "or `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(LIB_PATH)
        lib.afcodec_last_error.restype = C.c_char_p
        lib.afcodec_have.argtypes = [C.c_int]
        lib.afcodec_blosc_info.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.afcodec_blosc_decode.restype = C.c_int64
        lib.afcodec_blosc_decode.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        lib.afcodec_blosc_decode_mt.restype = C.c_int64
        lib.afcodec_blosc_decode_mt.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int]
        lib.afcodec_blosc_decode_many.argtypes = [C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64)]
        lib.afcodec_blosc_decode_files.argtypes = [C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                                   C.c_int, C.POINTER(C.c_int64)]
        lib.afcodec_decode_files.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                             C.c_int, C.POINTER(C.c_int64)]
        lib.afcodec_decode_ranges.argtypes = [C.c_int, C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                              C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64)]
        lib.afcodec_blosc_bound.restype = C.c_int64
        lib.afcodec_blosc_bound.argtypes = [C.c_int64, C.c_int64]
        lib.afcodec_blosc_encode_lz4.restype = C.c_int64
        lib.afcodec_blosc_encode_lz4.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64]
        lib.afcodec_blosc_encode.restype = C.c_int64
        lib.afcodec_blosc_encode.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64]
        lib.afcodec_lz4_decode.restype = C.c_int64
        lib.afcodec_lz4_decode.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        lib.afcodec_zstd_decode.restype = C.c_int64
        lib.afcodec_zstd_decode.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        lib.afcodec_zstd_bound.restype = C.c_int64
        lib.afcodec_zstd_bound.argtypes = [C.c_int64]
        lib.afcodec_zstd_encode.restype = C.c_int64
        lib.afcodec_zstd_encode.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64]
        lib.afcodec_blosc_lz4_plan.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                               C.POINTER(C.c_int32), C.c_void_p]
        lib.afcodec_blosc_plan.argtypes = ([C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_void_p, C.c_int64, C.POINTER(C.c_int64)] * 5
                                           + [C.POINTER(C.c_int64)] * 4 + [C.POINTER(C.c_int32), C.c_void_p])
        lib.afcodec_zstd_plan.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                          C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p]
        lib.afcodec_zstd_scratch_bytes.restype = C.c_int64
        lib.afcodec_zstd_scratch_bytes.argtypes = [C.c_int64] * 5
        lib.afcodec_zstd_emulate.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                             C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.afcodec_inflate_plan.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                             C.POINTER(C.c_int64), C.c_void_p, C.c_int64] + [C.POINTER(C.c_int64)] * 6 + [C.c_void_p]
        lib.afcodec_inflate_scratch_bytes.restype = C.c_int64
        lib.afcodec_inflate_scratch_bytes.argtypes = [C.c_int64] * 6
        lib.afcodec_inflate_emulate.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_int64] * 6 + [
            C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.afcodec_lz4_encode_emulate.restype = C.c_int64
        lib.afcodec_lz4_encode_emulate.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
        lib.afcodec_blosc_encode_plan.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_int64,
                                                  C.POINTER(C.c_int64), C.c_void_p]
        lib.afcodec_zstd_encode_block_emulate.restype = C.c_int64
        lib.afcodec_zstd_encode_block_emulate.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64]
        lib.afcodec_zstd_encode_scratch_bytes.restype = C.c_int64
        lib.afcodec_zstd_encode_scratch_bytes.argtypes = [C.c_int64]
        lib.afcodec_blosc_zstd_encode_plan.argtypes = lib.afcodec_blosc_encode_plan.argtypes
        lib.afcodec_read_packed.argtypes = [C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_int64,
                                            C.c_int64, C.c_int, C.c_void_p, C.c_void_p]
        lib.afcodec_aec_decode.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        lib.afcodec_lzw_decode_ranges.argtypes = [C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64)]
        _lib = lib
    return _lib


EXPORTS = ("afcodec_last_error", "afcodec_have", "afcodec_blosc_info", "afcodec_blosc_decode", "afcodec_blosc_decode_mt", "afcodec_blosc_decode_many",
           "afcodec_blosc_decode_files", "afcodec_decode_files", "afcodec_decode_ranges",
           "afcodec_blosc_bound", "afcodec_blosc_encode_lz4", "afcodec_zstd_decode", "afcodec_zstd_bound", "afcodec_zstd_encode", "afcodec_lz4_decode", "afcodec_blosc_lz4_plan", "afcodec_read_packed",
           "afcodec_zstd_plan", "afcodec_zstd_scratch_bytes", "afcodec_zstd_emulate",
           "afcodec_inflate_plan", "afcodec_inflate_scratch_bytes", "afcodec_inflate_emulate",
           "afcodec_blosc_plan", "afcodec_blosc_encode", "afcodec_lz4_encode_emulate", "afcodec_blosc_encode_plan",
           "afcodec_zstd_encode_block_emulate", "afcodec_zstd_encode_scratch_bytes", "afcodec_blosc_zstd_encode_plan", "afcodec_aec_decode",
           "afcodec_lzw_decode_ranges")


def _err(lib, what):
    return CodecError(f"{what}: {lib.afcodec_last_error().decode()}")


def _addr(buf):
    """Address of a bytes-like object without copying it."""
    if isinstance(buf, np.ndarray):
        return buf.ctypes.data, buf.nbytes
    mv = memoryview(buf)
    if mv.readonly:
        return C.cast(C.c_char_p(bytes(buf) if not isinstance(buf, bytes) else buf), C.c_void_p).value, mv.nbytes
    return C.addressof(C.c_char.from_buffer(mv)), mv.nbytes


def blosc_info(buf) -> dict:
    lib = load()
    p, n = _addr(buf)
    nb, bs, ts, fl = C.c_int64(), C.c_int64(), C.c_int32(), C.c_int32()
    if lib.afcodec_blosc_info(p, n, C.byref(nb), C.byref(bs), C.byref(ts), C.byref(fl)):
        raise _err(lib, "blosc_info")
    f = fl.value
    return {"nbytes": nb.value, "blocksize": bs.value, "typesize": ts.value, "flags": f, "codec": CODEC_NAMES.get((f >> 5) & 7, "?"),
            "shuffle": 1 if f & 1 else (2 if f & 4 else 0), "stored": bool(f & 2), "split": not (f & 0x10)}


def blosc_decode(buf, out: np.ndarray | None = None, threads: int = 1) -> np.ndarray:
    """Decode one Blosc-1 chunk; ``out`` (C-contiguous, >= nbytes) is filled in place when given;
    ``threads`` > 1 spreads the chunk's blocks over an OpenMP team (for large chunks)."""
    lib = load()
    p, n = _addr(buf)
    if out is None:
        out = np.empty(blosc_info(buf)["nbytes"], dtype=np.uint8)
    if not out.flags.c_contiguous:
        raise ValueError("blosc_decode: out must be C-contiguous")
    if threads > 1:
        r = lib.afcodec_blosc_decode_mt(p, n, out.ctypes.data, out.nbytes, int(threads))
    else:
        r = lib.afcodec_blosc_decode(p, n, out.ctypes.data, out.nbytes)
    if r < 0:
        raise _err(lib, "blosc_decode")
    return out


def blosc_decode_many(bufs, outs, threads: int = 8):
    """Decode chunks ``bufs[i]`` into the C-contiguous arrays ``outs[i]`` on an OpenMP team."""
    lib = load()
    n = len(bufs)
    keep = [b if isinstance(b, (bytes, np.ndarray)) else bytes(b) for b in bufs]
    addrs = [_addr(b) for b in keep]
    cp = (C.c_void_p * n)(*[a for a, _ in addrs])
    cs = (C.c_int64 * n)(*[s for _, s in addrs])
    dp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    ds = (C.c_int64 * n)(*[o.nbytes for o in outs])
    res = (C.c_int64 * n)()
    if lib.afcodec_blosc_decode_many(n, cp, cs, dp, ds, int(threads), res):
        bad = [i for i in range(n) if res[i] < 0]
        raise CodecError(f"blosc_decode_many: chunks {bad[:8]} failed: {lib.afcodec_last_error().decode()}")
    return [int(res[i]) for i in range(n)]


KIND = {"raw": 0, "blosc": 1, "zstd": 2, "zlib": 3, "gzip": 3, "lz4": 4}


def _require_full(what, names, outs, res):
    """A present chunk must fill its destination exactly: a Blosc header announcing fewer bytes, a truncated raw file or
    a zstd / zlib frame that decodes short would otherwise leave the rest of a (re-used, page-locked) staging slot to
    travel to HBM as data.  zarr / numcodecs raise on such chunks (`aggfly/dataset/dataset.py:697-728` reads through them)."""
    short = [(names[i], int(res[i]), outs[i].nbytes) for i in range(len(outs)) if res[i] != -100 and int(res[i]) != outs[i].nbytes]
    if short:
        nm, got, want = short[0]
        raise CodecError(f"{what}: chunk {nm} decoded to {got} bytes, expected {want}"
                         + (f" (and {len(short) - 1} more)" if len(short) > 1 else ""))


def decode_files(kind: str, paths, outs, threads: int = 8, exact: bool = True):
    """Read and decode the chunk files ``paths[i]`` (all of codec ``kind``: raw / blosc / zstd / zlib /
    gzip) into ``outs[i]`` on an OpenMP team.  -> list of decoded sizes; -100 marks a missing file (the
    caller applies the fill value).  ``exact``: a present chunk must decode to exactly ``outs[i].nbytes``."""
    lib = load()
    n = len(paths)
    pp = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
    dp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    ds = (C.c_int64 * n)(*[o.nbytes for o in outs])
    res = (C.c_int64 * n)()
    if lib.afcodec_decode_files(KIND[kind], n, pp, dp, ds, int(threads), res):
        bad = [paths[i] for i in range(n) if res[i] < 0 and res[i] != -100]
        raise CodecError(f"decode_files({kind}): {bad[:4]} failed: {lib.afcodec_last_error().decode()}")
    if exact:
        _require_full(f"decode_files({kind})", paths, outs, res)
    return [int(res[i]) for i in range(n)]


def decode_ranges(kind: str, locators, outs, threads: int = 8, exact: bool = True):
    """Like `decode_files` for ``locators[i] = (path, offset, nbytes)`` — nbytes < 0 = the whole file, None =
    an absent chunk (reported as -100 without touching the disk).  ``kind`` may be a pair ``(codec, element_size)``:
    the codec's output is then byte-unshuffled (HDF5 shuffle + deflate chunks).  ``exact`` as in `decode_files`."""
    lib = load()
    n = len(locators)
    pp = (C.c_char_p * n)(*[os.fsencode(l[0]) if l is not None else b"" for l in locators])
    offs = (C.c_int64 * n)(*[int(l[1]) if l is not None else 0 for l in locators])
    lens = (C.c_int64 * n)(*[int(l[2]) if l is not None else -1 for l in locators])
    dp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    ds = (C.c_int64 * n)(*[o.nbytes for o in outs])
    res = (C.c_int64 * n)()
    code = KIND[kind] if isinstance(kind, str) else KIND[kind[0]] + 16 * int(kind[1])      # (codec, element size): + byte unshuffle
    if lib.afcodec_decode_ranges(code, n, pp, offs, lens, dp, ds, int(threads), res):
        bad = [locators[i] for i in range(n) if res[i] < 0 and res[i] != -100]
        raise CodecError(f"decode_ranges({kind}): {bad[:4]} failed: {lib.afcodec_last_error().decode()}")
    if exact:
        _require_full(f"decode_ranges({kind})", locators, outs, res)
    return [int(res[i]) for i in range(n)]


def read_packed(locators, dst: np.ndarray, align: int = 64, threads: int = 8):
    """`afcodec_read_packed`: the byte ranges ``locators[i] = (path, offset, nbytes)`` (nbytes < 0: the whole file; None: an
    absent chunk) read back to back into the uint8 array ``dst`` -> (offsets int64[n + 1], sizes int64[n], -100 = missing).
    The files are neither stat'ed nor opened from Python."""
    lib = load()
    n = len(locators)
    pp = (C.c_char_p * n)(*[os.fsencode(l[0]) if l is not None else b"" for l in locators])
    offs = (C.c_int64 * n)(*[int(l[1]) if l is not None else 0 for l in locators])
    lens = (C.c_int64 * n)(*[int(l[2]) if l is not None else -1 for l in locators])
    out_off = np.zeros(n + 1, dtype=np.int64)
    res = np.zeros(n, dtype=np.int64)
    if lib.afcodec_read_packed(n, pp, offs, lens, dst.ctypes.data, dst.nbytes, int(align), int(threads), out_off.ctypes.data, res.ctypes.data):
        bad = [locators[i] for i in range(n) if res[i] < 0 and res[i] != -100]
        raise CodecError(f"read_packed: {bad[:4]} failed: {lib.afcodec_last_error().decode()}")
    return out_off, res


def blosc_decode_files(paths, outs, threads: int = 8):
    return decode_files("blosc", paths, outs, threads)


BLOSC_CNAME = {"lz4": 1, "zstd": 4}


def blosc_encode(data, typesize: int, shuffle: bool = True, blocksize: int = 0, cname: str = "lz4", bitshuffle: bool = False,
                 level: int = 3) -> bytes:
    """Blosc-1 chunk of ``data`` (bytes-like or array) with LZ4 or Zstandard (``cname``, ``level``: libzstd's) streams: what
    numcodecs' ``Blosc(cname=...)`` reads.  ``bitshuffle``: Blosc's bit shuffle (``shuffle=2``) in place of the byte shuffle."""
    lib = load()
    arr = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)
    cap = lib.afcodec_blosc_bound(arr.nbytes, blocksize)
    dst = np.empty(cap, dtype=np.uint8)
    r = lib.afcodec_blosc_encode(arr.ctypes.data, arr.nbytes, int(typesize), 2 if bitshuffle else (1 if shuffle else 0), BLOSC_CNAME[cname],
                                 int(level), int(blocksize), dst.ctypes.data, cap)
    if r < 0:
        raise _err(lib, "blosc_encode")
    return dst[:r].tobytes()


def zstd_decode(buf, nbytes: int, out: np.ndarray | None = None) -> np.ndarray:
    """Decode one Zstandard frame of at most ``nbytes`` decoded bytes."""
    lib = load()
    p, n = _addr(buf)
    if out is None:
        out = np.empty(nbytes, dtype=np.uint8)
    r = lib.afcodec_zstd_decode(p, n, out.ctypes.data, out.nbytes)
    if r < 0:
        raise _err(lib, "zstd_decode")
    return out[:r] if r != out.nbytes and out.ndim == 1 else out


def zstd_encode(data, level: int = 3) -> bytes:
    lib = load()
    arr = np.ascontiguousarray(data) if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)
    cap = lib.afcodec_zstd_bound(arr.nbytes)
    dst = np.empty(cap, dtype=np.uint8)
    r = lib.afcodec_zstd_encode(arr.ctypes.data, arr.nbytes, int(level), dst.ctypes.data, cap)
    if r < 0:
        raise _err(lib, "zstd_encode")
    return dst[:r].tobytes()


def lz4_decode(buf, nbytes: int, out: np.ndarray | None = None) -> np.ndarray:
    """numcodecs LZ4 chunk (int32 size header + raw block) of at most ``nbytes`` decoded bytes."""
    lib = load()
    p, n = _addr(buf)
    if out is None:
        out = np.empty(nbytes, dtype=np.uint8)
    r = lib.afcodec_lz4_decode(p, n, out.ctypes.data, out.nbytes)
    if r < 0:
        raise _err(lib, "lz4_decode")
    return out[:r] if r != out.nbytes and out.ndim == 1 else out


# record layouts shared with libaggfly_hip (include/aggfly_hip.h: afhip_lz4_stream, afhip_shuffle_block)
LZ4_STREAM = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("csize", "<i4"), ("dsize", "<i4"), ("to_out", "<i4"), ("pad", "<i4")])
SHUFFLE_BLOCK = np.dtype([("tmp_off", "<i8"), ("out_off", "<i8"), ("bsize", "<i4"), ("typesize", "<i4")])
E_UNSUPPORTED = -2


class PlanCapacityError(CodecError):
    """`blosc_lz4_plan`: the chunks need more stream / block records than the lists passed in hold (their geometry differs
    from the one the lists were sized for)."""


def blosc_lz4_plan(base: np.ndarray, comp_off, comp_size, out_off, out_size, streams: np.ndarray, blocks: np.ndarray):
    """Plan the GPU-side decode of Blosc-1 chunks that sit in ``base`` (uint8; chunk i = ``comp_size[i]`` bytes at
    ``comp_off[i]``): fills ``streams`` (dtype `LZ4_STREAM`) and ``blocks`` (dtype `SHUFFLE_BLOCK`) for
    `hip.lz4_decode_streams` / `hip.unshuffle_blocks`.  -> (n_streams, n_blocks, tmp_bytes, max_dsize, results);
    ``results[i]`` = decoded size, or `E_UNSUPPORTED` for a chunk the GPU route does not take (decode it on the host);
    malformed containers raise `CodecError`."""
    lib = load()
    n = len(comp_off)
    co, cs, oo, osz = (np.ascontiguousarray(a, dtype=np.int64) for a in (comp_off, comp_size, out_off, out_size))
    res = np.zeros(n, dtype=np.int64)
    ns, nb, tmp, maxd = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    assert streams.dtype == LZ4_STREAM and blocks.dtype == SHUFFLE_BLOCK and base.dtype == np.uint8
    rc = lib.afcodec_blosc_lz4_plan(base.ctypes.data, n, co.ctypes.data, cs.ctypes.data, oo.ctypes.data, osz.ctypes.data,
                                    streams.ctypes.data, len(streams), C.byref(ns), blocks.ctypes.data, len(blocks), C.byref(nb),
                                    C.byref(tmp), C.byref(maxd), res.ctypes.data)
    bad = [int(i) for i in np.nonzero((res < 0) & (res != E_UNSUPPORTED))[0]]
    if bad or (rc and rc != E_UNSUPPORTED):
        msg = lib.afcodec_last_error().decode()
        if not bad and "list too small" in msg:       # more streams / blocks than the caller's record lists hold: not damage
            raise PlanCapacityError(f"blosc_lz4_plan: {msg}")
        raise CodecError(f"blosc_lz4_plan: chunks {bad[:8]} are malformed: {msg}")
    return int(ns.value), int(nb.value), int(tmp.value), int(maxd.value), res


# ---- the write side in HBM: `hip.shuffle_blocks`, `hip.lz4_encode_streams`, `hip.copy_ranges` (io.dataset_to_zarr, encode="gpu") ----
COPY_RANGE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("n", "<i8")])       # == afhip_copy_range


def lz4_encode_emulate(data) -> bytes:
    """`afcodec_lz4_encode_emulate`: the LZ4 block encoder of `lz4_encode_pass.h` as `hip.lz4_encode_streams` runs it, on the host.
    -> the stream; as long as the input = stored (the raw bytes)."""
    lib = load()
    arr = np.ascontiguousarray(data).view(np.uint8).reshape(-1) if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)
    dst = np.empty(max(arr.nbytes, 1), dtype=np.uint8)
    r = lib.afcodec_lz4_encode_emulate(arr.ctypes.data, arr.nbytes, dst.ctypes.data, arr.nbytes)
    if r < 0:
        raise _err(lib, "lz4_encode_emulate")
    return dst[:r].tobytes()


def _put_u32(buf: np.ndarray, offs, vals):
    """Little-endian uint32 ``vals`` at the (unaligned) byte offsets ``offs`` of the uint8 array ``buf``."""
    offs = np.asarray(offs, dtype=np.int64).reshape(-1)
    buf[offs[:, None] + np.arange(4)] = np.asarray(vals).astype("<u4").reshape(-1).view(np.uint8).reshape(-1, 4)


class BloscEncodePlan:
    """`afcodec_blosc_encode_plan` for ``n`` chunks of ``nbytes`` bytes each (LZ4 + byte shuffle, automatic block size), and what the
    host does around the kernels: ``streams`` (`LZ4_STREAM`) / ``blocks`` (`SHUFFLE_BLOCK`) for `hip.lz4_encode_streams` /
    `hip.shuffle_blocks`; once the stream sizes are known, `place` lays the containers out in one packed buffer (-> `COPY_RANGE`
    records for `hip.copy_ranges`) and `finish` writes their headers, block tables and stream lengths into it."""

    def __init__(self, n: int, nbytes: int, typesize: int):
        lib = load()
        ns, nb = C.c_int64(0), C.c_int64(0)
        layout = np.zeros(5, dtype=np.int64)
        if lib.afcodec_blosc_encode_plan(int(n), int(nbytes), int(typesize), None, 0, C.byref(ns), None, 0, C.byref(nb), layout.ctypes.data):
            raise _err(lib, "blosc_encode_plan")
        self.n, self.nbytes, self.typesize = int(n), int(nbytes), int(typesize)
        self.streams = np.zeros(ns.value, dtype=LZ4_STREAM)
        self.blocks = np.zeros(nb.value, dtype=SHUFFLE_BLOCK)
        if lib.afcodec_blosc_encode_plan(int(n), int(nbytes), int(typesize), self.streams.ctypes.data, len(self.streams), C.byref(ns),
                                         self.blocks.ctypes.data, len(self.blocks), C.byref(nb), layout.ctypes.data):
            raise _err(lib, "blosc_encode_plan")
        self.blocksize, self.n_bstarts, self.per_chunk, self.flags, self.len_bytes = (int(v) for v in layout)
        self.header_bytes = 16 + 4 * self.n_bstarts
        self.max_bsize = int(self.blocks["bsize"].max()) if len(self.blocks) else 0
        # the first stream of every block of a chunk (the records' `pad` is the stream's block)
        self.block_first = np.searchsorted(self.streams["pad"][:self.per_chunk], np.arange(self.n_bstarts))

    def place(self, csizes):
        """``csizes[n * per_chunk]`` -> (ranges, chunk_off[n], chunk_size[n]): chunk i's container is ``chunk_size[i]`` bytes at
        ``chunk_off[i]`` of the packed buffer; ``ranges`` move every stream from its slot behind its length field."""
        cs = np.asarray(csizes, dtype=np.int64).reshape(self.n, self.per_chunk)
        step = cs + self.len_bytes
        self._rel = self.header_bytes + np.cumsum(step, axis=1) - step          # each stream's length field, from the chunk's start
        size = self.header_bytes + step.sum(axis=1)
        off = np.cumsum(size) - size
        ranges = np.zeros(self.n * self.per_chunk, dtype=COPY_RANGE)
        ranges["src_off"] = self.streams["dst_off"]
        ranges["dst_off"] = (off[:, None] + self._rel + self.len_bytes).reshape(-1)
        ranges["n"] = cs.reshape(-1)
        self._cs, self._off, self._size = cs, off, size
        return ranges, off, size

    def finish(self, buf: np.ndarray):
        """The 16-byte headers, the bstarts tables and the stream lengths of the containers `place` laid out, into ``buf`` (uint8)."""
        off, size = self._off, self._size
        head = np.zeros((self.n, 16), dtype=np.uint8)
        head[:, 0], head[:, 1], head[:, 2], head[:, 3] = 2, 1, self.flags, self.typesize
        head[:, 4:8] = np.frombuffer(np.uint32(self.nbytes).astype("<u4").tobytes(), dtype=np.uint8)
        head[:, 8:12] = np.frombuffer(np.uint32(self.blocksize).astype("<u4").tobytes(), dtype=np.uint8)
        head[:, 12:16] = size.astype("<u4").view(np.uint8).reshape(-1, 4)
        buf[off[:, None] + np.arange(16)] = head
        if self.n_bstarts:
            at = off[:, None] + 16 + 4 * np.arange(self.n_bstarts)
            _put_u32(buf, at, self._rel[:, self.block_first])
        if self.len_bytes:
            _put_u32(buf, off[:, None] + self._rel, self._cs)

    def assemble_host(self, slots: np.ndarray, csizes):
        """`place` + the range copies + `finish` on the host -> the n containers (the CPU tests' stand-in for `hip.copy_ranges`)."""
        ranges, off, size = self.place(csizes)
        buf = np.zeros(int(size.sum()), dtype=np.uint8)
        for r in ranges:
            buf[r["dst_off"]:r["dst_off"] + r["n"]] = slots[r["src_off"]:r["src_off"] + r["n"]]
        self.finish(buf)
        return [buf[o:o + z].tobytes() for o, z in zip(off, size)]


# ---- the same with Zstandard streams: `hip.zstd_encode_blocks` (io.dataset_to_zarr, compress="blosc-zstd", encode="gpu") ----
ZSTD_ENCODE_BLOCK = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("scratch_off", "<i8"), ("n", "<i4"), ("last", "<i4")])   # == afhip_zstd_encode_block
ZSTD_FRAME_HEADER = 9              # magic, Frame_Header_Descriptor (Single_Segment_Flag, 4-byte Frame_Content_Size), the size


def zstd_frame_header(size: int) -> bytes:
    """The 9-byte header of the frames the GPU route writes: no window descriptor, no dictionary, no checksum."""
    return b"\x28\xb5\x2f\xfd\xa0" + int(size).to_bytes(4, "little")


def zstd_encode_block_emulate(data, last: bool = True) -> bytes:
    """`afcodec_zstd_encode_block_emulate`: the Zstandard block encoder of `zstd_encode_pass.h` as `hip.zstd_encode_blocks` runs it, on
    the host.  ``data``: 1 .. 131072 bytes -> one block with its 3-byte header (at most ``len(data) + 3`` bytes)."""
    lib = load()
    arr = np.ascontiguousarray(data).view(np.uint8).reshape(-1) if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)
    dst = np.empty(arr.nbytes + 3, dtype=np.uint8)
    r = lib.afcodec_zstd_encode_block_emulate(arr.ctypes.data, arr.nbytes, int(bool(last)), dst.ctypes.data, dst.nbytes)
    if r < 0:
        raise _err(lib, "zstd_encode_block_emulate")
    return dst[:r].tobytes()


class BloscZstdEncodePlan:
    """`afcodec_blosc_zstd_encode_plan` for ``n`` chunks of ``nbytes`` bytes each: the Zstandard twin of `BloscEncodePlan` (byte shuffle,
    unsplit 256 KiB blocks, one frame per block behind its int32 length, as `blosc_encode(cname="zstd")` lays them out).  ``blocks``
    (`SHUFFLE_BLOCK`) for `hip.shuffle_blocks`, ``streams`` (`ZSTD_ENCODE_BLOCK`) for `hip.zstd_encode_blocks`: a frame is cut at the
    byte planes of its shuffled block (128 KiB pieces where a plane is longer), every piece one block of the frame.  The shuffled input
    and the slots share ONE work buffer (the slots from ``slot_base`` on), so that `hip.copy_ranges` takes a frame's blocks from their
    slots or, for a frame that is stored, the shuffled bytes.  `place` and `finish` as in `BloscEncodePlan`."""

    def __init__(self, n: int, nbytes: int, typesize: int):
        lib = load()
        ns, nb = C.c_int64(0), C.c_int64(0)
        layout = np.zeros(8, dtype=np.int64)
        if lib.afcodec_blosc_zstd_encode_plan(int(n), int(nbytes), int(typesize), None, 0, C.byref(ns), None, 0, C.byref(nb), layout.ctypes.data):
            raise _err(lib, "blosc_zstd_encode_plan")
        self.n, self.nbytes, self.typesize = int(n), int(nbytes), int(typesize)
        self.streams = np.zeros(ns.value, dtype=ZSTD_ENCODE_BLOCK)
        self.blocks = np.zeros(nb.value, dtype=SHUFFLE_BLOCK)
        if lib.afcodec_blosc_zstd_encode_plan(int(n), int(nbytes), int(typesize), self.streams.ctypes.data, len(self.streams), C.byref(ns),
                                              self.blocks.ctypes.data, len(self.blocks), C.byref(nb), layout.ctypes.data):
            raise _err(lib, "blosc_zstd_encode_plan")
        (self.blocksize, self.n_bstarts, self.per_chunk, self.flags, self.len_bytes, self.slot_base, self.slot_bytes,
         self.scratch_bytes) = (int(v) for v in layout)
        self.header_bytes = 16 + 4 * self.n_bstarts
        self.max_bsize = int(self.blocks["bsize"].max()) if len(self.blocks) else 0
        self.work_bytes = self.slot_base + self.slot_bytes
        self.stored = self.n_bstarts == 0                                      # chunks under 128 bytes: the raw bytes behind the header
        self.frames = max(1, self.n_bstarts)                                   # per chunk
        last = self.streams["last"][:self.per_chunk]
        self.frame_first = np.concatenate([[0], np.nonzero(last)[0][:-1] + 1]).astype(np.int64) if self.per_chunk else np.zeros(0, np.int64)
        self.frame_of = np.cumsum(np.concatenate([[0], last[:-1]])).astype(np.int64) if self.per_chunk else np.zeros(0, np.int64)
        self.bsize = self.blocks["bsize"][:self.frames].astype(np.int64)       # of every frame of a chunk

    def place(self, csizes):
        """``csizes[n * per_chunk]`` (bytes of every Zstandard block) -> (ranges, chunk_off[n], chunk_size[n]); a frame that would not be
        shorter than its block's size - 1 is stored: one range takes the shuffled bytes instead (``stored_frames`` counts them)."""
        if self.stored:
            size = np.full(self.n, 16 + self.nbytes, dtype=np.int64)
            off = np.cumsum(size) - size
            ranges = np.zeros(self.n, dtype=COPY_RANGE)
            ranges["src_off"], ranges["dst_off"], ranges["n"] = self.blocks["tmp_off"], off + 16, self.nbytes
            self._off, self._size, self.stored_frames = off, size, self.n
            return ranges, off, size
        cs = np.asarray(csizes, dtype=np.int64).reshape(self.n, self.per_chunk)
        fsize = ZSTD_FRAME_HEADER + np.add.reduceat(cs, self.frame_first, axis=1)               # (n, frames)
        kept = fsize < self.bsize[None, :] - 1
        fsize = np.where(kept, fsize, self.bsize[None, :])
        step = fsize + self.len_bytes
        rel = self.header_bytes + np.cumsum(step, axis=1) - step                                  # each frame's length field, from the chunk's start
        size = self.header_bytes + step.sum(axis=1)
        off = np.cumsum(size) - size
        inner = np.cumsum(cs, axis=1) - cs
        inner = inner - inner[:, self.frame_first][:, self.frame_of]                             # each block, from its frame's first block
        kept_b = kept[:, self.frame_of]
        at = (off[:, None] + rel + self.len_bytes)[:, self.frame_of] + ZSTD_FRAME_HEADER + inner
        packed = np.zeros(int(kept_b.sum()), dtype=COPY_RANGE)
        packed["src_off"] = self.slot_base + self.streams["dst_off"].reshape(self.n, self.per_chunk)[kept_b]
        packed["dst_off"], packed["n"] = at[kept_b], cs[kept_b]
        raw = np.zeros(int((~kept).sum()), dtype=COPY_RANGE)
        raw["src_off"] = self.blocks["tmp_off"].reshape(self.n, self.frames)[~kept]
        raw["dst_off"], raw["n"] = (off[:, None] + rel + self.len_bytes)[~kept], np.broadcast_to(self.bsize, kept.shape)[~kept]
        self._kept, self._fsize, self._rel, self._off, self._size = kept, fsize, rel, off, size
        self.stored_frames = int((~kept).sum())
        return np.concatenate([packed, raw]), off, size

    def finish(self, buf: np.ndarray):
        """The 16-byte headers, the bstarts tables, the frame lengths and the frame headers of the containers `place` laid out."""
        off, size = self._off, self._size
        head = np.zeros((self.n, 16), dtype=np.uint8)
        head[:, 0], head[:, 1], head[:, 2], head[:, 3] = 2, 1, self.flags, self.typesize
        head[:, 4:8] = np.frombuffer(np.uint32(self.nbytes).astype("<u4").tobytes(), dtype=np.uint8)
        head[:, 8:12] = np.frombuffer(np.uint32(self.blocksize).astype("<u4").tobytes(), dtype=np.uint8)
        head[:, 12:16] = size.astype("<u4").view(np.uint8).reshape(-1, 4)
        buf[off[:, None] + np.arange(16)] = head
        if self.stored:
            return
        _put_u32(buf, off[:, None] + 16 + 4 * np.arange(self.n_bstarts), self._rel)
        _put_u32(buf, off[:, None] + self._rel, self._fsize)
        at = (off[:, None] + self._rel + self.len_bytes)[self._kept]
        fh = np.zeros((len(at), ZSTD_FRAME_HEADER), dtype=np.uint8)
        fh[:, :5] = np.frombuffer(zstd_frame_header(0)[:5], dtype=np.uint8)
        fh[:, 5:] = np.broadcast_to(self.bsize, self._kept.shape)[self._kept].astype("<u4").view(np.uint8).reshape(-1, 4)
        buf[at[:, None] + np.arange(ZSTD_FRAME_HEADER)] = fh

    def assemble_host(self, work: np.ndarray, csizes):
        """`place` + the range copies + `finish` on the host -> the n containers (the CPU tests' stand-in for `hip.copy_ranges`);
        ``work``: the work buffer, shuffled input and slots."""
        ranges, off, size = self.place(csizes)
        buf = np.zeros(int(size.sum()), dtype=np.uint8)
        for r in ranges:
            buf[r["dst_off"]:r["dst_off"] + r["n"]] = work[r["src_off"]:r["src_off"] + r["n"]]
        self.finish(buf)
        return [buf[o:o + z].tobytes() for o, z in zip(off, size)]


# record layouts shared with libaggfly_hip (include/aggfly_hip.h: afhip_zstd_frame, afhip_zstd_block; zstd_passes.h)
ZSTD_FRAME = np.dtype([("dst_off", "<i8"), ("base", "<i8"), ("size", "<i8"), ("first_block", "<i4"), ("n_blocks", "<i4")])
ZSTD_BLOCK = np.dtype([("src", "<i8"), ("lit_off", "<i8"), ("seq_off", "<i8"), ("frame", "<i4"), ("btype", "<i4"), ("csize", "<i4"),
                       ("lit_type", "<i4"), ("lit_size", "<i4"), ("lit_src", "<i4"), ("lit_csize", "<i4"), ("n_streams", "<i4"),
                       ("huf_desc", "<i4"), ("huf_block", "<i4"), ("nseq", "<i4"), ("seq_src", "<i4"), ("mode", "<i4", 3),
                       ("tab_desc", "<i4", 3), ("tab_block", "<i4", 3), ("pad", "<i4")])


class ZstdPlan:
    """What `zstd_plan` found in a batch: record counts and the sizes of the per-batch buffers."""

    def __init__(self, n_frames, n_blocks, lit_bytes, n_seqs, dec_bytes, results):
        self.n_frames, self.n_blocks, self.lit_bytes, self.n_seqs, self.dec_bytes = n_frames, n_blocks, lit_bytes, n_seqs, dec_bytes
        self.results = results

    def scratch_bytes(self) -> int:
        return int(load().afcodec_zstd_scratch_bytes(self.n_blocks, self.n_frames, self.lit_bytes, self.n_seqs, self.dec_bytes))


def zstd_plan(base: np.ndarray, comp_off, comp_size, out_off, out_size, frames: np.ndarray, blocks: np.ndarray, strict: bool = True):
    """Plan the GPU-side decode of Zstandard frames that sit in ``base`` (uint8; chunk i = ``comp_size[i]`` bytes at
    ``comp_off[i]``, decoded to ``out_off[i]`` of the output, ``out_size[i]`` bytes): fills ``frames`` (dtype `ZSTD_FRAME`)
    and ``blocks`` (dtype `ZSTD_BLOCK`) for `hip.zstd_decode`.  -> `ZstdPlan`; ``results[i]`` = decoded size, or
    `E_UNSUPPORTED` for a frame the GPU route does not take (decode it on the host); malformed frames raise `CodecError`
    (``strict=False``: they are only marked negative in ``results``)."""
    lib = load()
    n = len(comp_off)
    co, cs, oo, osz = (np.ascontiguousarray(a, dtype=np.int64) for a in (comp_off, comp_size, out_off, out_size))
    res = np.zeros(n, dtype=np.int64)
    nf, nb, lit, nsq, dec = (C.c_int64(0) for _ in range(5))
    assert frames.dtype == ZSTD_FRAME and blocks.dtype == ZSTD_BLOCK and base.dtype == np.uint8
    rc = lib.afcodec_zstd_plan(base.ctypes.data, n, co.ctypes.data, cs.ctypes.data, oo.ctypes.data, osz.ctypes.data,
                               frames.ctypes.data, len(frames), C.byref(nf), blocks.ctypes.data, len(blocks), C.byref(nb),
                               C.byref(lit), C.byref(nsq), C.byref(dec), res.ctypes.data)
    bad = [int(i) for i in np.nonzero((res < 0) & (res != E_UNSUPPORTED))[0]]
    if rc and "list too small" in lib.afcodec_last_error().decode() and not bad:
        raise PlanCapacityError(f"zstd_plan: {lib.afcodec_last_error().decode()}")
    if strict and bad:
        raise CodecError(f"zstd_plan: chunks {bad[:8]} are malformed: {lib.afcodec_last_error().decode()}")
    return ZstdPlan(int(nf.value), int(nb.value), int(lit.value), int(nsq.value), int(dec.value), res)


def _emulation_scratch(scratch, nbytes: int) -> np.ndarray:
    """A fresh zeroed scratch, or the caller's (uint8, contiguous, 16-byte aligned like the device's, at least ``nbytes``) as it is."""
    if scratch is None:
        return np.zeros(nbytes, dtype=np.uint8)
    if scratch.dtype != np.uint8 or not scratch.flags.c_contiguous or scratch.nbytes < nbytes or scratch.ctypes.data % 16:
        raise ValueError(f"scratch must be a contiguous, 16-byte aligned uint8 array of at least {nbytes} bytes")
    return scratch


def zstd_emulate(base: np.ndarray, frames: np.ndarray, blocks: np.ndarray, plan: ZstdPlan, out: np.ndarray, scratch: np.ndarray | None = None):
    """Run the passes of the GPU decode (`hip.zstd_decode`) on this thread — the host reference of the GPU algorithm, for
    tests.  ``scratch``: the passes' scratch (at least ``plan.scratch_bytes()``), whose previous content is not an input; a fresh
    zeroed array when None.  -> (errors, pointer-jump rounds)."""
    lib = load()
    scratch = _emulation_scratch(scratch, plan.scratch_bytes())
    err, rounds = C.c_int32(0), C.c_int32(0)
    lib.afcodec_zstd_emulate(base.ctypes.data, base.nbytes, frames.ctypes.data, plan.n_frames, blocks.ctypes.data, plan.n_blocks,
                             plan.lit_bytes, plan.n_seqs, plan.dec_bytes, scratch.ctypes.data, out.ctypes.data, C.byref(err),
                             C.byref(rounds))
    return int(err.value), int(rounds.value)


class BloscPlan:
    """What `blosc_plan` found in a batch: the record counts of its five lists, the shuffle scratch, and — for `hip.zstd_decode`,
    which reads the same attributes of a `ZstdPlan` — the Zstandard totals (``n_blocks`` counts Zstandard blocks)."""

    def __init__(self, n_streams, n_shuf, n_bits, n_frames, n_blocks, lit_bytes, n_seqs, dec_bytes, tmp_bytes, max_dsize, max_shuf, max_bits,
                 results):
        self.n_streams, self.n_shuf, self.n_bits, self.n_frames, self.n_blocks = n_streams, n_shuf, n_bits, n_frames, n_blocks
        self.lit_bytes, self.n_seqs, self.dec_bytes, self.tmp_bytes, self.max_dsize = lit_bytes, n_seqs, dec_bytes, tmp_bytes, max_dsize
        self.max_shuf, self.max_bits, self.results = max_shuf, max_bits, results

    def scratch_bytes(self) -> int:
        return int(load().afcodec_zstd_scratch_bytes(self.n_blocks, self.n_frames, self.lit_bytes, self.n_seqs, self.dec_bytes))


def blosc_plan(base: np.ndarray, comp_off, comp_size, out_off, out_size, streams: np.ndarray, shuf: np.ndarray, bits: np.ndarray,
               frames: np.ndarray, zblocks: np.ndarray, strict: bool = True):
    """Plan the GPU-side decode of Blosc-1 chunks of any flavour the GPU takes — LZ4 / LZ4HC or Zstandard inside, shuffle none,
    byte or bit — that sit in ``base`` (uint8; chunk i = ``comp_size[i]`` bytes at ``comp_off[i]``): fills ``streams`` (`LZ4_STREAM`)
    for `hip.lz4_decode_streams`, ``frames`` / ``zblocks`` (`ZSTD_FRAME` / `ZSTD_BLOCK`) for `hip.zstd_decode` INTO THE SCRATCH,
    ``shuf`` and ``bits`` (`SHUFFLE_BLOCK`) for `hip.unshuffle_blocks` / `hip.bitunshuffle_blocks`.  -> `BloscPlan`;
    ``results[i]`` = decoded size, or `E_UNSUPPORTED` for a chunk the GPU route does not take (blosclz / zlib / snappy inside, a
    Zstandard frame `zstd_plan` would refuse: decode it on the host); malformed containers raise `CodecError` (``strict=False``:
    they are only marked negative in ``results``)."""
    lib = load()
    n = len(comp_off)
    co, cs, oo, osz = (np.ascontiguousarray(a, dtype=np.int64) for a in (comp_off, comp_size, out_off, out_size))
    res = np.zeros(n, dtype=np.int64)
    ns, nsh, nbt, nf, nzb, lit, nsq, dec, tmp = (C.c_int64(0) for _ in range(9))
    maxd = C.c_int32(0)
    assert streams.dtype == LZ4_STREAM and shuf.dtype == SHUFFLE_BLOCK and bits.dtype == SHUFFLE_BLOCK and base.dtype == np.uint8
    assert frames.dtype == ZSTD_FRAME and zblocks.dtype == ZSTD_BLOCK
    rc = lib.afcodec_blosc_plan(base.ctypes.data, n, co.ctypes.data, cs.ctypes.data, oo.ctypes.data, osz.ctypes.data,
                                streams.ctypes.data, len(streams), C.byref(ns), shuf.ctypes.data, len(shuf), C.byref(nsh),
                                bits.ctypes.data, len(bits), C.byref(nbt), frames.ctypes.data, len(frames), C.byref(nf),
                                zblocks.ctypes.data, len(zblocks), C.byref(nzb), C.byref(lit), C.byref(nsq), C.byref(dec), C.byref(tmp),
                                C.byref(maxd), res.ctypes.data)
    bad = [int(i) for i in np.nonzero((res < 0) & (res != E_UNSUPPORTED))[0]]
    if rc and not bad and "list too small" in lib.afcodec_last_error().decode():
        raise PlanCapacityError(f"blosc_plan: {lib.afcodec_last_error().decode()}")
    if strict and bad:
        raise CodecError(f"blosc_plan: chunks {bad[:8]} are malformed: {lib.afcodec_last_error().decode()}")
    max_shuf = int(shuf["bsize"][:nsh.value].max()) if nsh.value else 0
    max_bits = int(bits["bsize"][:nbt.value].max()) if nbt.value else 0
    return BloscPlan(int(ns.value), int(nsh.value), int(nbt.value), int(nf.value), int(nzb.value), int(lit.value), int(nsq.value),
                     int(dec.value), int(tmp.value), int(maxd.value), max_shuf, max_bits, res)


# record layout shared with libaggfly_hip (include/aggfly_hip.h: afhip_inflate_stream; inflate_passes.h)
INFLATE_STREAM = np.dtype([("src", "<i8"), ("dst_off", "<i8"), ("base", "<i8"), ("seq_off", "<i8"), ("csize", "<i4"), ("dsize", "<i4"),
                           ("to_out", "<i4"), ("first_block", "<i4"), ("n_blocks", "<i4"), ("first_piece", "<i4")])


class InflatePlan:
    """What `inflate_plan` found in a batch: record counts and the sizes of the per-batch buffers."""

    def __init__(self, n_streams, n_shuf, n_pblocks, n_seqs, n_pieces, dec_bytes, tmp_bytes, max_bsize, results):
        self.n_streams, self.n_shuf, self.n_pblocks, self.n_seqs, self.n_pieces = n_streams, n_shuf, n_pblocks, n_seqs, n_pieces
        self.dec_bytes, self.tmp_bytes, self.max_bsize, self.results = dec_bytes, tmp_bytes, max_bsize, results

    def sizes(self):
        return self.n_streams, self.n_pblocks, self.n_seqs, self.n_pieces, self.dec_bytes, self.tmp_bytes

    def scratch_bytes(self) -> int:
        return int(load().afcodec_inflate_scratch_bytes(*self.sizes()))


def inflate_plan(base: np.ndarray, comp_off, comp_size, out_off, out_size, streams: np.ndarray, shuf: np.ndarray, typesize=1,
                 strict: bool = True):
    """Plan the GPU-side decode of zlib streams that sit in ``base`` (uint8; chunk i = ``comp_size[i]`` bytes at ``comp_off[i]``,
    decoded to ``out_off[i]`` of the output, ``out_size[i]`` bytes; ``typesize`` — one for all chunks, or one per chunk — > 1: byte-unshuffled there, HDF5's
    shuffle + deflate): fills ``streams`` (dtype `INFLATE_STREAM`) and ``shuf`` (dtype `SHUFFLE_BLOCK`) for `hip.inflate_decode`.
    -> `InflatePlan`; ``results[i]`` = decoded size, or `E_UNSUPPORTED` for a chunk the GPU route does not take (preset
    dictionary, gzip member, 1 GiB or more: decode it on the host); other header bytes raise `CodecError` (``strict=False``: they
    are only marked negative in ``results``)."""
    lib = load()
    n = len(comp_off)
    co, cs, oo, osz = (np.ascontiguousarray(a, dtype=np.int64) for a in (comp_off, comp_size, out_off, out_size))
    res = np.zeros(n, dtype=np.int64)
    ns, nsh, nb, nsq, npc, dec, tmp = (C.c_int64(0) for _ in range(7))
    assert streams.dtype == INFLATE_STREAM and shuf.dtype == SHUFFLE_BLOCK and base.dtype == np.uint8
    ts = np.ascontiguousarray(np.broadcast_to(np.asarray(typesize, dtype=np.int32), (n,)))
    rc = lib.afcodec_inflate_plan(base.ctypes.data, n, co.ctypes.data, cs.ctypes.data, oo.ctypes.data, osz.ctypes.data, ts.ctypes.data,
                                  streams.ctypes.data, len(streams), C.byref(ns), shuf.ctypes.data, len(shuf), C.byref(nsh), C.byref(nb),
                                  C.byref(nsq), C.byref(npc), C.byref(dec), C.byref(tmp), res.ctypes.data)
    bad = [int(i) for i in np.nonzero((res < 0) & (res != E_UNSUPPORTED))[0]]
    if rc and not bad and ("list too small" in lib.afcodec_last_error().decode() or "2 GiB" in lib.afcodec_last_error().decode()):
        raise PlanCapacityError(f"inflate_plan: {lib.afcodec_last_error().decode()}")
    if rc == -3:
        raise _err(lib, "inflate_plan")
    if strict and bad:
        raise CodecError(f"inflate_plan: chunks {bad[:8]} are malformed: {lib.afcodec_last_error().decode()}")
    max_b = int(shuf["bsize"][:nsh.value].max()) if nsh.value else 0
    return InflatePlan(int(ns.value), int(nsh.value), int(nb.value), int(nsq.value), int(npc.value), int(dec.value), int(tmp.value), max_b, res)


def inflate_emulate(base: np.ndarray, streams: np.ndarray, shuf: np.ndarray, plan: InflatePlan, out: np.ndarray,
                    scratch: np.ndarray | None = None):
    """Run the passes of the GPU decode (`hip.inflate_decode`) on this thread — the host reference of the GPU algorithm, for
    tests.  ``scratch`` as for `zstd_emulate`.  -> (errors, pointer-jump rounds)."""
    lib = load()
    scratch = _emulation_scratch(scratch, plan.scratch_bytes())
    err, rounds = C.c_int32(0), C.c_int32(0)
    lib.afcodec_inflate_emulate(base.ctypes.data, base.nbytes, streams.ctypes.data, plan.n_streams, shuf.ctypes.data, plan.n_shuf,
                                plan.n_pblocks, plan.n_seqs, plan.n_pieces, plan.dec_bytes, plan.tmp_bytes, scratch.ctypes.data,
                                out.ctypes.data, C.byref(err), C.byref(rounds))
    return int(err.value), int(rounds.value)


def aec_decode(data, n_values: int, nbits: int, flags: int, block_size: int, rsi: int) -> np.ndarray:
    """`afcodec_aec_decode`: the ``n_values`` samples (uint32) of one CCSDS / AEC stream as libaec writes it (the body of section 7 of
    a GRIB2 message in template 5.42).  ``flags`` 8: the preprocessor; a damaged or truncated stream raises `CodecError`."""
    lib = load()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.empty(int(n_values), dtype=np.uint32)
    if lib.afcodec_aec_decode(buf.ctypes.data, buf.nbytes, int(n_values), int(nbits), int(flags), int(block_size), int(rsi), out.ctypes.data):
        raise _err(lib, "aec_decode")
    return out


def lzw_decode_ranges(locators, outs, threads: int = 8):
    """`afcodec_lzw_decode_ranges`: the TIFF LZW streams ``locators[i] = (path, offset, nbytes)`` (strips or tiles of a TIFF) decoded
    into the uint8 arrays ``outs[i]``, each of which its stream must fill exactly, on the native OpenMP team.  A damaged or truncated
    stream, or a range beyond its file, raises `CodecError` naming the first few."""
    lib = load()
    n = len(locators)
    pp = (C.c_char_p * n)(*[os.fsencode(l[0]) for l in locators])
    offs = (C.c_int64 * n)(*[int(l[1]) for l in locators])
    lens = (C.c_int64 * n)(*[int(l[2]) for l in locators])
    dp = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    ds = (C.c_int64 * n)(*[o.nbytes for o in outs])
    res = (C.c_int64 * n)()
    if lib.afcodec_lzw_decode_ranges(n, pp, offs, lens, dp, ds, int(threads), res):
        bad = [locators[i] for i in range(n) if res[i] < 0]
        raise CodecError(f"lzw_decode_ranges: {len(bad)} segment(s) failed, first {bad[:4]}: {lib.afcodec_last_error().decode()}")
    return [int(res[i]) for i in range(n)]
