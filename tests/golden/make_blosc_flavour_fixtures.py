"""Generates tests/golden/blosc_flavour_fixtures.json for the Blosc flavours of the decode-in-HBM route beyond LZ4 + byte shuffle
(tests/test_blosc_plan.py, tests/test_gpu_blosc_flavours.py):

* ``cases``: a few chunks compressed by the REAL c-blosc 1.x whose Zstandard frames hold MORE THAN ONE Zstandard block (Blosc
  blocks of 256 KiB and more: clevel >= 5 on >= 600 KB) — blosc_fixtures.json's Zstandard chunks are all single-block frames.
  Inputs are the seeded recipes of make_blosc_fixtures.py, so only the compressed bytes
  and a SHA-256 of the raw bytes are stored;
* ``encoder``: for the in-tree Blosc-1 encoder's new flavours (LZ4 + bit shuffle, Zstandard with byte / bit / no shuffle), the
  SHA-256 of the chunk it writes, stored only after the real c-blosc has decoded that chunk back to the input byte for byte.
  Zstandard bytes depend on the libzstd that compressed them: ``zstd_version`` records ZSTD_versionNumber(), and the test holds the
  Zstandard digests only where the loaded library reports the same number (the LZ4 digests always).

    python tests/golden/make_blosc_flavour_fixtures.py PATH/TO/libblosc.so.1      # after build()
"""
import base64
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_blosc_fixtures import recipe          # noqa: E402

CASES = [dict(cname="zstd", shuffle=1, dtype="<f4", n=160000, recipe="steps", clevel=5, blocksize=0),
         dict(cname="zstd", shuffle=2, dtype="<f4", n=160000, recipe="steps", clevel=5, blocksize=0),
         dict(cname="zstd", shuffle=0, dtype="<f8", n=100001, recipe="constant", clevel=5, blocksize=0)]

# the in-tree encoder: (flavour, dtype, n); flavour -> blosc_encode's keywords
FLAVOURS = {"lz4-bitshuffle": dict(cname="lz4", bitshuffle=True), "zstd-shuffle": dict(cname="zstd", shuffle=True),
            "zstd-bitshuffle": dict(cname="zstd", bitshuffle=True), "zstd-noshuffle": dict(cname="zstd", shuffle=False)}
ENCODER_SHAPES = [("<f4", 1000000), ("<f8", 333333), ("<f4", 17), ("<i2", 50000)]


def flavour_input(kind, dtype, n):
    """The seeded arrays the encoder tests compress: smooth (a field plus a little noise), noisy, constant (Zstandard RLE blocks),
    random (incompressible: stored streams)."""
    rng = np.random.default_rng(n + len(kind))
    dt = np.dtype(dtype)
    if kind == "smooth":
        x = 280 + 10 * np.sin(np.arange(n) / 50) + np.round(rng.normal(0, 0.3, n), 2)
    elif kind == "noisy":
        x = 280 + 10 * np.sin(np.arange(n) / 50) + rng.normal(0, 3, n)
    elif kind == "constant":
        x = np.full(n, 273.15)
    elif kind == "random":
        return np.frombuffer(rng.bytes(n * dt.itemsize), dtype=dt).copy()
    else:
        raise KeyError(kind)
    return np.round(x).astype(dt) if dt.kind in "iu" else x.astype(dt)


def encoder_case_id(flavour, dtype, n):
    return f"{flavour}-{dtype[1:]}-{n}"


def load():
    return json.load(open(os.path.join(HERE, "blosc_flavour_fixtures.json")))


def zstd_version():
    """ZSTD_versionNumber() of the libzstd the codec library compresses with (the same dlopen name)."""
    try:
        return int(C.CDLL("libzstd.so.1").ZSTD_versionNumber())
    except OSError:
        return 0


def main(lib_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from aggfly_amd import codec
    lib = C.CDLL(lib_path)
    lib.blosc_compress_ctx.restype = C.c_int
    lib.blosc_compress_ctx.argtypes = [C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                       C.c_char_p, C.c_size_t, C.c_int]
    lib.blosc_get_version_string.restype = C.c_char_p
    ver = lib.blosc_get_version_string().decode()
    out = {"generator": f"tests/golden/make_blosc_flavour_fixtures.py with c-blosc {ver}", "zstd_version": zstd_version(), "cases": [],
           "encoder": {}}
    for i, c in enumerate(CASES):
        raw = recipe(c["recipe"], c["n"], c["dtype"], seed=2000 + i)
        src = raw.tobytes()
        dst = C.create_string_buffer(len(src) + 16 + 4096)
        nb = lib.blosc_compress_ctx(c["clevel"], c["shuffle"], raw.dtype.itemsize, len(src), src, dst, len(dst), c["cname"].encode(),
                                    c["blocksize"], 1)
        assert nb > 0, (c, nb)
        back = C.create_string_buffer(len(src))
        assert lib.blosc_decompress_ctx(dst, back, len(src), 1) == len(src) and back.raw == src
        out["cases"].append(dict(c, seed=2000 + i, sha256=hashlib.sha256(src).hexdigest(), nbytes=len(src), cbytes=nb,
                                 chunk_b64=base64.b64encode(dst.raw[:nb]).decode()))
    for flavour, kw in FLAVOURS.items():
        for dtype, n in ENCODER_SHAPES:
            x = flavour_input("smooth", dtype, n)
            enc = codec.blosc_encode(x, x.dtype.itemsize, **kw)
            back = C.create_string_buffer(x.nbytes)
            if lib.blosc_decompress_ctx(enc, back, x.nbytes, 1) != x.nbytes or back.raw != x.tobytes():
                raise SystemExit(f"c-blosc does not read the encoder's chunk back for {encoder_case_id(flavour, dtype, n)}")
            out["encoder"][encoder_case_id(flavour, dtype, n)] = {"input_sha256": hashlib.sha256(x.tobytes()).hexdigest(),
                                                                 "chunk_sha256": hashlib.sha256(enc).hexdigest(), "chunk_bytes": len(enc)}
    with open(os.path.join(HERE, "blosc_flavour_fixtures.json"), "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(len(out["cases"]), "chunks,", sum(c["cbytes"] for c in out["cases"]), "compressed bytes;", len(out["encoder"]), "encoder digests; c-blosc", ver,
          "libzstd", out["zstd_version"])


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
