"""Writes tests/golden/blosc_encode_parent.json: sha256 of what `codec.blosc_encode` writes for a grid of inputs.  It was run on
the build BEFORE `afcodec_blosc_encode` came to share its block-size lines with `afcodec_blosc_encode_plan` (AGGFLY_CODEC_LIB
pointing at that build's libaggfly_codec.so); tests/test_lz4_encode.py holds every later build to these bytes.

    AGGFLY_CODEC_LIB=/path/to/older/libaggfly_codec.so python tests/golden/make_blosc_encode_parent_golden.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ctypes as C                              # noqa: E402

import numpy as np                              # noqa: E402
from aggfly_amd import codec                    # noqa: E402
from test_lz4_encode import _chunk              # noqa: E402

# (an older library lacks the entry points `codec.load` binds: the two this script needs are bound here)
lib = C.CDLL(os.environ.get("AGGFLY_CODEC_LIB", codec.LIB_PATH))
lib.afcodec_blosc_bound.restype = lib.afcodec_blosc_encode.restype = C.c_int64
lib.afcodec_blosc_bound.argtypes = [C.c_int64, C.c_int64]
lib.afcodec_blosc_encode.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64]


def encode(raw, typesize, shuffle, blocksize, cname):
    cap = lib.afcodec_blosc_bound(raw.nbytes, blocksize)
    dst = np.empty(cap, dtype=np.uint8)
    r = lib.afcodec_blosc_encode(raw.ctypes.data, raw.nbytes, typesize, shuffle, codec.BLOSC_CNAME[cname], 3, blocksize, dst.ctypes.data, cap)
    assert r > 0, r
    return dst[:r].tobytes()


cases = []
for cname in ("lz4", "zstd"):
    for shuffle in (0, 1, 2):
        for typesize in (1, 2, 4, 8):
            for nbytes, blocksize in ((0, 0), (100, 0), (127, 0), (128, 0), (1001, 0), (65536 * 4 - 4, 0), (65536 * 4 + 12, 0), (300000, 4096),
                                      (70001, 1000)):
                seed = len(cases)
                raw = _chunk(nbytes, typesize, seed)
                out = encode(raw, typesize, shuffle, blocksize, cname)
                cases.append({"cname": cname, "shuffle": shuffle, "typesize": typesize, "nbytes": nbytes, "blocksize": blocksize, "seed": seed,
                              "sha256": hashlib.sha256(out).hexdigest()})
json.dump({"cases": cases}, open(os.path.join(HERE, "blosc_encode_parent.json"), "w"), indent=0)
print(len(cases), "cases")
