"""Generates tests/golden/zstd_fixtures.json: Zstandard frames written by the REAL libzstd (libzstd.so.1, through ctypes;
ZSTD_compress2 + ZSTD_CCtx_setParameter for the advanced cases) for the decode-in-HBM route (afcodec_zstd_plan,
afhip_zstd_decode) to be checked against.  Inputs are recipes (seeded numpy: `make_blosc_fixtures.recipe`, float32 / float64
synth fields, and two byte recipes here), so only the frames and a SHA-256 of the raw bytes are stored.  The generator walks
every frame's headers and records the block types, literal types, stream counts and the LL / OF / ML modes it holds.

    python tests/golden/make_zstd_fixtures.py
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
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_blosc_fixtures import recipe as blosc_recipe  # noqa: E402

ZSTD_c_compressionLevel, ZSTD_c_windowLog, ZSTD_c_contentSizeFlag, ZSTD_c_checksumFlag = 100, 101, 200, 201


def recipe(name, n, dtype, seed):
    """n elements of dtype (bytes: n bytes)."""
    if name == "synth":                   # the synthetic temperature field of the benchmarks
        from aggfly_amd import synth
        ny = 16
        t = -(-n // (ny * ny))
        return synth.temperature_cube(t, ny, ny, dtype=np.dtype(dtype), seed=seed).reshape(-1)[:n].copy()
    if name == "noise_bytes":             # incompressible: raw blocks
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    if name == "fill_bytes":              # one byte value: RLE blocks
        return np.full(n, seed & 0xFF, dtype=np.uint8)
    if name == "sparse_bytes":            # a 16-byte period whose first byte is random: 1 literal + 1 repeat-offset match, RLE modes
        a = np.tile(np.arange(16, dtype=np.uint8), -(-n // 16))[:n]
        a[::16] = np.random.default_rng(seed).integers(0, 256, len(a[::16]))
        return a
    return blosc_recipe(name, n, dtype, seed)


def raw_of(case):
    return recipe(case["recipe"], case["n"], case["dtype"], case["seed"]).tobytes()


# (recipe, n, dtype, seed, level, extra parameters); level None = the advanced API with the parameters only
CASES = []
for lvl in (-5, 1, 3, 9, 19):
    CASES.append(dict(recipe="temperature", n=600, dtype="<f4", seed=1, level=lvl))
    CASES.append(dict(recipe="synth", n=300, dtype="<f8", seed=2, level=lvl))
    CASES.append(dict(recipe="steps", n=9000, dtype="<f4", seed=3, level=lvl))
CASES += [
    dict(recipe="steps", n=40000, dtype="<f4", seed=4, level=19),                           # 2 blocks: treeless literals, ML repeat
    dict(recipe="steps", n=70000, dtype="<f4", seed=5, level=3),                            # 3 blocks, the last short: repeat modes
    dict(recipe="nanmask", n=1000, dtype="<f4", seed=6, level=9),
    dict(recipe="sparse_bytes", n=16 * 9000 + 1, dtype="|u1", seed=18, level=3),          # 2nd block: LL / OF / ML RLE modes
    dict(recipe="constant", n=40000, dtype="<f8", seed=7, level=3),                         # period-8 runs: offset < length
    dict(recipe="noise_bytes", n=1500, dtype="|u1", seed=8, level=3),                       # a raw block
    dict(recipe="fill_bytes", n=300000, dtype="|u1", seed=9, level=3),                      # RLE blocks
    dict(recipe="random", n=300, dtype="<f8", seed=10, level=1),
    dict(recipe="temperature", n=3000, dtype="<i2", seed=11, level=19, params={ZSTD_c_windowLog: 10}),
    dict(recipe="noise_bytes", n=1, dtype="|u1", seed=12, level=3),                         # tiny
    dict(recipe="fill_bytes", n=7, dtype="|u1", seed=13, level=3),
    dict(recipe="noise_bytes", n=0, dtype="|u1", seed=14, level=3),                         # empty frame
    # not taken by the GPU route (results E_UNSUPPORTED):
    dict(recipe="temperature", n=500, dtype="<f4", seed=15, level=3, params={ZSTD_c_checksumFlag: 1}, taken=False, why="checksum"),
    dict(recipe="temperature", n=500, dtype="<f4", seed=16, level=3, params={ZSTD_c_contentSizeFlag: 0}, taken=False, why="no content size"),
    dict(recipe="temperature", n=500, dtype="<f4", seed=17, level=3, twice=True, taken=False, why="two frames"),
]


REQUIRED_MODES = {"block:raw", "block:rle", "block:compressed", "frame:single-block", "frame:multi-block",
                  "literals:raw", "literals:compressed", "literals:treeless", "streams:1", "streams:4"} | {
    f"{t}:{m}" for t in ("LL", "OF", "ML") for m in ("predefined", "rle", "fse", "repeat")}


def load():
    """-> [(fixture entry, frame bytes, raw bytes)] of zstd_fixtures.json."""
    with open(os.path.join(HERE, "zstd_fixtures.json")) as f:
        doc = json.load(f)
    return [(e, base64.b64decode(e["frame"]), raw_of(e)) for e in doc["fixtures"]]


def pack(frames, sizes, gap=64):
    """Frames back to back (64-byte steps) in one uint8 buffer, their outputs at 64-byte steps with ``gap`` bytes between ->
    (base, comp_off, comp_size, out_off, out_bytes)."""
    offs = np.concatenate([[0], np.cumsum([(len(c) + 63) // 64 * 64 for c in frames])]).astype(np.int64)
    base = np.zeros(max(int(offs[-1]), 64), dtype=np.uint8)
    for o, c in zip(offs, frames):
        base[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)
    out_off = (np.concatenate([[0], np.cumsum([(n + 63) // 64 * 64 + gap for n in sizes])]) + gap).astype(np.int64)
    return base, offs[:-1], np.array([len(c) for c in frames], dtype=np.int64), out_off[:-1], int(out_off[-1]) + gap


def walk(frame: bytes):
    """Which block / literal / sequence modes a frame holds (headers only)."""
    seen = set()
    if len(frame) < 6 or int.from_bytes(frame[:4], "little") != 0xFD2FB528:
        return seen
    fhd = frame[4]
    single, fcs_flag, did_flag = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[did_flag] + ((1 if single else 0) if fcs_flag == 0 else (2, 4, 8)[fcs_flag - 1])
    nblocks = 0
    while pos + 3 <= len(frame):
        bh = int.from_bytes(frame[pos:pos + 3], "little")
        last, bt, bs = bh & 1, (bh >> 1) & 3, bh >> 3
        pos += 3
        nblocks += 1
        seen.add(("block", ("raw", "rle", "compressed")[bt]))
        if bt == 2:
            q = frame[pos:pos + bs]
            lt, sf = q[0] & 3, (q[0] >> 2) & 3
            seen.add(("literals", ("raw", "rle", "compressed", "treeless")[lt]))
            if lt < 2:
                hs = 1 if sf & 1 == 0 else (2 if sf == 1 else 3)
                regen = q[0] >> 3 if hs == 1 else (q[0] >> 4) + (q[1] << 4) + ((q[2] << 12) if hs == 3 else 0)
                s = hs + (regen if lt == 0 else 1)
            else:
                seen.add(("streams", 1 if sf == 0 else 4))
                hs = 3 if sf < 2 else sf + 2
                h = int.from_bytes(q[:hs], "little")
                bits = {3: 10, 4: 14, 5: 18}[hs]
                s = hs + ((h >> (4 + bits)) & ((1 << bits) - 1))
            b0 = q[s]
            if b0:
                s += 1 if b0 < 128 else (2 if b0 < 255 else 3)
                modes = q[s]
                for t, name in enumerate(("LL", "OF", "ML")):
                    seen.add((name, ("predefined", "rle", "fse", "repeat")[(modes >> (6 - 2 * t)) & 3]))
        pos += 1 if bt == 1 else bs
        if last:
            break
    seen.add(("frame", "multi-block" if nblocks > 1 else "single-block"))
    return seen


def main():
    lib = C.CDLL("libzstd.so.1")
    lib.ZSTD_createCCtx.restype = C.c_void_p
    lib.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.ZSTD_CCtx_setParameter.restype = C.c_size_t
    lib.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.ZSTD_compress2.restype = C.c_size_t
    lib.ZSTD_freeCCtx.argtypes = [C.c_void_p]
    lib.ZSTD_isError.argtypes = [C.c_size_t]
    lib.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.ZSTD_decompress.restype = C.c_size_t
    lib.ZSTD_versionNumber.restype = C.c_uint
    out = {"libzstd": int(lib.ZSTD_versionNumber()), "fixtures": []}
    for case in CASES:
        raw = raw_of(case)
        cctx = lib.ZSTD_createCCtx()
        assert not lib.ZSTD_isError(lib.ZSTD_CCtx_setParameter(cctx, ZSTD_c_compressionLevel, case["level"]))
        for k, v in case.get("params", {}).items():
            assert not lib.ZSTD_isError(lib.ZSTD_CCtx_setParameter(cctx, k, v))
        cap = len(raw) + len(raw) // 128 + 1024
        dst = C.create_string_buffer(cap)
        src = C.create_string_buffer(raw, max(1, len(raw)))
        r = lib.ZSTD_compress2(cctx, dst, cap, src, len(raw))
        assert not lib.ZSTD_isError(r)
        lib.ZSTD_freeCCtx(cctx)
        frame = dst.raw[:r]
        if case.get("twice"):
            frame = frame + frame
        if not case.get("twice"):                            # the real library reads it back
            chk = C.create_string_buffer(max(1, len(raw)))
            assert lib.ZSTD_decompress(chk, max(1, len(raw)), frame, len(frame)) == len(raw) and chk.raw[:len(raw)] == raw
        entry = {k: v for k, v in case.items() if k not in ("params", "twice")}
        entry["params"] = {str(k): v for k, v in case.get("params", {}).items()}
        entry["taken"] = case.get("taken", True)
        entry["raw_sha256"] = hashlib.sha256(raw).hexdigest()
        entry["raw_bytes"] = len(raw)
        entry["frame"] = base64.b64encode(frame).decode()
        entry["modes"] = sorted("%s:%s" % m for m in walk(frame))
        out["fixtures"].append(entry)
    path = os.path.join(HERE, "zstd_fixtures.json")
    with open(path, "w") as f:                               # one fixture a line
        f.write('{"libzstd": %d, "fixtures": [\n' % out["libzstd"])
        f.write(",\n".join(json.dumps(e) for e in out["fixtures"]))
        f.write("\n]}\n")
    union = sorted(set(m for e in out["fixtures"] for m in e["modes"]))
    print(f"{len(out['fixtures'])} frames, {os.path.getsize(path)} bytes -> {path}\nmodes: {union}")


if __name__ == "__main__":
    main()
