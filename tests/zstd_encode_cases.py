"""Inputs for the Zstandard block encoder of aggfly_amd/csrc/zstd_encode_pass.h (`afcodec_zstd_encode_block_emulate` on the host,
`k_zstd_encode_blocks` on the GPU), each named for the encoder line it exercises.

A case is (name, input bytes, expectation): the expectation is a dict of facts that the encoder's rules imply for this input —
``block``: "raw" / "rle" / "comp", the block's type; ``shorter``: the block is shorter than its input; ``census``: entries the strict
decoder's census (tests/zstd_frames.decode) must hold for this block; ``nseq``: its number of sequences; ``lit_size``: its literals.
tests/test_zstd_encode.py checks them; tests/test_gpu_zstd_encode.py holds the kernel's bytes to the emulation's.

The encoder finds a run at its SECOND byte (the 4-byte word at p equals the one at p - 1), and it inserts no position behind the first
match of a round, so a run between two copies of a pattern leaves the first copy in the hash table: the way to an offset of nearly the
whole block.

Run as a program it writes the catalogue to a file for tests/zstd_encode_check.c (`make zstd_encode_check_san`): u32 count, then per
case u32 length and the bytes.
"""
import struct
import sys

import numpy as np

KIB = 1024
BLOCK = 128 * KIB
RUN = 250                                         # the byte of the runs; `noise` stays below it


def rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def noise(n: int, seed: int, top: int = 200) -> bytes:
    """Bytes 0 .. top - 1 with no 4-byte word twice (checked), so that the encoder finds no match inside: all literals."""
    rng = np.random.default_rng(seed)
    while True:
        b = rng.integers(0, top, n, dtype=np.uint8)
        if n < 4:
            return b.tobytes()
        w = b[:-3].astype(np.uint32) | (b[1:-2].astype(np.uint32) << 8) | (b[2:-1].astype(np.uint32) << 16) | (b[3:].astype(np.uint32) << 24)
        if len(np.unique(w)) == len(w):
            return b.tobytes()


def pattern(period: int, n: int) -> bytes:
    unit = bytes((37 * i + 11) % 251 for i in range(period))
    return (unit * (n // period + 1))[:n]


def draw(symbols, weights, n: int, seed: int) -> bytes:
    """n bytes drawn from `symbols` with the given relative weights; every symbol at least once."""
    rng = np.random.default_rng(seed)
    p = np.asarray(weights, dtype=np.float64)
    out = rng.choice(np.asarray(symbols, dtype=np.uint8), size=n, p=p / p.sum())
    out[rng.permutation(n)[:len(symbols)]] = np.asarray(symbols, dtype=np.uint8)
    return out.tobytes()


def counted(counts: dict, seed: int) -> bytes:
    """Exactly counts[symbol] bytes of every symbol, in a seeded order."""
    out = np.concatenate([np.full(c, s, dtype=np.uint8) for s, c in counts.items()])
    return out[np.random.default_rng(seed).permutation(len(out))].tobytes()


def shuffle(data: bytes, typesize: int) -> bytes:
    a = np.frombuffer(data, dtype=np.uint8)
    n = len(a) // typesize
    return a[:n * typesize].reshape(n, typesize).T.tobytes() + a[n * typesize:].tobytes()


def mix(seed: int) -> bytes:
    """A float32, quantised float32, int16 or float64 temperature-like field after the byte shuffle; the length is no multiple of 64."""
    rng = np.random.default_rng(1000 + seed)
    kind = seed % 4
    m = int(rng.integers(300, 4000))
    ts = (4, 4, 2, 8)[kind]
    while (m * ts) % 64 == 0:
        m += 1
    x = 280.0 + 15.0 * np.sin(np.arange(m) * float(rng.uniform(0.001, 0.05))) + rng.normal(0.0, float(rng.uniform(0.01, 2.0)), m)
    if kind == 0:
        a = x.astype("<f4")
    elif kind == 1:
        a = (np.round(x.astype("<f4") / 0.01) * 0.01).astype("<f4")
    elif kind == 2:
        a = np.round((x - 280.0) / 0.002).astype("<i2")
    else:
        a = x.astype("<f8")
    return shuffle(a.tobytes(), ts)


def sequences(k: int) -> bytes:
    """k pieces of 8 noise bytes and a run of 8: every run is one sequence, and the noise holds no match."""
    nz = noise(8 * k + 8, 4000 + k)
    return b"".join(nz[8 * i:8 * i + 8] + bytes([RUN]) * 8 for i in range(k)) + nz[8 * k:]


def catalogue():
    cases = []
    add = lambda name, data, **expect: cases.append((name, bytes(data), expect))
    for n in (1, 2, 3, 4, 7, 8, 63, 64, 65, 255, 256, 257, BLOCK - 1, BLOCK):
        add(f"len_{n}_run", bytes([RUN]) * n, block="rle", shorter=n > 4)
        add(f"len_{n}_noise", rand(n, n), block="rle" if n == 1 else "raw")
    add("constant_1000", bytes(1000), block="rle", shorter=True)
    add("two_values", draw([3, 200], [3, 1], 6000, 1), block="comp", shorter=True)
    for top in (127, 128, 129):                                                        # the direct description ends at symbol 128
        add(f"last_symbol_{top}", draw(list(range(16)) + [top], [2.0 ** -(i // 2) for i in range(17)], 8000, top), block="comp", shorter=True,
            census=[("lit", "huf", 4)] + ([("huf_desc", "fse", 6)] if top > 128 else []))
    for k in (8, 9):                                                                   # so few weights that the direct form is the shorter one
        add(f"few_symbols_{k}", draw(list(range(k)), [1.5 ** -i for i in range(k)], 4000, k), block="comp", shorter=True,
            census=[("huf_desc", "direct", "odd" if (k - 1) & 1 else "even")])
    add("all_256_skewed", draw(list(range(256)), [(1 + i) ** -1.3 for i in range(256)], 64 * KIB, 2), block="comp", shorter=True,
        census=[("huf_desc", "fse", 6), ("huf_symbols", 256), ("lit", "huf", 4)])
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    fib[-1] += BLOCK - sum(fib)
    add("fibonacci_24", counted({10 * i + 3: c for i, c in enumerate(fib)}, 3), block="comp", shorter=True, census=[("huf_depth", 11)])
    add("count_1_beside_heavy", counted({5: 3000, 6: 2000, 77: 1}, 4), block="comp", shorter=True)
    for n in (1023, 1024, 16383, 16384):                                               # the borders of the literals size formats
        add(f"literals_{n}", noise(n, n, 64 if n < 2000 else 200), block="comp", shorter=True, lit_size=n, nseq=0,
            census=[("lit", "huf", 1 if n < 1024 else 4), ("lit_hdr", "coded", 3 if n < 1024 else 4 if n < 16384 else 5)])
    for period in (2, 3, 7, 64):
        add(f"period_{period}", pattern(period, 20000), block="comp", shorter=True, nseq=1)
    head = noise(64, 99)
    add("pattern_ends_noise", head + rand(BLOCK - 128, 5) + head)                      # (the table has long forgotten the pattern)
    add("pattern_ends_run", head + bytes([RUN]) * (BLOCK - 128) + head, block="comp", shorter=True,
        census=[("code", "OF", 16)])                                                    # offset 131008: the largest code a block can reach
    add("match_70000", noise(20, 6) + bytes([RUN]) * 70000 + noise(20, 7), block="comp", shorter=True, census=[("code", "ML", 52)])
    add("literal_run_66000", noise(66000, 8, 256) + bytes([RUN]) * 100, block="comp", shorter=True, census=[("code", "LL", 35), ("lit", "raw", 1)])
    add("sequences_127", sequences(127), block="comp", shorter=True, nseq=127, census=[("nseq_form", 1)])
    add("sequences_128", sequences(128), block="comp", shorter=True, nseq=128, census=[("nseq_form", 2)])
    add("random_64k", rand(64 * KIB, 9), block="raw")
    for seed in range(100):
        add(f"mix_{seed}", mix(seed))
    return cases


def small_dataset(dtype="float32", shape=(100, 37, 29), seed=11):
    """The cube of the route tests: with chunks (96, 37, 29) one chunk above 256 KiB (float32), a short last Blosc block and edge chunks."""
    import pandas as pd

    import aggfly_amd as af
    rng = np.random.default_rng(seed)
    t, ny, nx = shape
    x = 280.0 + 12.0 * np.sin(np.arange(t)[:, None, None] * 0.26) + np.linspace(-8, 8, ny)[None, :, None] + rng.normal(0.0, 0.7, shape)
    if np.dtype(dtype).kind == "f":
        cube = x.astype(dtype)
        cube[3, 5, 7] = np.nan
    else:
        cube = np.round((x - 280.0) / 0.002).astype(dtype)
    time = pd.date_range("2001-01-01", periods=t, freq="h")
    return af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                   {"time": time, "latitude": 30 + 0.25 * np.arange(ny), "longitude": 230 + 0.25 * np.arange(nx)}), lon_is_360=True)


def tree_hashes(root: str) -> dict:
    """relative path -> sha256 of every file under root."""
    import hashlib
    import os
    out = {}
    for base, _, files in os.walk(root):
        for fn in files:
            full = os.path.join(base, fn)
            out[os.path.relpath(full, root).replace(os.sep, "/")] = hashlib.sha256(open(full, "rb").read()).hexdigest()
    return dict(sorted(out.items()))


HOST_ROUTE_STORES = [dict(compress=c, zarr_format=f, shards=s) for c in ("blosc-zstd", "zstd")
                     for f, s in ((2, None), (3, None), (3, {"time": 96, "latitude": 37, "longitude": 29}))]
SMALL_CHUNKS = {"time": 96, "latitude": 37, "longitude": 29}


def dump(path: str):
    cases = catalogue()
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for _, data, _ in cases:
            f.write(struct.pack("<I", len(data)))
            f.write(data)
    return len(cases)


if __name__ == "__main__":
    print(f"{dump(sys.argv[1])} inputs -> {sys.argv[1]}")
