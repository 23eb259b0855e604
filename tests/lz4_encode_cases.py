"""Inputs for the LZ4 block encoder of aggfly_amd/csrc/lz4_encode_pass.h (`afcodec_lz4_encode_emulate` on the host,
`k_lz4_encode_streams` on the GPU), each named for the encoder line it exercises.

A case is (name, input bytes, expectation): the expectation is None, "stored", or a dict of facts about the parsed stream that the
encoder's rules imply for this input — ``litlen`` / ``mlen`` / ``offset``: a sequence with that literal length / match length / offset
is in the stream; ``max_offset``: no offset is larger.  tests/test_lz4_encode.py checks them; tests/test_gpu_lz4_encode.py holds the
kernel's bytes to the emulation's.

The encoder finds a run at its SECOND byte (the 4-byte word at p equals the one at p - 1), so k noise bytes followed by a run of r
equal bytes give one sequence of k + 1 literals and a match of r - 1 bytes at offset 1.

Run as a program it writes the catalogue to a file for tests/lz4_encode_check.c (`make lz4_encode_check_san`): u32 count, then per
case u32 length and the bytes.
"""
import struct
import sys

import numpy as np

KIB = 1024
RUN = 250                                         # the byte of the runs; noise stays below it


def noise(n: int, seed: int) -> bytes:
    """Bytes 0 .. 199 with no 4-byte word twice (checked), so that the encoder finds no match inside."""
    rng = np.random.default_rng(seed)
    while True:
        b = rng.integers(0, 200, n, dtype=np.uint8).tobytes()
        words = {b[i:i + 4] for i in range(max(0, n - 3))}
        if len(words) == max(0, n - 3) and all(b[i] != b[i + 1] for i in range(n - 1)):
            return b


def rand(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def pattern(period: int, n: int) -> bytes:
    unit = bytes((37 * i + 11) % 251 for i in range(period))
    return (unit * (n // period + 1))[:n]


def mix(seed: int) -> bytes:
    """Runs, repeats of earlier pieces and noise; the length is no multiple of 64."""
    rng = np.random.default_rng(seed)
    out = bytearray()
    want = int(rng.integers(1, 6000))
    while len(out) < want:
        kind = int(rng.integers(0, 4))
        k = int(rng.integers(1, 400))
        if kind == 0:
            out += bytes([int(rng.integers(0, 256))]) * k
        elif kind == 1 and out:
            a = int(rng.integers(0, len(out)))
            for i in range(k):                     # (an overlapping repeat when a + k runs past the end)
                out.append(out[a + i])
        elif kind == 2:
            out += rng.integers(0, 256, k, dtype=np.uint8).tobytes()
        else:
            out += rng.integers(0, 4, k, dtype=np.uint8).tobytes()
    if len(out) % 64 == 0:
        out.append(7)
    return bytes(out)


def sparse_far(distance: int) -> bytes:
    """64 noise bytes, a run up to `distance`, the 64 bytes again, a short run of another byte (the first run's word is in the table
    too): the run's positions are not inserted, so the table still holds the first 64 when the second arrive — candidates at exactly
    `distance`."""
    head = noise(64, 99)
    return head + bytes([RUN]) * (distance - 64) + head + bytes([RUN + 1]) * 40


def catalogue():
    cases = []
    add = lambda name, data, expect=None: cases.append((name, bytes(data), expect))
    for n in (0, 1, 4, 11, 12, 13, 63, 64, 65, 127, 128):
        add(f"len_{n}_run", bytes([RUN]) * n, "stored" if n < 13 else None)            # under 13 bytes: all literals, so stored
        add(f"len_{n}_noise", rand(n, n), "stored")
    for n in (64 * KIB - 1, 64 * KIB, 64 * KIB + 1):
        add(f"constant_{n}", bytes([RUN]) * n, {"offset": 1, "max_offset": 1})
        for period in (2, 3, 7, 64):
            add(f"period_{period}_{n}", pattern(period, n), {"offset": period, "max_offset": period})
    for k in (14, 15, 16, 269, 270, 271):                                              # token nibble 14 / 15, extension bytes 0 / 1 / 255, 0
        add(f"literal_run_{k}", noise(k - 1, k) + bytes([RUN]) * 60 + noise(20, 1000 + k), {"litlen": k, "offset": 1})
    for m in (18, 19, 20, 273, 274, 275):
        add(f"match_length_{m}", noise(20, m) + bytes([RUN]) * (m + 1) + noise(20, 2000 + m), {"mlen": m, "offset": 1})
    add("match_into_last_5", noise(20, 5) + bytes([RUN]) * 40, {"mlen": 40 - 1 - 5})   # clipped 5 bytes before the end
    add("match_in_last_12", bytes([7]) * 100 + noise(30, 12) + bytes([RUN]) * 10, {"max_offset": 1, "last_litlen": 30 + 10})
    add("repeat_at_65535", rand(65535, 1) * 2)                                         # (legal; the table has long forgotten it)
    add("repeat_at_65536", rand(65536, 2) * 2, "stored")
    add("repeats_at_70000_200k", (rand(70000, 3) * 3)[:200 * KIB], "stored")           # positions beyond 64 KiB must not alias
    add("candidate_at_65535", sparse_far(65535), {"offset": 65535})
    add("candidate_at_65536", sparse_far(65536), {"max_offset": 1})
    add("candidate_at_70000", sparse_far(70000), {"max_offset": 1})
    add("random_64k", rand(64 * KIB, 4), "stored")
    for seed in range(300):
        add(f"mix_{seed}", mix(seed))
    return cases


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
