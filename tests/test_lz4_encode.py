"""The LZ4 block encoder of aggfly_amd/csrc/lz4_encode_pass.h on the host, no GPU (`afcodec_lz4_encode_emulate` runs the kernel's
text with its 64 lanes in loops): every input of tests/lz4_encode_cases.py decodes again — by the strict decoder of
tests/lz4_streams.py and by liblz4 —, the parsed stream keeps the block format's end rules and the distance limit, nothing is written
outside the slot, and the Blosc-1 containers assembled from emulated streams (`codec.BloscEncodePlan`) are what `codec.blosc_decode`
reads and what the host encoder lays out.  tests/test_gpu_lz4_encode.py holds the kernel's bytes to these."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lz4_encode_cases as cases_mod            # noqa: E402
import lz4_streams as lz                        # noqa: E402

from aggfly_amd import codec                    # noqa: E402

CASES = cases_mod.catalogue()
_ENCODED = {}


def encoded(name, data):
    """The emulation's stream of a case, computed once."""
    if name not in _ENCODED:
        _ENCODED[name] = codec.lz4_encode_emulate(data)
    return _ENCODED[name]


def parse(stream: bytes):
    """-> [(literal length, offset, match length)] + the last sequence's literal length."""
    p, n, seqs = 0, len(stream), []

    def length(v, p):
        if v == 15:
            while True:
                b = stream[p]
                p += 1
                v += b
                if b != 255:
                    break
        return v, p

    while True:
        token = stream[p]
        L, p = length(token >> 4, p + 1)
        p += L
        if p == n:
            return seqs, L
        off = stream[p] | (stream[p + 1] << 8)
        M, p = length(token & 15, p + 2)
        seqs.append((L, off, M + 4))


def test_the_catalogue_names_every_case_of_the_issue():
    names = {c[0] for c in CASES}
    assert len(names) == len(CASES)
    for n in (0, 1, 4, 11, 12, 13, 63, 64, 65, 127, 128):
        assert f"len_{n}_run" in names and f"len_{n}_noise" in names
    for n in (65535, 65536, 65537):
        assert f"constant_{n}" in names and all(f"period_{p}_{n}" in names for p in (2, 3, 7, 64))
    assert sum(n.startswith("mix_") for n in names) == 300
    assert all(len(d) % 64 for n, d, _ in CASES if n.startswith("mix_"))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stream_decodes_and_keeps_the_block_rules(case):
    name, data, expect = case
    n = len(data)
    s = encoded(name, data)
    assert len(s) <= max(n - 1, 0) or s == data, "csize <= dsize - 1, or stored: csize == dsize with the raw bytes"
    if expect == "stored":
        assert s == data
    if len(s) == n:
        return
    assert lz.decode(s, n) == data
    back = codec.lz4_decode(struct.pack("<i", n) + s, n)
    assert bytes(back) == data, "liblz4"
    seqs, last = parse(s)
    assert all(1 <= off <= 65535 for _, off, _ in seqs)
    assert all(m >= 4 for _, _, m in seqs)
    if seqs:                                                # (a stream of literals alone would have been stored)
        assert last >= 5, "the last 5 bytes are literals"
        start = n - last - seqs[-1][2]
        assert start <= n - 12, "no match starts within the last 12 bytes"
    assert n >= 13, "an input shorter than 13 bytes is all literals (and so stored)"
    if isinstance(expect, dict):
        if "litlen" in expect:
            assert expect["litlen"] in [L for L, _, _ in seqs]
        if "mlen" in expect:
            assert expect["mlen"] in [m for _, _, m in seqs]
        if "offset" in expect:
            assert expect["offset"] in [off for _, off, _ in seqs]
        if "max_offset" in expect:
            assert max(off for _, off, _ in seqs) <= expect["max_offset"]
        if "last_litlen" in expect:
            assert last == expect["last_litlen"]


def test_nothing_is_written_beyond_the_slot():
    lib = codec.load()
    for name, data, _ in CASES:
        n = len(data)
        src = np.frombuffer(data, dtype=np.uint8)
        buf = np.full(n + 128, 0xAB, dtype=np.uint8)
        c = lib.afcodec_lz4_encode_emulate(src.ctypes.data if n else None, n, buf[64:].ctypes.data, n)
        assert 0 <= c <= n, name
        assert (buf[:64] == 0xAB).all() and (buf[64 + n:] == 0xAB).all(), name
        assert buf[64:64 + c].tobytes() == encoded(name, data), name
    small = np.zeros(100, dtype=np.uint8)
    assert lib.afcodec_lz4_encode_emulate(small.ctypes.data, 100, small.ctypes.data, 99) < 0, "a slot under n bytes is refused"


def test_a_constant_plane_stays_small_and_random_bytes_are_stored():
    """A single offset-1 match over 64 KiB needs about 270 bytes (its length extension): under 1 KiB there is room for a few dozen
    sequences, none for an encoder that has stopped finding matches inside a round."""
    by_name = {c[0]: c[1] for c in CASES}
    assert len(encoded("constant_65536", by_name["constant_65536"])) < 1024
    exponent = np.full(65536, 0x41, dtype=np.uint8)
    exponent[::997] = 0x42                                  # the exponent plane of a smooth float field: nearly constant
    assert len(codec.lz4_encode_emulate(exponent)) < 2048
    assert encoded("random_64k", by_name["random_64k"]) == by_name["random_64k"]


def _chunk(nbytes: int, typesize: int, seed: int) -> np.ndarray:
    """Smooth values of `typesize` bytes: compressible planes and noisy ones."""
    rng = np.random.default_rng(seed)
    n = -(-nbytes // typesize)
    v = np.cumsum(rng.integers(-3, 4, n)).astype({1: np.int8, 2: np.int16, 4: np.float32, 8: np.float64}[typesize])
    return v.view(np.uint8)[:nbytes].copy()


def _emulated_containers(raw: np.ndarray, n: int, nbytes: int, typesize: int):
    """The GPU route on the host: shuffle per block record, the emulation per stream record, `assemble_host`."""
    plan = codec.BloscEncodePlan(n, nbytes, typesize)
    tmp = np.zeros_like(raw)
    for b in plan.blocks:
        ts, bs, src = int(b["typesize"]), int(b["bsize"]), raw[b["out_off"]:b["out_off"] + b["bsize"]]
        ne = bs // ts
        dst = tmp[b["tmp_off"]:b["tmp_off"] + bs]
        dst[:ne * ts] = src[:ne * ts].reshape(ne, ts).T.reshape(-1)
        dst[ne * ts:] = src[ne * ts:]
    slots = np.zeros_like(raw)
    csizes = np.zeros(len(plan.streams), dtype=np.int32)
    for i, s in enumerate(plan.streams):
        piece = tmp[s["src_off"]:s["src_off"] + s["dsize"]]
        out = piece.tobytes() if s["to_out"] else codec.lz4_encode_emulate(piece)
        csizes[i] = len(out)
        slots[s["dst_off"]:s["dst_off"] + len(out)] = np.frombuffer(out, dtype=np.uint8)
    return plan, plan.assemble_host(slots, csizes)


@pytest.mark.parametrize("typesize", [1, 2, 4, 8])
@pytest.mark.parametrize("nbytes", [100, 127, 128, 1001, 65536 * 4 - 4, 65536 * 4 + 12])
def test_containers_of_emulated_streams(nbytes, typesize):
    n = 3
    raw = np.concatenate([_chunk(nbytes, typesize, 10 * typesize + i) for i in range(n)])
    plan, chunks = _emulated_containers(raw, n, nbytes, typesize)
    for i, c in enumerate(chunks):
        want = raw[i * nbytes:(i + 1) * nbytes]
        assert bytes(codec.blosc_decode(c)) == want.tobytes()
        host = codec.blosc_encode(want, typesize, shuffle=True)
        a, b = codec.blosc_info(c), codec.blosc_info(host)
        assert {k: a[k] for k in ("nbytes", "blocksize", "typesize", "flags")} == {k: b[k] for k in ("nbytes", "blocksize", "typesize", "flags")}
        nb = plan.n_bstarts                                 # the same block table entries where the streams' sizes agree: its length does
        assert struct.unpack_from("<I", c, 12)[0] == len(c)
        if nb:
            assert struct.unpack_from("<I", c, 16)[0] == struct.unpack_from("<I", host, 16)[0] == 16 + 4 * nb


def test_the_host_encoder_is_unchanged_on_the_committed_fixtures():
    """`afcodec_blosc_encode` shares its block-size lines with the plan now: its output on the encoder fixtures' inputs is what the
    build before wrote (tests/golden/blosc_encode_parent.json: sha256 of every container)."""
    import hashlib
    gold = json.load(open(os.path.join(HERE, "golden", "blosc_encode_parent.json")))
    assert len(gold["cases"]) >= 40
    for g in gold["cases"]:
        raw = _chunk(g["nbytes"], g["typesize"], g["seed"])
        out = codec.blosc_encode(raw, g["typesize"], shuffle=g["shuffle"] == 1, blocksize=g["blocksize"], cname=g["cname"],
                                 bitshuffle=g["shuffle"] == 2)
        assert hashlib.sha256(out).hexdigest() == g["sha256"], g


def test_the_checker_runs_clean_under_the_sanitizers():
    """`make lz4_encode_check_san`: tests/lz4_encode_check.c with blosc1.c under -fsanitize=address,undefined over the catalogue."""
    csrc = os.path.join(os.path.dirname(HERE), "aggfly_amd", "csrc")
    build = os.path.join(csrc, "_build")
    os.makedirs(build, exist_ok=True)
    r = subprocess.run(["make", "-C", csrc, "lz4_encode_check_san"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert f"{len(CASES)} inputs" in r.stdout and " 0 failures" in r.stdout
