"""zlib streams for tests/test_inflate_plan.py and tests/test_gpu_inflate_decode.py: streams the real zlib writes at test time,
edge streams it never writes (hand-assembled by a small bit writer), damaged streams, and the packing of a batch."""
import zlib

import numpy as np

from aggfly_amd import codec, synth

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_BITS = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_BITS = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bits:
    """Deflate's bit order (RFC 1951 §3.1.1): values least significant bit first, Huffman codes most significant bit first."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n

    def code(self, c, n):
        self.put(int(format(c, f"0{n}b")[::-1], 2), n)

    def header(self, final, btype):
        self.put(final, 1)
        self.put(btype, 2)

    def stored(self, final, data, nlen=None):
        self.header(final, 0)
        self.n = (self.n + 7) // 8 * 8
        self.put(len(data), 16)
        self.put((~len(data) & 0xffff) if nlen is None else nlen, 16)
        for b in data:
            self.put(b, 8)

    def fixed_sym(self, s):                      # literal/length symbol of the fixed code (§3.2.6)
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def fixed_match(self, length, dist):
        ls = max(i for i in range(29) if LEN_BASE[i] <= length and (i < 28 or length == 258))
        self.fixed_sym(257 + ls)
        self.put(length - LEN_BASE[ls], LEN_BITS[ls])
        ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.code(ds, 5)
        self.put(dist - DIST_BASE[ds], DIST_BITS[ds])

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def wrap(deflate: bytes, raw: bytes) -> bytes:
    return b"\x78\x9c" + deflate + zlib.adler32(raw).to_bytes(4, "big")


def shuffle(raw: bytes, ts: int) -> bytes:
    a = np.frombuffer(raw, dtype=np.uint8)
    n = a.size // ts
    return a[:n * ts].reshape(n, ts).T.tobytes() + a[n * ts:].tobytes()


def cobj(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, flush_at=None, flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if flush_at is None:
        return c.compress(raw) + c.flush()
    return c.compress(raw[:flush_at]) + c.flush(flush) + c.compress(raw[flush_at:]) + c.flush()


CUBE = synth.temperature_cube(48, 26, 40, dtype=np.float32, seed=3)
SHUF = shuffle(CUBE.tobytes(), 4)                # 199,680 bytes, ~155 KB at every level: many dynamic blocks


def far_match_stream():
    """A stored block of 32,768 bytes, then a fixed block with a match of length 258 at distance 32,768."""
    noise = np.random.default_rng(11).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    b = Bits()
    b.stored(0, noise)
    b.header(1, 1)
    b.fixed_match(258, 32768)
    b.fixed_sym(256)
    raw = noise + noise[:258]
    return wrap(b.bytes(), raw), raw


def good_streams():
    """(name, stream, decoded bytes) of every stream of the issue's test 1, and a few small ones for the fuzzer."""
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()
    out = [("empty", zlib.compress(b""), b""), ("one byte", zlib.compress(b"q"), b"q"),
           ("noise level 0", zlib.compress(noise, 0), noise), ("constant", zlib.compress(b"\x07" * 100000), b"\x07" * 100000)]
    for lvl in (1, 4, 6, 9):
        out.append((f"cube level {lvl}", zlib.compress(SHUF, lvl), SHUF))
    for name, st in (("Z_FIXED", zlib.Z_FIXED), ("Z_HUFFMAN_ONLY", zlib.Z_HUFFMAN_ONLY), ("Z_RLE", zlib.Z_RLE)):
        out.append((f"cube {name}", cobj(SHUF, strategy=st), SHUF))
    out.append(("cube wbits 9", cobj(SHUF, wbits=9), SHUF))
    out.append(("cube sync flush", cobj(SHUF, flush_at=90001, flush=zlib.Z_SYNC_FLUSH), SHUF))
    out.append(("cube full flush", cobj(SHUF, flush_at=90001, flush=zlib.Z_FULL_FLUSH), SHUF))
    far, far_raw = far_match_stream()
    out.append(("far match", far, far_raw))
    part = SHUF[100000:120000]
    for lvl in (1, 6, 9):
        out.append((f"part level {lvl}", zlib.compress(part, lvl), part))
    out.append(("part Z_FIXED", cobj(part, strategy=zlib.Z_FIXED), part))
    out.append(("part sync flush", cobj(part, flush_at=7001), part))
    return out


def block_types(stream: bytes):
    """The BTYPE of every deflate block of a valid zlib stream, found by a plain walk of its symbols (RFC 1951 §3.2.3)."""
    data = stream[2:-4] + b"\0\0\0\0"
    pos, out = 0, []

    def take(n):
        nonlocal pos
        v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    def table(lens):                             # {(length, code): symbol}
        code, tab = 0, {}
        for ln in range(1, 16):
            for sym, l_ in enumerate(lens):
                if l_ == ln:
                    tab[(ln, code)] = sym
                    code += 1
            code <<= 1
        return tab

    def symbol(tab):
        code = 0
        for ln in range(1, 16):
            code = (code << 1) | take(1)
            if (ln, code) in tab:
                return tab[(ln, code)]
        raise ValueError("no code")

    final = 0
    while not final:
        final, btype = take(1), take(2)
        out.append(btype)
        if btype == 0:
            pos = (pos + 7) // 8 * 8
            n = take(16)
            pos += 16 + 8 * n
            continue
        if btype == 1:
            lt, dt = table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), table([5] * 32)
        else:
            nl, nd, nc = take(5) + 257, take(5) + 1, take(4) + 4
            cl = [0] * 19
            for i in range(nc):
                cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][i]] = take(3)
            ct, lens = table(cl), []
            while len(lens) < nl + nd:
                sy = symbol(ct)
                if sy < 16:
                    lens.append(sy)
                elif sy == 16:
                    lens += [lens[-1]] * (3 + take(2))
                else:
                    lens += [0] * (3 + take(3) if sy == 17 else 11 + take(7))
            lt, dt = table(lens[:nl]), table(lens[nl:])
        while True:
            sy = symbol(lt)
            if sy == 256:
                break
            if sy > 256:
                take(LEN_BITS[sy - 257])
                take(DIST_BITS[symbol(dt)])
    return out


def _fixed(items, final_eob=True):
    b = Bits()
    b.header(1, 1)
    for it in items:
        it(b)
    if final_eob:
        b.fixed_sym(256)
    return b.bytes()


def refused_streams():
    """(name, stream, planned size): streams the decoder must refuse."""
    out = []
    out.append(("distance before the start", wrap(_fixed([lambda b: b.fixed_sym(97), lambda b: b.fixed_match(3, 2)]), b"aaaa"), 4))
    out.append(("symbol 286", wrap(_fixed([lambda b: b.fixed_sym(97), lambda b: b.fixed_sym(286)]), b"a"), 1))

    def code30(b):
        b.fixed_sym(257)
        b.code(30, 5)
    out.append(("distance code 30", wrap(_fixed([lambda b: b.fixed_sym(97), code30]), b"aaaa"), 4))
    b = Bits()
    b.stored(1, b"hello", nlen=0x1234)
    out.append(("LEN != ~NLEN", wrap(b.bytes(), b"hello"), 5))
    b = Bits()                                   # dynamic block whose 19 code length codes all have length 1
    b.header(1, 2)
    b.put(0, 5); b.put(0, 5); b.put(15, 4)
    for _ in range(19):
        b.put(1, 3)
    b.put(0, 32)
    out.append(("over-subscribed code length code", wrap(b.bytes(), b"a"), 1))
    b = Bits()                                   # dynamic block: literals 0 and 1 have codes, 256 has none
    b.header(1, 2)
    b.put(0, 5); b.put(0, 5); b.put(14, 4)       # 257 literal/length codes, 1 distance code, 18 code length codes
    cl = {18: 2, 0: 2, 1: 1}                      # canonical: 1 -> 0, 0 -> 10, 18 -> 11
    for s in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1]:
        b.put(cl.get(s, 0), 3)
    b.code(0, 1); b.code(0, 1)                   # lengths of literals 0 and 1: 1
    b.code(3, 2); b.put(138 - 11, 7)             # 138 zeros
    b.code(3, 2); b.put(118 - 11, 7)             # 118 zeros: 258 lengths, none for symbol 256
    b.put(0, 16)
    out.append(("no end-of-block code", wrap(b.bytes(), b"\x00"), 1))
    part = SHUF[:5000]
    good = zlib.compress(part, 6)
    out.append(("truncated", good[:len(good) // 2], len(part)))
    out.append(("wrong Adler-32", good[:-1] + bytes([good[-1] ^ 1]), len(part)))
    out.append(("one byte short of the plan", good, len(part) + 1))
    out.append(("one byte long for the plan", good, len(part) - 1))
    return out


def mutate(rng, it, stream: bytes) -> bytes:
    """Cut or mutated as tests/test_zstd_plan.py does, the two header bytes left alone."""
    b = bytearray(stream)
    kind = it % 4
    if kind == 0:
        return bytes(b[:int(rng.integers(1, len(b)))])
    for _ in range(int(rng.integers(1, 4))):
        j = int(rng.integers(2, len(b))) if kind < 3 else int(rng.integers(2, min(len(b), 40)))
        b[j] = int(rng.integers(256)) if kind != 2 else b[j] ^ (1 << int(rng.integers(8)))
    return bytes(b)


PAD = 48                                         # canary bytes between destinations


def pack(streams, sizes):
    """The streams back to back (64-byte aligned) -> (base, comp_off, comp_size, out_off, out bytes with canary gaps)."""
    offs, pos = [], 0
    for s in streams:
        offs.append(pos)
        pos += (len(s) + 63) // 64 * 64
    base = np.zeros(max(pos, 64), dtype=np.uint8)
    for o, s in zip(offs, streams):
        base[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    sizes = np.asarray(sizes, dtype=np.int64)
    oo = np.cumsum(np.concatenate([[PAD], sizes[:-1] + PAD])).astype(np.int64)
    return base, np.array(offs, dtype=np.int64), np.array([len(s) for s in streams], dtype=np.int64), oo, int(oo[-1] + sizes[-1] + PAD)


def plan(streams, sizes, typesize=1, strict=True):
    base, co, cs, oo, nout = pack(streams, sizes)
    st = np.zeros(len(streams) + 1, dtype=codec.INFLATE_STREAM)
    sh = np.zeros(len(streams) + 1, dtype=codec.SHUFFLE_BLOCK)
    p = codec.inflate_plan(base, co, cs, oo, np.asarray(sizes, dtype=np.int64), st, sh, typesize=typesize, strict=strict)
    return base, co, cs, oo, nout, st, sh, p


def canary_mask(nout, oo, sizes):
    m = np.ones(nout, dtype=bool)
    for o, n in zip(oo, sizes):
        m[o:o + n] = False
    return m


def damaged_streams(n=32):
    """A fixed set: the refused streams, then seeded mutations of the small good streams that the planner accepts and zlib
    refuses.  -> [(stream, planned size)]"""
    out = [(s, n_) for _, s, n_ in refused_streams()]
    small = [(s, r) for _, s, r in good_streams() if 64 < len(s) < 65536]
    rng = np.random.default_rng(99)
    it = 0
    while len(out) < n:
        s, raw = small[int(rng.integers(len(small)))]
        m = mutate(rng, it, s)
        it += 1
        try:
            zlib.decompress(m)
        except zlib.error:
            out.append((m, len(raw)))
    return out[:n]
