"""Hand-built LZ4 block streams for `k_lz4_streams_vec` and `k_unshuffle_blocks` (aggfly_amd/csrc/afhip_lz4_kernels.h).

LZ4's block format has no entropy stage, so a stream can be written down sequence by sequence: `build` does that and nothing
else, `expand` is what the sequence list means, `decode` is a strict decoder of the bytes, `census` restates the kernel's PARSE
DECISIONS (which path every sequence takes; it moves no bytes), `catalogue` names the shapes the kernel branches on, `fuzz`
draws random sequence lists weighted towards them, `damaged` holds streams with one defect each, `blosc_wrap` puts streams
into a Blosc-1 chunk as the byte planes of split blocks and `layout` places records in the buffers of one launch.
Used by tests/test_lz4_streams.py (host) and tests/test_gpu_lz4_streams.py (GPU).

Constants restated from the kernel header (if it changes them, the census test fails, and that is intended):
    constexpr int LZ4_NEAR = 4096;          the ring: output bytes mirrored in LDS
    a window = the 64 bytes at the read position (one wave, a byte per lane); lane < 32 && nxt <= 64 in token_walk_lifted
    if (offg <= NEAR - 64)                  the generic near path
    far = todo && srcpos < op + r0 + 64 - NEAR
"""
from __future__ import annotations

import struct
import zlib
from collections import Counter

import numpy as np

NEAR = 4096
WINDOW = 64
MAX_TOKENS = 32
GUARD = 64

CLASSES = ("rounds>1", "fast_overlap", "fast_same_round_source", "fast_far", "fast_far_unacked", "generic_near_short_period",
           "generic_near", "generic_far_plain", "generic_far_overlap", "generic_ext_scan_two_passes", "literal_jump_3_lines",
           "literal_copy_from_window", "literal_copy_from_stream", "final_in_window", "final_generic", "ring_wrap_inside_match")


# ---------------------------------------------------------------------------------------------------------------------
# the format
# ---------------------------------------------------------------------------------------------------------------------
def _ext(n: int) -> bytes:
    """The extension bytes of a length field whose nibble is 15: n - 15 as a chain of 255s and a last byte < 255."""
    q, r = divmod(n - 15, 255)
    return b"\xff" * q + bytes([r])


def build(seqs, tail) -> bytes:
    """``seqs`` = [(literals, offset, match_len)], ``tail`` = the final literals (None: no final sequence, for damaged streams)."""
    out = bytearray()
    for lit, off, m in seqs:
        assert m >= 4 and 0 <= off <= 0xFFFF
        out.append((min(len(lit), 15) << 4) | min(m - 4, 15))
        if len(lit) >= 15:
            out += _ext(len(lit))
        out += lit
        out += struct.pack("<H", off)
        if m - 4 >= 15:
            out += _ext(m - 4)
    if tail is not None:
        out.append(min(len(tail), 15) << 4)
        if len(tail) >= 15:
            out += _ext(len(tail))
        out += tail
    return bytes(out)


def _repeat(out: bytearray, off: int, m: int):
    start = len(out) - off
    if off >= m:
        out += out[start:start + m]
    else:                                               # overlapping: the last `off` bytes, repeated
        pat = bytes(out[start:])
        out += (pat * (m // off + 1))[:m]


def expand(seqs, tail) -> bytes:
    """What the sequence list means, with no stream in between."""
    out = bytearray()
    for lit, off, m in seqs:
        out += lit
        assert 1 <= off <= len(out), "the list itself is invalid"
        _repeat(out, off, m)
    out += tail
    return bytes(out)


def conformant(seqs, tail) -> bool:
    """The end-of-block rule liblz4 enforces: the last 5 bytes are literals, and the last match starts 12 bytes before the end."""
    return len(tail) >= 5 and (not seqs or seqs[-1][2] + len(tail) >= 12)


class StreamError(ValueError):
    pass


def decode(stream: bytes, dsize: int) -> bytes:
    """Strict decoder of one block: raises `StreamError` on offset 0, an offset before the start, input or output overrun, a
    stream that ends on a match, or a decoded size other than ``dsize``."""
    n, p, out = len(stream), 0, bytearray()

    def length(v, p):
        if v == 15:
            while True:
                if p >= n:
                    raise StreamError("input ends inside a length extension")
                b = stream[p]
                p += 1
                v += b
                if b != 255:
                    break
        return v, p

    if n == 0:
        raise StreamError("empty stream")
    while True:
        if p >= n:
            raise StreamError("the stream ends on a match")
        token = stream[p]
        L, p = length(token >> 4, p + 1)
        if p + L > n:
            raise StreamError("literals beyond the input")
        if len(out) + L > dsize:
            raise StreamError("literals beyond the output")
        out += stream[p:p + L]
        p += L
        if p == n:
            break
        if p + 2 > n:
            raise StreamError("input ends inside an offset")
        off = stream[p] | (stream[p + 1] << 8)
        M, p = length(token & 15, p + 2)
        M += 4
        if off == 0:
            raise StreamError("offset 0")
        if off > len(out):
            raise StreamError("offset before the start")
        if len(out) + M > dsize:
            raise StreamError("match beyond the output")
        _repeat(out, off, M)
    if len(out) != dsize:
        raise StreamError(f"decoded {len(out)} bytes, not {dsize}")
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# the kernel's parse decisions
# ---------------------------------------------------------------------------------------------------------------------
def _speculate(s: bytes, p: int, i: int, wl: int):
    """Lane i of the window at p: (L, off, M, nx) if a sequence that starts there fits the window, else None."""
    csize = len(s)

    def w(k):                                           # a field past the window's valid bytes makes nx > wl
        return s[p + k] if k < wl else None
    t = w(i)
    if t is None:
        return None
    L, ls = t >> 4, i + 1
    if L == 15:
        b1 = w(i + 1)
        if b1 is None or b1 == 255:
            return None
        L, ls = 15 + b1, i + 2
    opos = ls + L
    lo, hi = w(opos), w(opos + 1)
    if lo is None or hi is None:
        return None
    M, nx = (t & 15) + 4, opos + 2
    if (t & 15) == 15:
        e = w(opos + 2)
        if e is None or e == 255:
            return None
        M, nx = 19 + e, opos + 3
    if nx > wl or p + nx >= csize:
        return None
    return L, lo | (hi << 8), M, nx


def _mod_range(a: int, b: int, off: int):
    """min and max of (i mod off) over a <= i <= b."""
    if b - a + 1 >= off or a % off > b % off:
        return 0, off - 1
    return a % off, b % off


def census(stream: bytes, dsize: int) -> Counter:
    """Walks a VALID stream as `k_lz4_streams_vec` does and counts the paths taken (`CLASSES`, ``window_tokens=k``, and the
    totals ``windows``, ``fast_sequences``, ``generic_sequences``, ``line_shift_twice``, and ``read_residue=r`` / ``window_residue=r``:
    the read position mod 64 at every turn of the loop / at every window that holds a sequence)."""
    s, csize = stream, len(stream)
    cnt = Counter()
    p = op = acked = lk = 0

    def ext_scan(q):                                    # the 64-lane scan of a length extension -> (value added, q after)
        add, passes = 0, 0
        while True:
            passes += 1
            k = 0
            while k < 64 and q + k < csize and s[q + k] == 255:
                k += 1
            if k < 64:
                assert q + k < csize
                if passes > 1:
                    cnt["generic_ext_scan_two_passes"] += 1
                return add + 255 * k + s[q + k], q + k + 1
            add += 255 * 64
            q += 64

    while True:
        assert p < csize
        cnt[f"read_residue={p & 63}"] += 1              # where in its 64-byte line the window is cut
        if (p >> 6) - lk > 2:
            cnt["literal_jump_3_lines"] += 1
            lk = p >> 6
        elif (p >> 6) - lk == 2:
            cnt["line_shift_twice"] += 1
        lk = max(lk, p >> 6)
        wl = min(WINDOW, csize - p)
        toks, i = [], 0
        while i < WINDOW and len(toks) < MAX_TOKENS:
            q = _speculate(s, p, i, wl)
            if q is None:
                break
            toks.append(q)
            i = q[3]
        if toks:
            cnt["windows"] += 1
            cnt[f"window_residue={p & 63}"] += 1
            cnt[f"window_tokens={len(toks)}"] += 1
            cnt["fast_sequences"] += len(toks)
            tot = sum(L + M for L, _, M, _ in toks)
            assert tot <= dsize - op
            if tot > 64:
                cnt["rounds>1"] += 1
            far_rounds = {}                             # round -> (any far lane, any far lane with srcpos >= acked at that round)
            drel = 0
            for L, off, M, _ in toks:
                m0 = op + drel + L                      # first match byte
                assert 1 <= off <= m0
                if M > off:
                    cnt["fast_overlap"] += 1
                if (m0 >> 12) != ((m0 + M - 1) >> 12):
                    cnt["ring_wrap_inside_match"] += 1
                same = False
                for r0 in range((drel + L) // 64 * 64, drel + L + M, 64):
                    a, b = max(op + r0, m0) - m0, min(op + r0 + 63, m0 + M - 1) - m0       # match bytes a..b of this round
                    los, his = [], []                   # source of byte i: m0 - off + (i < off ? i : i mod off)
                    if a < off:
                        los.append(a)
                        his.append(min(b, off - 1))
                    if b >= off:
                        mn, mx = _mod_range(max(a, off), b, off)
                        los.append(mn)
                        his.append(mx)
                    lo, hi = m0 - off + min(los), m0 - off + max(his)
                    same |= hi >= op + r0
                    if lo < op + r0 + 64 - NEAR:        # (far sources come from matches shorter than their offset: one range)
                        far_rounds[r0] = max(far_rounds.get(r0, -1), min(hi, op + r0 + 64 - NEAR - 1))
                if same:
                    cnt["fast_same_round_source"] += 1
                drel += L + M
            for r0 in sorted(far_rounds):
                cnt["fast_far"] += 1
                if far_rounds[r0] >= acked:
                    cnt["fast_far_unacked"] += 1
                    acked = op + r0
            p += toks[-1][3]
            op += tot
            continue
        # generic: one sequence
        cnt["generic_sequences"] += 1
        token = s[p]
        Lg, hdr, window_ok = token >> 4, 1, True
        if Lg == 15:
            add, q = ext_scan(p + 1)
            Lg += add
            hdr, window_ok = q - p, False
        assert Lg <= dsize - op and p + hdr + Lg <= csize
        last = p + hdr + Lg >= csize
        from_window = window_ok and 1 + Lg <= wl
        if Lg:
            cnt["literal_copy_from_window" if from_window else "literal_copy_from_stream"] += 1
        if last:
            cnt["final_in_window" if from_window else "final_generic"] += 1
        p += hdr + Lg
        op += Lg
        if last:
            break
        assert p + 2 <= csize
        offg = s[p] | (s[p + 1] << 8)
        p += 2
        Mg = (token & 15) + 4
        if (token & 15) == 15:
            add, p = ext_scan(p)
            Mg += add
        assert 1 <= offg <= op and Mg <= dsize - op
        if (op >> 12) != ((op + Mg - 1) >> 12):
            cnt["ring_wrap_inside_match"] += 1
        if offg <= NEAR - 64:
            cnt["generic_near_short_period" if offg < 64 else "generic_near"] += 1
        else:
            if op - offg + min(Mg, offg) > acked:
                acked = op
            if offg >= Mg:
                cnt["generic_far_plain"] += 1
            else:
                cnt["generic_far_overlap"] += 1
                acked = op + Mg
        op += Mg
    assert op == dsize
    return cnt


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------
class _Case:
    """Collects the sequences of one case; the literals are random bytes seeded by the case's name."""

    def __init__(self, name):
        self.name, self.seqs, self.n = name, [], 0
        self.rng = np.random.default_rng(zlib.crc32(name.encode()))

    def lit(self, k):
        return self.rng.bytes(k) if k else b""

    def seq(self, L, off, M):
        assert 1 <= off <= self.n + L and M >= 4, (self.name, L, off, M, self.n)
        self.seqs.append((self.lit(L), off, M))
        self.n += L + M
        return self

    def dense(self, k, off=3):
        """k short sequences, 4 to 6 stream bytes each"""
        for j in range(k):
            self.seq(1 + j % 3, min(off + j % 4, self.n + 1), 4 + j % 5)
        return self

    def done(self, tail=12):
        t = self.lit(tail)
        assert conformant(self.seqs, t), self.name
        return self.name, self.seqs, t


def _group(c: _Case, k: int, off_of=lambda j: 3 + j % 9, m_of=lambda j: 4 + (5 * j) % 15):
    """k sequences that fill one 64-byte window when the read position is at their first token: k - 1 of three bytes and a
    last one whose literals take the rest."""
    for j in range(k - 1):
        c.seq(0, off_of(j), m_of(j))
    rest = WINDOW - 3 * k
    c.seq(rest if rest < 15 else rest - 1, 5, 6)


def residue_prefix(k: int) -> int:
    """The fewest literals (>= 4, for a match of offset 4) of a first sequence (L, 4, 274) after which the next token is stream byte
    k mod 64: token, an extension byte from 15 literals on, the literals, two offset bytes, the extension 255, 0.  That second
    extension byte sends the sequence down the generic path alone, so the kernel's next read position is exactly that token.
    (5 + L skips 20, where the literals' extension byte appears: k = 20 is reached a line later, and so is k < 9.)"""
    return next(L for L in range(4, 4 + 2 * WINDOW) if (5 + L + (L >= 15)) % WINDOW == k)


def catalogue():
    """-> [(name, seqs, tail)], every one conformant."""
    out = []

    def add(c, tail=12):
        out.append(c.done(tail))

    # ---- literal length ----
    two_pass = 15 + 255 * 64
    for L in (0, 1, 14, 15, 16, 59, 60, 61, 62, 63, 64, 269, 270, 525, two_pass, two_pass + 1):
        add(_Case(f"lit_{L}").seq(8, 8, 8).seq(L, 5, 6).dense(4))
        if L:
            add(_Case(f"lit_first_{L}").seq(L, min(L, 3), 6).dense(4))
    for L in (128, 192, 200, 1000):                     # the line shift twice, the reload of all three lines; dense sequences at once
        add(_Case(f"run_{L}").seq(8, 8, 8).seq(L, 7, 5).dense(30).seq(L + 1, 9, 4).dense(30))
    # ---- match length ----
    for M in (4, 5, 18, 19, 20, 272, 273, 274, 528, 529, 19 + 255 * 64, 20 + 255 * 64, 70_000):
        add(_Case(f"match_{M}").seq(16, 16, M).dense(4).seq(2, 100 if M >= 100 else 11, M if M < 1000 else 4).dense(3))
    # ---- window packing ----
    c = _Case("pack_21x3").seq(64, 64, 4)               # (a generic sequence first: the next window starts at a token)
    for _ in range(4):
        _group(c, 21)
    add(c)
    for k in range(1, 22):
        c = _Case(f"pack_{k}").seq(64, 64, 4)
        for _ in range(3):
            _group(c, k)
        add(c)
    c = _Case("pack_16x273").seq(64, 64, 4)
    for rep in range(2):
        for j in range(16):
            c.seq(0, (1, 2, 3, 5, 17, 63, 64, 65)[j % 8] if rep else 68 - 4 * j, 273)
    add(c)
    c = _Case("edge_nx64").seq(64, 64, 4)               # 20 x 3 bytes + a 4-byte sequence: its next token is at window index 64
    for rep in range(2):
        for j in range(20):
            c.seq(0, 4 + j, 4 + j % 15)
        c.seq(1, 6, 9)
    add(c)
    c = _Case("edge_nx65").seq(64, 64, 4)               # ... + a 5-byte one: index 65, it opens the next window
    for rep in range(2):
        for j in range(20):
            c.seq(0, 4 + j, 4 + j % 15)
        c.seq(2, 6, 9)
    add(c)
    for k in range(64):                                 # the read position at every residue of a 64-byte line
        L = residue_prefix(k)
        c = _Case(f"residue_{k}").seq(L, 4, 274)        # the body's first token is stream byte k (mod 64), and a window starts there
        for j in range(36):
            c.seq((0, 1, 15, 3, 0, 16, 2)[j % 7], (1, 2, 7, 40, 64, 300)[j % 6] if c.n > 300 else 3, (4, 19, 30, 273, 5, 18, 274)[j % 7])
        add(c, 12 + k % 5)
    # ---- offsets against the copy width ----
    # (What the fast-path cases can and cannot tell apart: match byte i, at output position pos, is read from
    # pos - i - off + (i mod off); with i in place of `mod_small(i, off)` that is pos - off, which by the match's period holds the
    # same byte and which the pending loop resolves all the same, since it lies before the lane.  Far lanes never have i >= off: off > NEAR - 64 > 273 >= M.  So no stream separates the two forms; what
    # these cases hold is the order in which the pending loop lets the lanes of one round read one another.)
    for off in (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 63, 64, 65):
        c = _Case(f"off_{off}_fast").seq(80, 80, 4)
        for M in sorted({max(4, off - 1), max(4, off), off + 1 if off >= 3 else 4, 2 * off + 1 if off >= 2 else 6, 100, 273}):
            c.seq(3, off, M)
        add(c)
        add(_Case(f"off_{off}_generic").seq(80, 80, 4).seq(3, off, 274).seq(2, off, 529).seq(1, off, 5000).dense(3))
    c = _Case("off_sweep_273").seq(300, 300, 4)
    for off in range(1, 301):
        c.seq(1, off, 273)
    add(c)
    # ---- same-round dependence ----
    for off in (4, 1):
        c = _Case(f"chain_{off}_4").seq(8, 8, 4)
        for _ in range(96):
            c.seq(0, off, 4)
        add(c)
    # ---- the ring's edge and beyond ----
    for off in (4031, 4032, 4033, 4095, 4096, 4097, 8192, 65535):
        c = _Case(f"far_{off}_fast").seq(off + 100, off, 4)
        for _ in range(3):                              # windows of 64 stream bytes whose first round has a match byte in lane 0 and a
            c.seq(0, off, 7)                            # literal in lane 63: the ring slot lane 0's source had is that literal's by then
            for _ in range(9):
                c.seq(1, off, 6)
            for _ in range(5):
                c.seq(2, off, 5)
        for j in range(120):                            # every phase of literal and match lanes against the round
            c.seq(1 + j % 4, off, 4 + j % 5)
        c.seq(0, off, 273).seq(2, off, 19).dense(3)
        for j in range(40):
            c.seq(j % 3, off, 4 + j % 7)
        add(c)
        add(_Case(f"far_{off}_generic_M274").seq(off + 100, off, 4).seq(2, off, 274).dense(3).seq(61, off, 8).seq(0, off, 600).dense(3))
        for M in (off + 1, 2 * off + 17, 20_000):
            add(_Case(f"far_{off}_generic_M{M}").seq(off + 100, off, 4).seq(2, off, M).dense(3))
    c = _Case("far_long_stored").seq(5000, 5000, 4)     # (the generic far match waits for the literals' stores)
    for j in range(70):
        c.seq(2, 4100 + j, 6)                           # fast far matches whose sources that wait covered
    add(c)
    c = _Case("far_unacked_after_fast_rounds").seq(100, 50, 4)      # no far match yet, so nothing was waited for
    for rep in range(3):
        for j in range(16):
            c.seq(1, 30 + j, 273)                       # 4,384 bytes by fast rounds
        c.seq(2, 4200 + rep, 8).dense(14).seq(1, 4300, 6)       # sources those rounds stored; the second, rounds later, is covered by the first's wait
    add(c)
    c = _Case("far_residues").seq(5000, 5000, 4)        # 8-byte far matches: source and destination at every residue mod 4
    for generic in (0, 64):
        for d in range(4):
            for sres in range(4):
                L = (d - c.n) % 4 + generic
                pos = c.n + L
                c.seq(L, 4100 + (pos - sres - 4100) % 4, 8)
    add(c)
    c = _Case("ring_wrap_match").seq(4000, 4000, 4).seq(0, 100, 273).dense(3)
    c.seq(8192 - c.n - 103, 50, 4).seq(3, 50, 600).dense(3).seq(3, 5000, 273)
    add(c)
    # ---- stream ends ----
    for r in (0, 1, 2, 63):
        for t in range(12, 90):
            c = _Case(f"csize_mod64_{r}").seq(8, 8, 8).dense(20)
            name, seqs, tail = c.done(t)
            if len(build(seqs, tail)) % 64 == r:
                out.append((name, seqs, tail))
                break
        else:
            raise AssertionError(r)
    for t in (5, 12, 14, 15, 16, 59, 60, 61, 62, 63, 64, 300):
        add(_Case(f"tail_{t}").seq(8, 8, 8).dense(5).seq(1, 6, 9), t)
    add(_Case("last_match_5_before_end").seq(8, 8, 8).dense(5).seq(1, 6, 273), 5)
    for t in (5, 14, 15, 64, 300):
        add(_Case(f"litonly_{t}"), t)
    names = [o[0] for o in out]
    assert len(set(names)) == len(names)
    return out


STORED_SIZES = (1, 15, 16, 17, 1023, 1039, 70_001)


# ---------------------------------------------------------------------------------------------------------------------
# sequence-level fuzz
# ---------------------------------------------------------------------------------------------------------------------
_FUZZ_L = (0, 0, 0, 0, 1, 1, 2, 3, 5, 14, 15, 16, 59, 60, 61, 62, 63, 64, 269, 270, 525)
_FUZZ_M = (4, 4, 4, 5, 6, 8, 18, 19, 20, 64, 100, 272, 273, 274, 528, 529, 4096, 5000)
_FUZZ_OFF = (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 63, 64, 65, 300, 4031, 4032, 4033, 4095, 4096, 4097, 8192, 65535)
FUZZ_MAX_BYTES = 20 << 20


def fuzz(seed: int, n: int):
    """n random sequence lists (up to 60 sequences each) through no encoder -> [(name, seqs, tail)], conformant."""
    rng = np.random.default_rng(seed)
    out, total = [], 0
    for i in range(n):
        seqs, have = [], 0
        start = int(rng.choice((0, 0, 100, 4200, 4200, 9000, 70_000)))      # (history for the far offsets)
        if start:
            seqs.append((rng.bytes(start), int(rng.integers(1, min(start, 0xFFFF) + 1)), 4))
            have = start + 4
        dense = rng.random() < 0.5                      # half the streams: short sequences only, windows of many tokens
        for _ in range(int(rng.integers(1, 61)) - len(seqs)):
            if dense:
                L, M = int(rng.integers(0, 4)), int(rng.choice((4, 4, 5, 6, 8, 18, 19, 30, 273)))
            else:
                L = int(rng.choice(_FUZZ_L)) if rng.random() < 0.8 else int(rng.integers(0, 40))
                M = int(rng.choice(_FUZZ_M)) if rng.random() < 0.8 else int(rng.integers(4, 400))
                if rng.random() < 0.01:
                    M = 20_000
            if have + L == 0:
                L = 1
            off = int(rng.choice(_FUZZ_OFF)) if rng.random() < 0.7 else int(rng.integers(1, have + L + 1))
            off = min(off, have + L, 0xFFFF)            # clamped to the bytes produced so far
            seqs.append((rng.bytes(L) if L else b"", off, M))
            have += L + M
        tail = rng.bytes(int(rng.choice((8, 12, 14, 15, 16, 40, 64, 70))))
        assert conformant(seqs, tail)
        if total + have + len(tail) > FUZZ_MAX_BYTES:
            break
        total += have + len(tail)
        out.append((f"fuzz_{seed}_{i}", seqs, tail))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# damaged streams: one defect each.  Beside every one, the line of k_lz4_streams_vec that refuses it (the `bad = true` sites;
# "entry" = the csize / dsize check before the loop, "exit" = `bad || op != dsize` after it) and why nothing before that line
# leaves the stream's bytes or its destination.  Common to all: the compressed bytes are only read through ld_line (index
# clamped to csize - 1), the extension scans (clamped likewise) and, in the generic path, `from[i]`, i < Lg, after
# p + hdr + Lg <= csize, and src[p + (lane & 1)] after p + 2 <= csize; the fast path stores nothing before its checks
# (tot <= dsize - op; 1 <= off <= the bytes before the match), after which every stored position is op + r0 + lane < op + tot
# and every source is >= 0; the generic path stores literals after Lg <= dsize - op and matches after
# 1 <= offg <= op && Mg <= dsize - op.  ld_l2_u8 reads the aligned dword that holds a byte of the destination.
# ---------------------------------------------------------------------------------------------------------------------
def damaged():
    """-> [(name, stream, dsize)]"""
    rng = np.random.default_rng(77)
    r = rng.bytes
    head = (r(8), 8, 8)                                  # a first sequence that fits the window: the fast path takes it
    out = []

    def full(seqs, tail):
        return sum(len(l) + m for l, _, m in seqs) + len(tail)

    def case(name, seqs, tail, dsize=None, cut=None, append=b""):
        s = build(seqs, tail)
        s = (s if cut is None else s[:cut]) + append
        out.append((name, s, full(seqs, tail or b"") if dsize is None else dsize))

    # fast path, `off == 0` in the check after the scan (is_tok && (off == 0 || ...)): before any store
    case("off0_window", [head, (r(2), 0, 6), (r(2), 3, 4)], r(12))
    # generic path (70 literals do not fit a window), `offg == 0 || ...` after the literals were put inside dsize
    case("off0_generic", [head, (r(70), 0, 6)], r(12))
    # fast path, `off > op + drel + L` of the same check: 9 > 8 bytes produced
    case("before_start_first_window", [(r(8), 9, 8), (r(2), 3, 4)], r(12))
    # generic path, `offg > op`: 71 > 70
    case("before_start_first_generic", [(r(70), 71, 8)], r(12))
    # fast path, `off > op + drel + L`: 19 > 16 + 2
    case("before_start_mid_window", [head, (r(2), 19, 6), (r(2), 3, 4)], r(12))
    # generic path, `offg > op`: 87 > 16 + 70
    case("before_start_mid_generic", [head, (r(70), 87, 6)], r(12))
    # fast path, `tot > dsize - op`: 28 > 27, before any store
    case("match_past_dsize_window", [head, (r(2), 3, 10)], r(12), dsize=27)
    # generic path, `Mg > dsize - op`: 10 > 9, the 70 literals were inside
    case("match_past_dsize_generic", [head, (r(70), 3, 10)], r(12), dsize=16 + 70 + 9)
    # generic path (the final sequence), `Lg > dsize - op`: 12 > 11
    case("literals_past_dsize_final", [head], r(12), dsize=16 + 11)
    # generic path, `Lg > dsize - op`: 70 > 69
    case("literals_past_dsize_mid", [head, (r(70), 3, 4)], r(12), dsize=16 + 69)
    # generic path, `p + hdr + Lg > csize`: the token promises 10 literals, 5 follow
    case("literal_length_past_csize", [head], None, dsize=16 + 10, append=b"\xa0" + r(5))
    s2 = [head, (r(5), 3, 6), (r(3), 2, 4)]
    at = len(build([head], None))                        # the second sequence's token
    # generic path, `p + hdr + Lg > csize` (the token is the last byte)
    case("cut_after_token", s2, r(12), cut=at + 1)
    # the same line, three literals in
    case("cut_inside_literals", s2, r(12), cut=at + 1 + 3)
    # generic path, `p + 2 > csize` after the five literals were put (inside dsize)
    case("cut_after_one_offset_byte", s2, r(12), cut=at + 1 + 5 + 1)
    # generic path, the match-length scan: the lane past the end counts as "not 255", `p + k >= csize`
    case("cut_inside_match_extension", [head, (r(3), 2, 19 + 255 + 10)], r(12), cut=at + 1 + 3 + 2 + 1)
    # generic path, the literal-length scan: `q + k >= csize`
    case("cut_inside_literal_extension", [head, (r(15 + 255 + 3), 2, 4)], r(12), cut=at + 2)
    # the literal-length scan, `q + k >= csize`: 20 bytes of 0xFF to the end; and 70 of them: a second pass of the scan, then the same line
    case("ff_to_the_end", [head], None, dsize=6000, append=b"\xf0" + b"\xff" * 20)
    case("ff_to_the_end_two_passes", [head], None, dsize=20_000, append=b"\xf0" + b"\xff" * 70)
    # `p >= csize` at the loop's head after the match was copied (inside dsize: it decodes to exactly dsize)
    case("ends_on_a_match", [head, (r(2), 3, 6)], None)
    # exit: op != dsize
    case("dsize_one_more", [head, (r(2), 3, 6)], r(12), dsize=16 + 8 + 12 + 1)
    # generic path (the final sequence), `Lg > dsize - op`
    case("dsize_one_less", [head, (r(2), 3, 6)], r(12), dsize=16 + 8 + 12 - 1)
    # entry: `csize <= 0 || dsize <= 0`, before any load
    out.append(("csize_0", b"", 16))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Blosc-1 container and launch layout
# ---------------------------------------------------------------------------------------------------------------------
def blosc_wrap(streams, typesize: int, shuffle: bool, blocksize: int):
    """A Blosc-1 chunk (layout: the comment at the top of aggfly_amd/csrc/blosc1.c) of split blocks whose byte planes are the
    given LZ4 streams, ``typesize`` per block, each decoding to ``blocksize // typesize`` bytes.
    -> (chunk, [(offset of the stream in the chunk, csize, dsize)])."""
    assert len(streams) % typesize == 0 and blocksize % typesize == 0 and blocksize // typesize >= 128 and typesize <= 16
    nblocks = len(streams) // typesize
    body, bstarts, recs = bytearray(), [], []
    base = 16 + 4 * nblocks
    for b in range(nblocks):
        bstarts.append(base + len(body))
        for s in streams[b * typesize:(b + 1) * typesize]:
            assert len(s) != blocksize // typesize, "a stream as long as its plane reads as stored"
            body += struct.pack("<i", len(s))
            recs.append((base + len(body), len(s), blocksize // typesize))
            body += s
    flags = (1 if shuffle else 0) | (1 << 5)             # LZ4, blocks split (0x10 clear)
    head = struct.pack("<BBBBIII", 2, 1, flags, typesize, nblocks * blocksize, blocksize, base + len(body))
    return head + struct.pack(f"<{nblocks}i", *bstarts) + bytes(body), recs


def padded(seqs, tail, dsize: int, seed: int = 0):
    """The same sequences with the tail lengthened by random literals so that the stream decodes to ``dsize`` bytes."""
    have = sum(len(l) + m for l, _, m in seqs) + len(tail)
    assert have <= dsize
    return seqs, tail + np.random.default_rng(seed).bytes(dsize - have)


WRAP_PLANE = 16384
WRAP_SHAPES = ((2, True), (4, True), (8, True), (4, False), (2, False))            # (typesize, shuffled)


def wrapped_chunks():
    """Catalogue streams (those that decode to at most `WRAP_PLANE` bytes, their tails lengthened to exactly that) as the byte
    planes of two split blocks per chunk -> [(typesize, shuffled, chunk, records of `blosc_wrap`, what the chunk decodes to)]."""
    small = [(n, q, t) for n, q, t in catalogue() if sum(len(l) + m for l, _, m in q) + len(t) <= WRAP_PLANE and q]
    pick = [c for c in small if not c[0].startswith(("residue_", "lit_first_"))] + [c for c in small if c[0].startswith("residue_")]
    out, at = [], 0
    for ts, shuffle in WRAP_SHAPES:
        cases = [padded(q, t, WRAP_PLANE, seed=at + j) for j, (_, q, t) in enumerate(pick[at:at + 2 * ts])]
        assert len(cases) == 2 * ts
        at += 2 * ts
        planes = [expand(q, t) for q, t in cases]
        chunk, recs = blosc_wrap([build(q, t) for q, t in cases], ts, shuffle, WRAP_PLANE * ts)
        out.append((ts, shuffle, chunk, recs, weave(planes, ts) if shuffle else b"".join(planes)))
    return out


def weave(planes, typesize: int) -> bytes:
    """Blosc's byte shuffle undone: planes j of every block -> elements."""
    out = bytearray()
    for b in range(0, len(planes), typesize):
        out += np.stack([np.frombuffer(p, dtype=np.uint8) for p in planes[b:b + typesize]], axis=1).tobytes()
    return bytes(out)


def layout(items, stored=(), fill=0xAB):
    """Places records for one `hip.lz4_decode_streams` launch.  ``items`` = [(stream, dsize, expected bytes | None)]; None =
    a damaged stream, whose own destination is not compared.  ``stored`` = [(bytes, src aligned?, dst aligned?)].
    src_off / dst_off residues mod 16 rotate over 0 .. 15 (stored records: as asked), to_out alternates, 64 guard bytes lie
    before and after every destination.  -> (comp, records, {0: expected tmp, 1: expected out}, {0: mask, 1: mask}); the
    masks are False inside damaged destinations."""
    recs, comp = [], bytearray()
    at = {0: GUARD, 1: GUARD}
    want = []
    jobs = [(s, d, e, i % 16, (7 * i + 3) % 16) for i, (s, d, e) in enumerate(items)]
    jobs += [(b, len(b), b, 0 if sa else 5, 0 if da else 9) for b, sa, da in stored]
    for i, (s, d, e, sres, dres) in enumerate(jobs):
        comp += bytes(-len(comp) % 16 + sres)
        to_out = i & 1
        dst = (at[to_out] + 15) // 16 * 16 + dres
        recs.append((len(comp), dst, len(s), d, to_out, 0))
        comp += s
        want.append((to_out, dst, d, e))
        at[to_out] = dst + d + GUARD
    comp += bytes(64)
    dtype = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("csize", "<i4"), ("dsize", "<i4"), ("to_out", "<i4"), ("pad", "<i4")])
    image = {k: np.full(at[k] + 16, fill, dtype=np.uint8) for k in (0, 1)}
    mask = {k: np.ones(at[k] + 16, dtype=bool) for k in (0, 1)}
    for to_out, dst, d, e in want:
        if e is None:
            mask[to_out][dst:dst + d] = False
        else:
            assert len(e) == d
            image[to_out][dst:dst + d] = np.frombuffer(e, dtype=np.uint8)
    return np.frombuffer(bytes(comp), dtype=np.uint8).copy(), np.array(recs, dtype=dtype), image, mask
