"""Hand-built Zstandard frames for `afcodec_zstd_plan` (aggfly_amd/csrc/blosc1.c) and the seven passes of
aggfly_amd/csrc/zstd_passes.h (`k_zstd_tables` ... `k_zstd_gather`, afhip_zstd_kernels.h).

A compressor writes only what its heuristics choose; RFC 8878 allows far more, and the passes implement it.  Here a frame is
written from a DESCRIPTION (a list of blocks: their literals, how the literals are coded, their sequences as (literal length,
Offset_Value, match length), the mode of each of the three code tables, the header forms): `build` writes the bytes, `expand` is
what the description means (sequential, CONCRETE repeat offsets, RFC 8878 §3.1.1.3.2.1 and §3.1.1.5), `decode` is a strict RFC
decoder of the bytes (the judge of damaged frames; it also takes the census), `catalogue` names the shapes the passes branch
on, `fuzz` draws random block lists weighted towards them, `damaged` holds frames with one defect each beside the source text
that must refuse it, and `layout` places frames in the buffers of one batch with no padding at all.  Nothing here shares code
with the passes.  Used by tests/test_zstd_frames.py (host) and tests/test_gpu_zstd_frames.py (GPU).
"""
from __future__ import annotations

import bisect

import numpy as np

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 131072

# RFC 8878 §3.1.1.3.2.1.1: baselines and extra bits of the literal-length and match-length codes
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
# §3.1.1.3.2.2: the predefined distributions (accuracy logs 6 / 5 / 6)
LL_DEFAULT = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1]
OF_DEFAULT = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DEFAULT = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
DEFAULT = (LL_DEFAULT, OF_DEFAULT, ML_DEFAULT)
DEFAULT_LOG = (6, 5, 6)
MAX_SYM = (35, 31, 52)
MAX_LOG = (9, 8, 9)
TABLES = ("LL", "OF", "ML")
MODES = ("pre", "rle", "fse", "rep")
assert len(LL_BASE) == len(LL_BITS) == len(LL_DEFAULT) == 36 and len(ML_BASE) == len(ML_BITS) == len(ML_DEFAULT) == 53


class Invalid(Exception):
    """The bytes are no Zstandard frame that RFC 8878 allows (or one this project leaves to the host)."""


def ll_code(v):
    c = bisect.bisect_right(LL_BASE, v) - 1
    assert v - LL_BASE[c] < (1 << LL_BITS[c]), v
    return c, v - LL_BASE[c]


def ml_code(v):
    c = bisect.bisect_right(ML_BASE, v) - 1
    assert c >= 0 and v - ML_BASE[c] < (1 << ML_BITS[c]), v
    return c, v - ML_BASE[c]


def of_code(ofv):
    c = ofv.bit_length() - 1
    return c, ofv - (1 << c)


# ---------------------------------------------------------------------------------------------------------------------
# bit streams
# ---------------------------------------------------------------------------------------------------------------------
class BackBits:
    """Writer of a backward bitstream (§4.1): fields are `put` in the order the decoder reads them; the final 1-bit mark sits
    above the first field."""

    def __init__(self):
        self.parts = []

    def put(self, v, n):
        if n:
            assert 0 <= v < (1 << n), (v, n)
            self.parts.append(format(v, "0%db" % n))

    def nbits(self):
        return sum(len(p) for p in self.parts)

    def bytes(self):
        s = "1" + "".join(self.parts)
        return int(s, 2).to_bytes((len(s) + 7) // 8, "little")


class BackReader:
    """Reader of a backward bitstream; bits below the stream's start read as zero and leave `pos` negative."""

    def __init__(self, data):
        if not len(data) or data[-1] == 0:
            raise Invalid("bitstream without its end mark")
        self.d = bytes(data)
        self.pos = (len(data) - 1) * 8 + data[-1].bit_length() - 1

    def bits(self, lo, n):
        if n == 0:
            return 0
        if lo < 0:
            return self.bits(0, n + lo) << -lo if n + lo > 0 else 0
        return (int.from_bytes(self.d[lo >> 3:(lo + n + 7) >> 3], "little") >> (lo & 7)) & ((1 << n) - 1)

    def read(self, n):
        self.pos -= n
        return self.bits(self.pos, n)

    def peek(self, n):
        return self.bits(self.pos - n, n)


# ---------------------------------------------------------------------------------------------------------------------
# FSE (§4.1)
# ---------------------------------------------------------------------------------------------------------------------
def ncount_write(norm, log):
    """FSE table description of a normalised distribution (§4.1.1): forward bits, LSB first; short values take one bit less,
    a zero probability is followed by 2-bit repeat flags.  A distribution that does not sum to the table size is written as
    far as it goes (for `damaged`)."""
    bits, nbits = 0, 0

    def put(v, n):
        nonlocal bits, nbits
        assert 0 <= v < (1 << n)
        bits |= v << nbits
        nbits += n

    put(log - 5, 4)
    remaining, thr, nb, s, prev0 = (1 << log) + 1, 1 << log, log + 1, 0, False
    while remaining > 1 and s < len(norm):
        if prev0:
            run = 0
            while s + run < len(norm) and norm[s + run] == 0:
                run += 1
            s += run
            while run >= 3:
                put(3, 2)
                run -= 3
            put(run, 2)
            if s >= len(norm):
                break
        count = norm[s]
        s += 1
        mx = 2 * thr - 1 - remaining
        remaining -= abs(count)
        v = count + 1
        if v >= thr:
            v += mx
        put(v, nb - 1 if v < mx else nb)
        prev0 = count == 0
        while remaining < thr and thr > 1:
            nb -= 1
            thr >>= 1
    return bits.to_bytes((nbits + 7) // 8, "little")


def ncount_read(data, max_sym, max_log):
    """§4.1.1 read back -> (norm, log, bytes used)."""
    V, have, bit = int.from_bytes(data, "little"), len(data) * 8, 4
    if have < 8:
        raise Invalid("no table description")
    log = (V & 15) + 5
    if log > max_log:
        raise Invalid("accuracy log above the limit")
    remaining, thr, nb, norm, prev0 = (1 << log) + 1, 1 << log, log + 1, [], False
    while remaining > 1:
        if prev0:
            while True:
                r = (V >> bit) & 3
                bit += 2
                norm += [0] * r
                if r != 3:
                    break
        if len(norm) > max_sym or bit > have:
            raise Invalid("more symbols than the table may hold")
        mx = 2 * thr - 1 - remaining
        v = (V >> bit) & ((1 << nb) - 1)
        if (v & (thr - 1)) < mx:
            v &= thr - 1
            bit += nb - 1
        else:
            if v >= thr:
                v -= mx
            bit += nb
        count = v - 1
        remaining -= abs(count)
        if remaining < 1 or bit > have:
            raise Invalid("distribution does not sum to the table size")
        norm.append(count)
        prev0 = count == 0
        while remaining < thr and thr > 1:
            nb -= 1
            thr >>= 1
    return norm, log, (bit + 7) // 8


def fse_table(norm, log):
    """Decoding table of a distribution by the spec's spread -> [(symbol, nbits, baseline)] per state."""
    size = 1 << log
    if sum(abs(c) for c in norm) != size:
        raise Invalid("distribution does not sum to the table size")
    sym, high = [0] * size, size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nxt = [c if c > 0 else 1 for c in norm]
    table = []
    for u in range(size):
        s = sym[u]
        ns = nxt[s]
        nxt[s] += 1
        nb = log - (ns.bit_length() - 1)
        table.append((s, nb, (ns << nb) - size))
    return table


class FseEncoder:
    """The decoding table inverted: `back[(x, S')]` is the one state that carries x and whose update can reach S'."""
    _cache = {}

    def __init__(self, norm, log):
        self.log, self.table = log, fse_table(norm, log)
        self.states, self.back = {}, {}
        for s, (x, nb, base) in enumerate(self.table):
            self.states.setdefault(x, []).append(s)
            for v in range(base, base + (1 << nb)):
                assert (x, v) not in self.back
                self.back[(x, v)] = s
        assert len(self.back) == len(self.states) << log

    @classmethod
    def of(cls, norm, log):
        key = (tuple(norm), log)
        if key not in cls._cache:
            cls._cache[key] = cls(norm, log)
        return cls._cache[key]

    def chain(self, syms, rng, last_reads_bits=False):
        """States of a symbol list; the final state is free (a seeded draw among the states that carry the symbol)."""
        cand = self.states[syms[-1]]
        if last_reads_bits:
            cand = [s for s in cand if self.table[s][1] > 0]
        st = [0] * len(syms)
        st[-1] = cand[int(rng.integers(len(cand)))]
        for i in range(len(syms) - 2, -1, -1):
            st[i] = self.back[(syms[i], st[i + 1])]
        return st

    def update(self, s, s_next):
        """(value, nbits) the decoder reads when it leaves state s for s_next."""
        _, nb, base = self.table[s]
        return s_next - base, nb


def normalise(hist, log):
    """A distribution of 2^log over the symbols hist counts (each present symbol at least 1)."""
    size, total = 1 << log, sum(hist)
    norm = [max(1, h * size // total) if h else 0 for h in hist]
    while sum(norm) > size:
        top = max(range(len(norm)), key=lambda i: norm[i])
        assert norm[top] > 1, (hist, log)
        norm[top] -= 1
    norm[max(range(len(norm)), key=lambda i: norm[i])] += size - sum(norm)
    while norm and norm[-1] == 0:
        norm.pop()
    return norm


def auto_norm(codes, log, also=()):
    """A distribution over the codes a block uses (and `also`); never a single symbol."""
    hist = [0] * (max(max(codes), max(also, default=0), 1) + 1)
    for c in codes:
        hist[c] += 4
    for c in also:
        hist[c] += 1
    if sum(1 for h in hist if h) < 2:
        hist[0 if not hist[0] else 1] += 1
    return normalise(hist, log)


# ---------------------------------------------------------------------------------------------------------------------
# Huffman (§4.2)
# ---------------------------------------------------------------------------------------------------------------------
def huf_codes(weights):
    """weights[symbol] (0 = absent; the last is the one the description leaves out) -> (max bits, {symbol: (code, nbits)}),
    by the table layout: ascending weight, then ascending symbol, each taking 2^(weight-1) entries."""
    total = sum(1 << (w - 1) for w in weights if w)
    maxb = total.bit_length() - 1
    assert total == 1 << maxb and 1 <= maxb <= 11 and weights[-1] > 0, weights
    given = sum(1 << (w - 1) for w in weights[:-1] if w)
    assert given.bit_length() == maxb and (1 << maxb) - given == 1 << (weights[-1] - 1), "the last weight must be the implied one"
    codes, pos = {}, 0
    for wv in range(1, maxb + 1):
        for s, w in enumerate(weights):
            if w == wv:
                codes[s] = (pos >> (wv - 1), maxb + 1 - wv)
                pos += 1 << (wv - 1)
    return maxb, codes


def huf_stream(data, codes, pad=0):
    bb = BackBits()
    for x in data:
        bb.put(*codes[x])
    bb.put(0, pad)
    return bb.bytes()


def huf_description(weights, desc="direct", wlog=6, rng=None, wnorm=None):
    """Tree description of weights[:-1]: 4 bits a weight, or FSE-compressed with two interleaved states; the stream ends as
    the weight loop of the decoder expects — the update after the last but one weight runs out of bits."""
    w = list(weights[:-1])
    if desc == "direct":
        assert 1 <= len(w) <= 128
        body = bytes((w[i] << 4) | (w[i + 1] if i + 1 < len(w) else 0) for i in range(0, len(w), 2))
        return bytes([127 + len(w)]) + body
    assert len(w) >= 2
    hist = [0] * (max(w) + 1)
    for x in w:
        hist[x] += 1
    norm = wnorm or normalise(hist, wlog)
    enc = FseEncoder.of(norm, wlog)
    a, b = w[0::2], w[1::2]
    even = len(w) % 2 == 0                              # even: the first state's chain runs out; odd: the second's
    sa = enc.chain(a, rng, last_reads_bits=even)
    sb = enc.chain(b, rng, last_reads_bits=not even)
    bb = BackBits()
    bb.put(sa[0], wlog)
    bb.put(sb[0], wlog)
    for i in range(len(w) - 2):                         # the update after weight i; the last two weights have none written
        ch = sa if i % 2 == 0 else sb
        bb.put(*enc.update(ch[i // 2], ch[i // 2 + 1]))
    body = ncount_write(norm, wlog) + bb.bytes()
    assert len(body) < 128, len(body)
    return bytes([len(body)]) + body


def random_tree(rng, nsym, maxdepth=11, alphabet=None, skew=0.7):
    """Valid weights of nsym symbols: leaves split until there are enough; the last symbol is one of the deepest."""
    lens = [1, 1]
    while len(lens) < nsym:
        can = [i for i, d in enumerate(lens) if d < maxdepth]
        i = max(can, key=lambda j: lens[j]) if rng.random() < skew else can[int(rng.integers(len(can)))]
        lens[i] += 1
        lens.append(lens[i])
    maxb = max(lens)
    lens.sort()
    body = lens[:-1]
    rng.shuffle(body)
    ws = [maxb + 1 - d for d in body] + [1]
    if alphabet is None:
        return ws
    syms = sorted(int(x) for x in rng.choice(alphabet, size=nsym, replace=False))
    out = [0] * (syms[-1] + 1)
    for s, wv in zip(syms, ws):
        out[s] = wv
    return out


def draw(weights, n, rng):
    """n literals over the tree's symbols, likelier where the code is shorter; every symbol at least once when n allows."""
    if n == 0:
        return b""
    syms = [s for s, w in enumerate(weights) if w]
    p = np.array([float(1 << (weights[s] - 1)) for s in syms])
    x = rng.choice(syms, size=n, p=p / p.sum()).astype(np.uint8)
    k = min(n, len(syms))
    x[rng.choice(n, size=k, replace=False)] = np.array(syms[:k], dtype=np.uint8) if k else 0
    return x.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# descriptions
# ---------------------------------------------------------------------------------------------------------------------
PRE = ("pre", "pre", "pre")


def raw(data):
    return {"t": "raw", "data": bytes(data)}


def rle(byte, n):
    return {"t": "rle", "byte": byte, "n": n}


def comp(lit, seqs=(), modes=PRE, **kw):
    return dict(t="comp", lit=lit, seqs=[tuple(s) for s in seqs], modes=tuple(modes), **kw)


def l_raw(data, **kw):
    return dict(type="raw", data=bytes(data), **kw)


def l_rle(byte, n, **kw):
    return dict(type="rle", byte=byte, n=n, **kw)


def l_huf(data, weights, streams=1, **kw):
    return dict(type="huf", data=bytes(data), weights=list(weights), streams=streams, **kw)


def l_treeless(data, streams=1, **kw):
    return dict(type="treeless", data=bytes(data), streams=streams, **kw)


def frame(blocks, **header):
    return dict(blocks=list(blocks), **header)


def O(offset):
    """Offset_Value of a new offset."""
    return offset + 3


def lit_bytes(lit):
    return bytes([lit["byte"]]) * lit["n"] if lit["type"] == "rle" else lit["data"]


def block_size(b):
    if b["t"] == "raw":
        return len(b["data"])
    if b["t"] == "rle":
        return b["n"]
    return len(lit_bytes(b["lit"])) + sum(s[2] for s in b["seqs"])


def _copy(out, off, ml):
    if off >= ml:
        out += out[len(out) - off:len(out) - off + ml]
    else:
        pat = bytes(out[-off:])
        out += (pat * (ml // off + 1))[:ml]


def expand(fd):
    """The bytes a description means."""
    out, rep = bytearray(), [1, 4, 8]
    for b in fd["blocks"]:
        if b["t"] == "raw":
            out += b["data"]
        elif b["t"] == "rle":
            out += bytes([b["byte"]]) * b["n"]
        else:
            lit, p = lit_bytes(b["lit"]), 0
            for ll, ofv, ml in b["seqs"]:
                if p + ll > len(lit):
                    raise Invalid("more literal lengths than literals")
                out += lit[p:p + ll]
                p += ll
                if ofv > 3:
                    rep = [ofv - 3, rep[0], rep[1]]
                else:
                    i = ofv - 1 + (ll == 0)
                    if i == 1:
                        rep = [rep[1], rep[0], rep[2]]
                    elif i == 2:
                        rep = [rep[2], rep[0], rep[1]]
                    elif i == 3:
                        rep = [rep[0] - 1, rep[0], rep[1]]
                off = rep[0]
                if off <= 0 or off > len(out):
                    raise Invalid("offset outside the frame")
                _copy(out, off, ml)
            out += lit[p:]
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------------
def literals_header(lt, regen, comp_size=0, streams=1, fmt=None):
    """Literals_Section_Header in size format `fmt` (raw / RLE: 1, 2, 3 bytes; compressed: 0 = 3 bytes one stream, 1 / 2 / 3 =
    3 / 4 / 5 bytes four streams); the smallest that fits when None."""
    if lt < 2:
        fmt = fmt or (1 if regen < 32 else 2 if regen < 4096 else 3)
        assert regen < (32, 4096, 1 << 20)[fmt - 1]
        if fmt == 1:
            return bytes([lt | (regen << 3)])
        h = lt | ((1 if fmt == 2 else 3) << 2) | (regen << 4)
        return h.to_bytes(fmt, "little")
    if fmt is None:
        big = max(regen, comp_size)
        fmt = 0 if streams == 1 else (1 if big < 1024 else 2 if big < 16384 else 3)
    assert (fmt == 0) == (streams == 1)
    bits = (10, 10, 14, 18)[fmt]
    assert regen < (1 << bits) and comp_size < (1 << bits), (regen, comp_size, fmt)
    return (lt | (fmt << 2) | (regen << 4) | (comp_size << (4 + bits))).to_bytes((3, 3, 4, 5)[fmt], "little")


def _literals(lit, st):
    t = lit["type"]
    data = lit_bytes(lit)
    if t == "raw":
        return literals_header(0, len(data), fmt=lit.get("fmt")) + data
    if t == "rle":
        return literals_header(1, len(data), fmt=lit.get("fmt")) + data[:1]
    if t == "huf":
        st["huf"] = lit["weights"]
        desc = lit["desc_bytes"] if "desc_bytes" in lit else huf_description(
            lit["weights"], lit.get("desc", "direct"), lit.get("wlog", 6), st["rng"], lit.get("wnorm"))
    else:
        desc = b""
        if st["huf"] is None:
            st["huf"] = lit["weights"]                  # (damaged: treeless with nothing before it)
    _, codes = huf_codes(st["huf"])
    n, streams, pad = len(data), lit.get("streams", 1), lit.get("pad", 0)
    if streams == 1:
        body = huf_stream(data, codes, pad) + (b"\x00" if lit.get("zero_mark") else b"")
    else:
        seg = (n + 3) // 4
        parts = [huf_stream(data[i * seg:(i + 1) * seg], codes, pad if i == 1 else 0) for i in range(3)] + [huf_stream(data[3 * seg:], codes)]
        jump = lit.get("jump", [len(p) for p in parts[:3]])
        body = b"".join(int(j).to_bytes(2, "little") for j in jump) + b"".join(parts)
    return literals_header(2 if t == "huf" else 3, n, len(desc) + len(body), streams, lit.get("fmt")) + desc + body


def nseq_header(n, form=None):
    form = form or (1 if n < 128 else 2 if n < 0x7F00 else 3)
    if form == 1:
        assert 0 < n < 128
        return bytes([n])
    if form == 2:
        assert n < 0x7F00
        return bytes([128 + (n >> 8), n & 255])
    assert n >= 0x7F00
    return b"\xff" + (n - 0x7F00).to_bytes(2, "little")


def _sequences(b, st):
    seqs = b["seqs"]
    if not seqs:
        return b"\x00"
    codes = [[], [], []]
    extra = [[], [], []]
    for ll, ofv, ml in seqs:
        for t, (c, e) in enumerate((ll_code(ll), of_code(ofv), ml_code(ml))):
            codes[t].append(c)
            extra[t].append(e)
    head, modes_byte, enc = b"", b.get("modes_reserved", 0), [None] * 3
    for t, mode in enumerate(b["modes"]):
        modes_byte |= MODES.index(mode) << (6 - 2 * t)
        if mode == "pre":
            tab = ("fse", DEFAULT[t], DEFAULT_LOG[t])
        elif mode == "rle":
            assert len(set(codes[t])) == 1, "RLE mode needs one code"
            tab = ("rle", codes[t][0])
            head += bytes([codes[t][0]])
        elif mode == "fse":
            norm = b.get("norms", {}).get(t)
            log = b.get("logs", {}).get(t, DEFAULT_LOG[t])
            if norm is None:
                norm = auto_norm(codes[t], log, b.get("also", {}).get(t, ()))
            tab = ("fse", norm, log)
            head += ncount_write(norm, log)
        else:
            tab = st["tabs"][t] or ("fse", DEFAULT[t], DEFAULT_LOG[t])     # (damaged: Repeat_Mode with nothing before it)
        st["tabs"][t] = tab
        if tab[0] == "rle":
            assert set(codes[t]) == {tab[1]}, "the repeated RLE symbol is another"
        elif "raw_table" not in b:
            enc[t] = FseEncoder.of(tab[1], tab[2])
    chains = [e.chain(codes[t], st["rng"]) if e else None for t, e in enumerate(enc)]
    bb = BackBits()
    for t in range(3):
        if enc[t]:
            bb.put(chains[t][0], enc[t].log)
    for i in range(len(seqs)):
        bb.put(extra[1][i], codes[1][i])
        bb.put(extra[2][i], ML_BITS[codes[2][i]])
        bb.put(extra[0][i], LL_BITS[codes[0][i]])
        if i + 1 < len(seqs):
            for t in (0, 2, 1):
                if enc[t]:
                    bb.put(*enc[t].update(chains[t][i], chains[t][i + 1]))
    bb.put(0, b.get("seq_pad", 0))
    stream = bb.bytes() + (b"\x00" if b.get("zero_mark") else b"")
    return nseq_header(len(seqs), b.get("nseq_form")) + bytes([modes_byte]) + head + stream


def block_header(size, btype, last):
    return ((size << 3) | (btype << 1) | int(last)).to_bytes(3, "little")


def frame_header(n, single=True, did=0, fcs=None, reserved=0):
    """Magic, Frame_Header_Descriptor, Window_Descriptor unless single, a zero Dictionary_ID of `did` bytes, Frame_Content_Size in
    `fcs` bytes (1 only when single; 2 holds n - 256)."""
    if fcs is None:
        fcs = (1 if n < 256 and single else 2 if 256 <= n < 65792 else 4)
    assert (fcs != 1 or single) and (fcs != 2 or 256 <= n < 65792)
    fhd = ({1: 0, 2: 1, 4: 2, 8: 3}[fcs] << 6) | (int(single) << 5) | {0: 0, 1: 1, 2: 2, 4: 3}[did] | reserved
    out = MAGIC + bytes([fhd])
    if not single:
        out += bytes([max(0, (max(n, 1024) - 1).bit_length() - 10) << 3])
    return out + bytes(did) + (n - 256 if fcs == 2 else n).to_bytes(fcs, "little")


def build(fd, seed=0):
    """The frame's bytes."""
    st = {"huf": None, "tabs": [None] * 3, "rng": np.random.default_rng(fd.get("seed", seed))}
    n = fd.get("claim", sum(block_size(b) for b in fd["blocks"]))
    out = [frame_header(n, fd.get("single", True), fd.get("did", 0), fd.get("fcs"), fd.get("reserved", 0))]
    for i, b in enumerate(fd["blocks"]):
        last = i + 1 == len(fd["blocks"])
        if b["t"] == "raw":
            out += [block_header(len(b["data"]), 0, last), b["data"]]
        elif b["t"] == "rle":
            out += [block_header(b["n"], 1, last), bytes([b["byte"]])]
        else:
            body = _literals(b["lit"], st) + _sequences(b, st)
            assert len(body) <= BLOCK_MAX, len(body)
            out += [block_header(len(body), b.get("btype", 2), last), body]
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------------
# the strict decoder (and the census)
# ---------------------------------------------------------------------------------------------------------------------
def _huf_read(sec, census):
    """§4.2.1 -> (bytes used, table of 2^maxb (symbol, nbits), maxb)."""
    if not sec:
        raise Invalid("no tree description")
    h = sec[0]
    if h < 128:
        if h == 0 or 1 + h > len(sec):
            raise Invalid("tree description beyond the literals section")
        norm, log, used = ncount_read(sec[1:1 + h], 12, 6)
        if used >= h:
            raise Invalid("no weight stream")
        tab = fse_table(norm, log)
        br = BackReader(sec[1 + used:1 + h])
        s1 = br.read(log)
        s2 = br.read(log)
        w = []
        while True:
            if len(w) > 253:
                raise Invalid("more than 255 weights")
            w.append(tab[s1][0])
            s1 = tab[s1][2] + br.read(tab[s1][1])
            if br.pos < 0:
                w.append(tab[s2][0])
                census.add(("huf_end", 1))
                break
            w.append(tab[s2][0])
            s2 = tab[s2][2] + br.read(tab[s2][1])
            if br.pos < 0:
                w.append(tab[s1][0])
                census.add(("huf_end", 2))
                break
        used = 1 + h
        census.add(("huf_desc", "fse", log))
    else:
        n = h - 127
        used = 1 + (n + 1) // 2
        if used > len(sec):
            raise Invalid("weights beyond the literals section")
        w = [(sec[1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(n)]
        census.add(("huf_desc", "direct", "odd" if n & 1 else "even"))
    if any(x > 11 for x in w):
        raise Invalid("Huffman weight above 11")
    total = sum(1 << (x - 1) for x in w if x)
    if total == 0:
        raise Invalid("no weights")
    maxb = total.bit_length()
    rest = (1 << maxb) - total
    if maxb > 11 or rest & (rest - 1):
        raise Invalid("weights that complete no tree")
    w.append(rest.bit_length())
    census.add(("huf_symbols", sum(1 for x in w if x)))
    census.add(("huf_depth", maxb))
    table = []
    for wv in range(1, maxb + 1):
        for s, x in enumerate(w):
            if x == wv:
                table += [(s, maxb + 1 - wv)] * (1 << (wv - 1))
    assert len(table) == 1 << maxb
    return used, (table, maxb)


def _huf_decode(data, huf, n):
    table, maxb = huf
    br = BackReader(data)
    out = bytearray(n)
    for i in range(n):
        s, nb = table[br.peek(maxb)]
        out[i] = s
        br.pos -= nb
    if br.pos != 0:
        raise Invalid("Huffman stream does not end on its last symbol")
    return bytes(out)


class _State:
    def __init__(self):
        self.huf, self.tabs, self.rep = None, [None] * 3, [1, 4, 8]


def _block(q, out, S, bi, census, rec):
    if not q:
        raise Invalid("empty compressed block")
    lt, sf = q[0] & 3, (q[0] >> 2) & 3
    if lt < 2:
        hs = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        if hs > len(q):
            raise Invalid("truncated literals header")
        regen = q[0] >> 3 if hs == 1 else int.from_bytes(q[:hs], "little") >> 4
        size = regen if lt == 0 else 1
        if hs + size > len(q) or regen > BLOCK_MAX:
            raise Invalid("literals beyond the block")
        lit = q[hs:hs + regen] if lt == 0 else q[hs:hs + 1] * regen
        s, ns = hs + size, 1
    else:
        hs = 3 if sf < 2 else sf + 2
        if hs > len(q):
            raise Invalid("truncated literals header")
        bits = (10, 10, 14, 18)[sf]
        h = int.from_bytes(q[:hs], "little")
        regen, csz, ns = (h >> 4) & ((1 << bits) - 1), (h >> (4 + bits)) & ((1 << bits) - 1), 1 if sf == 0 else 4
        if hs + csz > len(q) or regen > BLOCK_MAX:
            raise Invalid("literals beyond the block")
        sec = q[hs:hs + csz]
        if lt == 2:
            used, S.huf = _huf_read(sec, census)
            sec = sec[used:]
        elif S.huf is None:
            raise Invalid("treeless literals with no tree before them")
        if ns == 1:
            lit = _huf_decode(sec, S.huf, regen)
        else:
            if len(sec) < 6:
                raise Invalid("no jump table")
            l = [int.from_bytes(sec[2 * i:2 * i + 2], "little") for i in range(3)]
            seg = (regen + 3) // 4
            if 6 + sum(l) >= len(sec) or 3 * seg > regen:
                raise Invalid("jump table longer than its section")
            at, lit = 6, b""
            for i, ln in enumerate(l + [len(sec) - 6 - sum(l)]):
                lit += _huf_decode(sec[at:at + ln], S.huf, seg if i < 3 else regen - 3 * seg)
                at += ln
        s = hs + csz
    name = ("raw", "rle", "huf", "treeless")[lt]
    census.add(("lit", name, ns))
    census.add(("lit_hdr", "plain" if lt < 2 else "coded", hs))
    if s >= len(q):
        raise Invalid("no sequences section")
    b0 = q[s]
    if b0 == 0:
        nseq, s = 0, s + 1
        if s != len(q):
            raise Invalid("bytes after an empty sequences section")
        census.add(("nseq_form", 0))
    else:
        form = 1 if b0 < 128 else 2 if b0 < 255 else 3
        if s + form >= len(q):
            raise Invalid("truncated sequences header")
        nseq = b0 if form == 1 else ((b0 - 128) << 8) + q[s + 1] if form == 2 else q[s + 1] + (q[s + 2] << 8) + 0x7F00
        s += form
        census.add(("nseq_form", form))
    rec.append(dict(btype=2, lit_type=lt, lit_size=regen, n_streams=ns, nseq=nseq))
    p = 0
    if nseq:
        modes = q[s]
        s += 1
        if modes & 3:
            raise Invalid("reserved bits of the compression modes set")
        tabs = []
        for t in range(3):
            m = (modes >> (6 - 2 * t)) & 3
            census.add(("mode", TABLES[t], MODES[m]))
            if m == 0:
                tab = ("fse", fse_table(DEFAULT[t], DEFAULT_LOG[t]), DEFAULT_LOG[t])
            elif m == 1:
                if s >= len(q) or q[s] > MAX_SYM[t]:
                    raise Invalid("RLE symbol")
                tab = ("rle", q[s])
                s += 1
            elif m == 2:
                norm, log, used = ncount_read(q[s:], MAX_SYM[t], MAX_LOG[t])
                census.add(("fse_log", TABLES[t], log))
                if -1 in norm:
                    census.add(("fse_less_than_one", TABLES[t]))
                tab = ("fse", fse_table(norm, log), log)
                s += used
            else:
                tab = S.tabs[t]
                if tab is None:
                    raise Invalid("Repeat_Mode with no table before it")
                census.add(("repeat_of", TABLES[t], tab[0] if tab[0] == "rle" else ("pre" if tab[3:] else "fse")))
            if m == 0:
                tab = tab + ("pre",)
            S.tabs[t] = tab
            tabs.append(tab)
        if s >= len(q):
            raise Invalid("no sequences bitstream")
        br = BackReader(q[s:])
        st = [br.read(tab[2]) if tab[0] == "fse" else 0 for tab in tabs]
        total = regen
        for i in range(nseq):
            c = [tab[1][st[t]][0] if tab[0] == "fse" else tab[1] for t, tab in enumerate(tabs)]
            census.add(("code", "LL", c[0]))
            census.add(("code", "OF", c[1]))
            census.add(("code", "ML", c[2]))
            ofv = (1 << c[1]) + br.read(c[1])
            ml = ML_BASE[c[2]] + br.read(ML_BITS[c[2]])
            ll = LL_BASE[c[0]] + br.read(LL_BITS[c[0]])
            if br.pos < 0:
                raise Invalid("sequences bitstream overrun")
            if p + ll > len(lit):
                raise Invalid("more literal lengths than literals")
            out += lit[p:p + ll]
            p += ll
            rep = S.rep
            if ofv > 3:
                S.rep = [ofv - 3, rep[0], rep[1]]
            else:
                census.add(("rep", ofv, "ll=0" if ll == 0 else "ll>0", "first" if bi == 0 else "later"))
                i3 = ofv - 1 + (ll == 0)
                if i3 == 1:
                    S.rep = [rep[1], rep[0], rep[2]]
                elif i3 == 2:
                    S.rep = [rep[2], rep[0], rep[1]]
                elif i3 == 3:
                    S.rep = [rep[0] - 1, rep[0], rep[1]]
            off = S.rep[0]
            if off <= 0 or off > len(out):
                raise Invalid("offset outside the frame")
            total += ml
            if total > BLOCK_MAX:
                raise Invalid("block regenerates more than 128 KiB")
            _copy(out, off, ml)
            if i + 1 < nseq:
                for t in (0, 2, 1):
                    if tabs[t][0] == "fse":
                        _, nb, base = tabs[t][1][st[t]]
                        st[t] = base + br.read(nb)
        if br.pos != 0:
            raise Invalid("sequences bitstream does not end on its last field")
    out += lit[p:]


def decode(fb, census=None, records=None):
    """Strict decoder of one frame -> its bytes; raises `Invalid`.  `census` (a set) receives what the frame exercises,
    `records` one dict per block (what `afcodec_zstd_plan` must have found)."""
    census = set() if census is None else census
    rec = [] if records is None else records
    fb = bytes(fb)
    if len(fb) < 6 or fb[:4] != MAGIC:
        raise Invalid("no Zstandard frame")
    fhd = fb[4]
    if fhd & 8:
        raise Invalid("reserved bit of the frame header set")
    if fhd & 4:
        raise Invalid("content checksum (left to the host)")
    single, p = (fhd >> 5) & 1, 5 + (0 if fhd & 32 else 1)
    dsz = (0, 1, 2, 4)[fhd & 3]
    fsz = (1 if single else 0, 2, 4, 8)[fhd >> 6]
    if p + dsz + fsz > len(fb):
        raise Invalid("truncated frame header")
    if int.from_bytes(fb[p:p + dsz], "little"):
        raise Invalid("dictionary (left to the host)")
    p += dsz
    fcs = int.from_bytes(fb[p:p + fsz], "little") + (256 if fsz == 2 else 0) if fsz else None
    p += fsz
    census.add(("frame", "single" if single else "window", dsz, fsz))
    out, S, bi = bytearray(), _State(), 0
    while True:
        if p + 3 > len(fb):
            raise Invalid("truncated block header")
        bh = int.from_bytes(fb[p:p + 3], "little")
        p += 3
        last, bt, bs = bh & 1, (bh >> 1) & 3, bh >> 3
        if bt == 3:
            raise Invalid("reserved block type")
        if bs > BLOCK_MAX or p + (1 if bt == 1 else bs) > len(fb):
            raise Invalid("block beyond the frame")
        census.add(("block", ("raw", "rle", "comp")[bt]))
        if bt == 0:
            out += fb[p:p + bs]
            p += bs
            rec.append(dict(btype=0, lit_type=0, lit_size=bs, n_streams=1, nseq=0))
        elif bt == 1:
            out += fb[p:p + 1] * bs
            p += 1
            rec.append(dict(btype=1, lit_type=1, lit_size=bs, n_streams=1, nseq=0))
        else:
            _block(fb[p:p + bs], out, S, bi, census, rec)
            p += bs
        bi += 1
        if last:
            break
    if p != len(fb):
        raise Invalid("bytes after the frame")
    if fcs is not None and len(out) != fcs:
        raise Invalid("decoded size differs from Frame_Content_Size")
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------
def R(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


T12 = [1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]                    # depth 11: code lengths 11, 11, 10, ... 1
T5 = [1, 1, 2, 3, 4]
T4 = [1, 1, 2, 3]
T256 = [3] * 64 + [2] * 64 + [1] * 128                          # 256 symbols, depth 9


def pack_codes(values, which, rng, modes=PRE, later=None, room=100000, **kw):
    """Blocks (after 8 raw bytes) whose sequences carry the given literal lengths (which = 0) or match lengths (2), as many to a
    block as fit; the literals are raw, the offsets new and small; `later`: the modes of every block after the first."""
    blocks, cur = [raw(R(8, 1))], []

    def flush():
        if cur:
            blocks.append(comp(l_raw(R(sum(s[0] for s in cur), len(blocks) + 7)), list(cur), modes if len(blocks) == 1 or later is None else later, **kw))
        cur.clear()

    for v in values:
        ll, ml = (v, 3) if which == 0 else (1, v)
        if sum(s[0] + s[2] for s in cur) + ll + ml > room:
            flush()
        cur.append((ll, O(1 + int(rng.integers(3))), ml))
    flush()
    return blocks


def draw_seqs(rng, n, produced, reps, fixed=(None, None, None), lls=(0, 0, 1, 2, 5, 17, 40, 63), mls=(3, 3, 4, 5, 9, 30, 100, 130), cap=60000,
              far=1 << 17):
    """Up to n valid sequences after `produced` bytes of the frame, half of them repeat codes; reps (the concrete history, for
    validity only) is updated in place; fixed[t]: the one code table t allows."""
    seqs, made = [], 0
    for _ in range(n):
        ll = LL_BASE[fixed[0]] if fixed[0] is not None else int(rng.choice(lls))
        ml = ML_BASE[fixed[2]] if fixed[2] is not None else int(rng.choice(mls))
        have = produced + made + ll
        if fixed[1] is not None:
            lo, hi = (1 << fixed[1]) - 3, (2 << fixed[1]) - 4
            if have < lo and fixed[0] is None:
                ll = min(63, lo - produced - made)
                have = produced + made + ll
            if have < lo:
                break
            ofv = O(int(rng.integers(lo, min(hi, have) + 1)))
        else:
            if have == 0:
                ll = 1 + int(rng.integers(8))
                have = ll
            ofv = int(rng.integers(1, 4)) if rng.random() < 0.5 else O(int(rng.integers(1, min(have, far) + 1)))
            if ofv <= 3:
                i3 = ofv - 1 + (ll == 0)
                off = reps[i3] if i3 < 3 else reps[0] - 1
                if off <= 0 or off > have:
                    ofv = O(int(rng.integers(1, min(have, 60) + 1)))
        if ofv > 3:
            reps[:] = [ofv - 3, reps[0], reps[1]]
        else:
            i3 = ofv - 1 + (ll == 0)
            if i3 == 1:
                reps[:] = [reps[1], reps[0], reps[2]]
            elif i3 == 2:
                reps[:] = [reps[2], reps[0], reps[1]]
            elif i3 == 3:
                reps[:] = [reps[0] - 1, reps[0], reps[1]]
        seqs.append((ll, ofv, ml))
        made += ll + ml
        if made > cap:
            break
    return seqs


def mixed_blocks(n, rng, sizes=(1, 40)):
    """n small blocks of every kind in turn: raw, RLE and sequence-free blocks between blocks that use repeat offsets, Repeat_Mode
    and treeless literals."""
    blocks, tree, defined, produced, reps = [], None, False, 0, [1, 4, 8]
    for i in range(n):
        k = i % 6
        m = int(rng.integers(sizes[0], sizes[1]))
        if k == 0:
            blocks.append(raw(R(m, 1000 + i)))
        elif k == 2:
            blocks.append(rle(int(rng.integers(256)), m))
        elif k == 4:
            blocks.append(comp(l_raw(R(m, 2000 + i))))
        else:
            seqs = draw_seqs(rng, 5, produced, reps, lls=(0, 1, 2, 3), mls=(3, 4, 5, 6), far=60)
            nl = sum(s[0] for s in seqs) + m % 3
            streams = 4 if i % 4 == 1 and nl >= 6 else 1
            if tree is None or i % 30 == 1:
                tree = random_tree(rng, int(rng.integers(3, 20)), maxdepth=8)
                lit = l_huf(draw(tree, nl, rng), tree, streams=streams)
            else:
                lit = l_treeless(draw(tree, nl, rng), streams=streams)
            blocks.append(comp(lit, seqs, ("rep",) * 3 if defined else ("fse", "fse", "fse"), also={0: range(4), 1: range(8), 2: range(4)}))
            defined = True
        produced += block_size(blocks[-1])
    return blocks


def catalogue():
    """[(name, the branch it is for, description)]"""
    out = []
    rng = np.random.default_rng(8878)

    def add(name, why, blocks, **hdr):
        assert name not in {n for n, _, _ in out}, name
        out.append((name, why, frame(blocks, seed=len(out), **hdr)))

    # ---- frame headers
    for n, fcs in ((255, 1), (256, 2), (65791, 2), (65792, 4), (300, 4), (300, 8)):
        add(f"fcs-{n}-in-{fcs}", "zstd_plan_frames: fcs_size / fcs += 256", [raw(R(n, n))], fcs=fcs)
    add("frame-empty", "one raw block of size 0", [raw(b"")])
    for did in (1, 2, 4):
        add(f"frame-zero-dictionary-id-{did}", "did_size, did == 0", [raw(R(40, did))], did=did)
    for fcs in (2, 4, 8):
        add(f"frame-window-descriptor-fcs-{fcs}", "single == 0", [raw(R(700, fcs))], single=False, fcs=fcs)
    # ---- blocks
    add("block-raw", "btype 0", [raw(R(1000, 1))])
    add("block-rle", "btype 1", [rle(0x5A, 1000)])
    add("block-raw-rle-131072", "Block_Size at its bound", [raw(R(BLOCK_MAX, 2)), rle(7, BLOCK_MAX)])
    add("block-nseq-0", "b0 == 0", [comp(l_raw(R(100, 3)))])
    add("block-comp-131072-rle-literals", "lit_size == AFZ_BLOCK_MAX", [comp(l_rle(9, BLOCK_MAX))])
    add("block-comp-131072-with-matches", "lit_size + sum_ml == AFZ_BLOCK_MAX", [comp(l_raw(R(72, 4)), [(50, O(7), 100000), (22, O(30), 31000)])])
    add("blocks-300-small", "afz_pass_frame over 300 blocks; raw, RLE, sequence-free blocks between the others", mixed_blocks(300, rng))
    # ---- literals, raw and RLE
    for n in (1, 31, 32, 4095, 4096):
        add(f"literals-raw-{n}", "zstd_literals_header: hs of raw literals", [comp(l_raw(R(n, n)))])
        add(f"literals-rle-{n}", "zstd_literals_header: hs of RLE literals; lit_type == 1 in afz_pass_literals", [comp(l_rle(n & 255, n))])
    add("literals-raw-131067", "the most raw literals a block holds", [comp(l_raw(R(131067, 5)))])
    add("literals-rle-131072", "20-bit size", [raw(R(9, 1)), comp(l_rle(3, BLOCK_MAX))])
    for fmt in (2, 3):
        add(f"literals-raw-wide-header-{fmt}", "a larger size format than needed", [comp(l_raw(R(20, fmt), fmt=fmt), [(5, O(2), 4)])])
        add(f"literals-rle-wide-header-{fmt}", "a larger size format than needed", [comp(l_rle(fmt, 20, fmt=fmt), [(5, O(2), 4)])])
    # ---- literals, compressed
    t20 = random_tree(rng, 20, maxdepth=9)
    add("literals-huf-1-stream", "n_streams == 1", [comp(l_huf(draw(t20, 700, rng), t20))])
    for n, fmt in ((900, 1), (900, 2), (900, 3), (5000, 2), (20000, 3), (BLOCK_MAX, 3)):
        add(f"literals-huf-4-streams-{n}-format-{fmt}", "10-, 14- and 18-bit sizes", [comp(l_huf(draw(T5, n, rng), T5, streams=4, fmt=fmt))])
    for n in (6, 7, 8, 9, 20, 21, 22, 23):
        add(f"literals-huf-4-streams-{n}", "seg = (n + 3) / 4, seg * 3 > n", [comp(l_huf(draw(T4, n, rng), T4, streams=4))])
    # ---- Huffman trees
    add("tree-direct-1-weight", "nw == 1: two symbols", [comp(l_huf(draw([1, 1], 50, rng), [1, 1]))])
    add("tree-two-symbols-apart", "a two-symbol tree, zero weights between", [comp(l_huf(draw([0] * 5 + [1, 0, 0, 0, 1], 50, rng), [0] * 5 + [1, 0, 0, 0, 1]))])
    add("tree-direct-odd-count", "nw = 3", [comp(l_huf(draw(T4, 60, rng), T4))])
    add("tree-direct-even-count", "nw = 4", [comp(l_huf(draw(T5, 60, rng), T5))])
    add("tree-direct-128-weights", "h == 255", [comp(l_huf(draw([1] * 128 + [8], 600, rng), [1] * 128 + [8]))])
    add("tree-depth-11", "maxb == 11", [comp(l_huf(draw(T12, 4000, rng), T12, streams=4))])
    add("tree-256-symbols", "nw == 255, FSE-compressed", [comp(l_huf(draw(T256, 3000, rng), T256, streams=4, desc="fse", wlog=6))])
    for wlog in (5, 6):
        for parity in (0, 1):
            t = random_tree(rng, 30, maxdepth=10, alphabet=200)
            while (len(t) - 1) % 2 != parity:
                t = random_tree(rng, 30, maxdepth=10, alphabet=200)
            add(f"tree-fse-log-{wlog}-{'odd' if parity else 'even'}-count", "FSE-compressed weights; the loop of afz_huffman_table ends on state %d" % (2 if parity else 1),
                [comp(l_huf(draw(t, 500, rng), t, desc="fse", wlog=wlog))])
    # ---- treeless
    seq3 = [(4, O(3), 5)]
    add("treeless-after-1-block", "huf_block = the block before", [comp(l_huf(draw(t20, 90, rng), t20), seq3), comp(l_treeless(draw(t20, 80, rng)), seq3)])
    add("treeless-after-several", "huf_block further back", [comp(l_huf(draw(t20, 90, rng), t20))] + [comp(l_treeless(draw(t20, 70 + i, rng), streams=1 + 3 * (i & 1))) for i in range(5)])
    add("treeless-across-raw-literals", "raw-literal, raw and RLE blocks do not reset the tree",
        [comp(l_huf(draw(t20, 90, rng), t20)), comp(l_raw(R(30, 1))), raw(R(10, 2)), rle(1, 10), comp(l_rle(4, 12)), comp(l_treeless(draw(t20, 75, rng), streams=4))])
    add("treeless-across-workgroups", "k_zstd_literals: the table in block 15, its user in block 16",
        [raw(R(5 + i, i)) for i in range(15)] + [comp(l_huf(draw(t20, 200, rng), t20, streams=4))] + [comp(l_treeless(draw(t20, 150 + i, rng), streams=4 if i & 1 else 1)) for i in range(4)])
    trees = [random_tree(rng, 3 + 2 * i, maxdepth=6 + i % 6) for i in range(16)]
    add("workgroup-of-16-tables", "k_zstd_literals: 16 tables staged in LDS, 64 streams",
        [comp(l_huf(draw(t, 300 + i, rng), t, streams=4)) for i, t in enumerate(trees)] + [comp(l_treeless(draw(trees[-1], 100, rng), streams=4))])
    # ---- sequence counts
    for n in (1, 127, 128, 0x7EFF, 0x7F00, BLOCK_MAX // 3):
        seqs = [(2, O(2), 3)] + [(0, O(1 + i % 2), 3) for i in range(n - 1)]
        add(f"nseq-{n}", "Number_of_Sequences header forms; AFZ_BLOCK_MAX / 3", [comp(l_raw(b"ab"), seqs, ("pre", "fse", "pre") if n % 2 else PRE)])
    add("nseq-100-in-2-bytes", "the 2-byte form below 128", [comp(l_raw(b"abc"), [(3, O(2), 3)] + [(0, O(3), 3)] * 99, nseq_form=2)])
    # ---- sequence modes: every triple, as the second block of a frame whose first block defines all three tables
    const = lambda k: [(2, 4 + (k + j) % 4, 5) for j in range(3)]   # LL code 2, OF code 2, ML code 2 throughout
    for a in range(4):
        for b in range(4):
            for c in range(4):
                tri = (MODES[a], MODES[b], MODES[c])
                first = tuple(MODES[(a + b + c + t) % 3] if m == "rep" else "fse" for t, m in enumerate(tri))
                add("modes-" + "-".join(tri), "k->mode[t] / tab_block[t] of a block after one that defines " + "-".join(first),
                    [comp(l_raw(R(8, a)), const(0), first), comp(l_raw(R(8, b)), const(1), tri)])
    add("repeat-after-rle", "tmode carried: RLE symbol again", [comp(l_raw(R(8, 1)), const(0), ("rle",) * 3), comp(l_raw(R(8, 2)), const(2), ("rep",) * 3)])
    add("repeat-after-predefined", "tmode carried: predefined again", [comp(l_raw(R(8, 1)), const(0), PRE), comp(l_raw(R(8, 2)), const(2), ("rep",) * 3)])
    add("repeat-across-other-blocks", "sequence-free, raw and RLE blocks leave the tables",
        [comp(l_raw(R(8, 1)), const(0), ("fse",) * 3), comp(l_raw(R(5, 3))), raw(R(6, 4)), rle(2, 7), comp(l_raw(R(8, 2)), const(1), ("rep",) * 3)])
    add("repeat-chain-of-5", "tab_block five blocks back", [comp(l_raw(R(8, 1)), const(0), ("fse",) * 3)] + [comp(l_raw(R(8, 2 + i)), const(i), ("rep",) * 3) for i in range(5)])
    # ---- FSE tables
    some = [(3, O(2), 3), (3, O(5), 9), (0, O(1), 14), (7, O(9), 22), (2, O(3), 5)]
    add("fse-logs-5", "accuracy log 5 in all three", [comp(l_raw(R(20, 1)), some, ("fse",) * 3, logs={0: 5, 1: 5, 2: 5})])
    add("fse-logs-9-8-9", "accuracy logs at their limits", [comp(l_raw(R(20, 2)), some, ("fse",) * 3, logs={0: 9, 1: 8, 2: 9}, also={0: range(36), 1: range(12), 2: range(53)})])
    add("fse-less-than-one", "norm[s] == -1 in afz_build_fse",
        [comp(l_raw(R(20, 3)), some, ("fse",) * 3, norms={0: [20, -1, 10, 10, -1, 5, 5, 12], 1: [8, 8, -1, 14, -1], 2: [22, -1, 10, -1, -1, -1, 10, -1, -1, -1, -1, 5, -1, -1, -1, -1, -1, -1, -1, 2]},
              logs={0: 6, 1: 5, 2: 6})])
    add("fse-zero-runs-1-3-4-7", "the chained 2-bit repeat flags of afz_read_ncount",
        [comp(l_raw(R(20, 4)), some, ("pre", "pre", "fse"), norms={2: [16, 0, 16, 0, 0, 0, 16, 0, 0, 0, 0, 8, 0, 0, 0, 0, 0, 0, 0, 8]})])
    every = {0: [1] * 35 + [29], 1: [1] * 20 + [12], 2: [1] * 52 + [12]}
    lls = [LL_BASE[c] + x for c in range(36) for x in sorted({0, (1 << LL_BITS[c]) - 1}) if LL_BASE[c] + x <= 131069]
    mls = [ML_BASE[c] + x for c in range(53) for x in sorted({0, (1 << ML_BITS[c]) - 1}) if ML_BASE[c] + x <= 131071]
    for which, vals, nm in ((0, lls, "LL"), (2, mls, "ML")):
        add(f"codes-{nm}-all-predefined", "every code that fits a block, extra bits all zero and all one; the predefined tables' last symbols",
            pack_codes(vals, which, rng))
        add(f"codes-{nm}-all-fse-every-symbol", "a table that lists every symbol, repeated across the blocks that use them",
            pack_codes(vals, which, rng, ("fse",) * 3, ("rep",) * 3, norms=every))
    # every offset code a frame of 1 MiB can hold: 2^c - 3 and 2^(c+1) - 4
    early = [raw(R(BLOCK_MAX, 11)), rle(1, BLOCK_MAX), raw(R(BLOCK_MAX, 12)), rle(2, BLOCK_MAX), rle(3, BLOCK_MAX), raw(R(BLOCK_MAX, 13)), rle(4, BLOCK_MAX)]
    ofs = [v for c in range(2, 20) for v in ((1 << c), (2 << c) - 1)]
    n2 = (1 << 20) - 4 - 7 * BLOCK_MAX - 4 * (len(ofs) - 1)          # RLE literals up to the last match: offset 2^20 - 4, code 19, all ones
    add("codes-OF-2-to-19", "every offset code with both extremes of its extra bits; sources in raw and RLE blocks",
        early + [comp(l_raw(R(len(ofs) - 1, 14)), [(1, v, 3) for v in ofs[:-1]], ("pre", "fse", "pre"), logs={1: 8}),
                 comp(l_rle(0x77, n2), [(n2, ofs[-1], 3)], ("pre", "rle", "pre"))])
    add("codes-OF-20-in-1MiB", "the largest offset code a frame of 1 MiB can hold; an offset that reaches the frame's first byte",
        early + [comp(l_rle(0x78, BLOCK_MAX - 3), [(BLOCK_MAX - 3, 1 << 20, 3)], ("pre", "rle", "pre"))])
    # ---- bit window
    add("bits-49-extra-in-one-sequence", "afz_peek refills inside a sequence",
        [rle(1, BLOCK_MAX), raw(R(BLOCK_MAX, 15)), comp(l_rle(8, 32768 + 0x1555), [(32768 + 0x1555, (1 << 18) + 0x5555, 65539 + 0x5555)], ("fse", "fse", "fse"))])
    for c in range(2, 10):
        add(f"bits-end-mark-{(17 + c) % 8}", "afz_bits_init: the end mark in each bit position", [raw(R(1100, c)), comp(l_raw(b"xy"), [(1, (1 << c) + 1, 3)])])
    # ---- repeat offsets
    for ofv in (1, 2, 3):
        add(f"rep-{ofv}-first-of-frame", "initial 1, 4, 8 through rep_in of block 0", [comp(l_raw(R(12, ofv)), [(9, ofv, 6)])])
        add(f"rep-{ofv}-ll0-second-of-frame", "ll == 0 shifts the repeat codes, in the frame's first block", [comp(l_raw(R(12, ofv)), [(9, O(5), 4), (0, ofv, 6)])])
        for ll in (3, 0):
            if (ofv, ll) != (3, 0):
                add(f"rep-{ofv}-ll{ll}-first-sequences-after-raw", "initial 1, 4, 8 carried through a raw block", [raw(R(12, ofv)), comp(l_raw(R(5, ll)), [(ll, ofv, 6)])])
            for at in range(3):
                pre = [(1, 2, 3), (0, 1, 4)][:at]
                add(f"rep-{ofv}-ll{ll}-sequence-{at + 1}-of-later-block", "AFZ_SYM entries, swapped %d times before use, resolved in afz_pass_fill" % at,
                    [comp(l_raw(R(30, at)), [(10, O(7), 4), (5, O(12), 4), (5, O(20), 5)]), comp(l_raw(R(9, ofv)), pre + [(ll, ofv, 6), (1, O(3), 3), (1, 3, 4)])])
    add("rep0-minus-1-three-times", "off = r0 - 3 on a symbolic entry, three times", [comp(l_raw(R(30, 1)), [(20, O(9), 4), (5, O(12), 4)]), comp(l_raw(R(4, 2)), [(0, 3, 5), (0, 3, 4), (0, 3, 6), (2, 1, 3), (1, 2, 3), (1, 3, 3)])])
    add("rep-history-across-10-blocks", "afz_pass_frame composes identity entries",
        [comp(l_raw(R(40, 1)), [(20, O(9), 4), (5, O(14), 4), (5, O(21), 4)])] + [b for i in range(3) for b in (raw(R(3, i)), rle(i, 4), comp(l_raw(R(5, i))))] +
        [comp(l_raw(R(2, 5)))] + [comp(l_raw(R(6, 9)), [(0, 3, 5), (2, 3, 4), (1, 2, 3)])])
    # ---- matches
    add("match-offset-1-whole-block", "one 131071-byte chain in afz_pass_fill / afz_jump", [comp(l_raw(b"q"), [(1, O(1), BLOCK_MAX - 1)])])
    add("jump-bound-2^18", "afz_rounds_host is tight on an offset-1 chain as long as the frame", [comp(l_raw(b"q"), [(1, O(1), BLOCK_MAX - 1)]), comp(l_raw(b""), [(0, O(1), BLOCK_MAX)])])
    add("jump-bound-2^18+1", "afz_rounds_host one byte past a power of two",
        [comp(l_raw(b"q"), [(1, O(1), BLOCK_MAX - 1)]), comp(l_raw(b""), [(0, O(1), BLOCK_MAX - 3)]), comp(l_raw(b""), [(0, O(1), 4)])])
    add("match-reaches-first-byte", "off == pos + ll - fr->base", [raw(R(33, 1)), comp(l_raw(R(7, 2)), [(7, O(40), 50)])])
    add("match-sources-in-raw-and-rle-blocks", "sources in earlier blocks", [raw(R(50, 1)), rle(0xEE, 60), comp(l_raw(R(4, 3)), [(2, O(100), 20), (2, O(40), 30)])])
    add("match-overlap-crosses-block-end", "offset < length, the source runs from the block before into the match itself", [raw(R(10, 4)), comp(l_raw(b""), [(0, O(4), 29)])])
    # ---- literal totals
    add("literals-all-in-sequences", "sum_ll == lit_size: rest == 0", [comp(l_raw(R(10, 1)), [(4, O(2), 3), (6, O(5), 4)])])
    add("literals-trailing-only", "every ll == 0", [raw(R(9, 1)), comp(l_raw(R(10, 2)), [(0, O(2), 3), (0, 1, 4)])])
    return out


# what the census of tests/test_zstd_frames.py must find: in the catalogue all of it, in the fuzz all but NOT_BY_FUZZ
CLASSES = ([("lit", t, n) for t, n in (("raw", 1), ("rle", 1), ("huf", 1), ("huf", 4), ("treeless", 1), ("treeless", 4))] +
           [("mode", t, m) for t in TABLES for m in MODES] +
           [("rep", ofv, ll, where) for ofv in (1, 2, 3) for ll in ("ll>0", "ll=0") for where in ("first", "later")] +
           [("huf_end", 1), ("huf_end", 2)] + [("nseq_form", k) for k in (0, 1, 2, 3)] +
           [("lit_hdr", "plain", k) for k in (1, 2, 3)] + [("lit_hdr", "coded", k) for k in (3, 4, 5)])
NOT_BY_FUZZ = {("nseq_form", 3), ("lit_hdr", "coded", 5)}          # 32512 sequences or 16 KiB of coded literals in one block
LAUNCH_GEOMETRY = ("blocks-300-small", "workgroup-of-16-tables", "treeless-across-workgroups")
JUMP_BOUND = ("jump-bound-2^18", "jump-bound-2^18+1")


# ---------------------------------------------------------------------------------------------------------------------
# fuzz
# ---------------------------------------------------------------------------------------------------------------------
WIDE = {0: range(25), 1: range(18), 2: range(43)}       # the support of every FSE table the fuzz defines


def _fuzz_block(rng, produced, reps, prev, tree):
    """One compressed block -> (block, bytes it adds, tree in force); reps / prev are updated in place."""
    kind = int(rng.integers(4)) if tree else int(rng.integers(3))
    nlit = int(rng.choice([0, 1, 5, 40, 300, 2000]))
    nseq = int(rng.choice([0, 1, 2, 3, 8, 40, 200]))
    modes = [MODES[int(rng.integers(4))] for _ in range(3)]
    for t in range(3):
        if modes[t] == "rep" and prev[t] is None:
            modes[t] = "fse"
    fixed = [None] * 3                                  # the one code an RLE table (new or repeated) allows
    for t in range(3):
        if modes[t] == "rle":
            fixed[t] = int(rng.integers(4, 21)) if t == 0 else int(rng.integers(2, 5)) if t == 1 else int(rng.integers(0, 40))
        elif modes[t] == "rep" and prev[t][0] == "rle":
            fixed[t] = prev[t][1]
    seqs = draw_seqs(rng, nseq, produced, reps, fixed)
    lits = sum(q[0] for q in seqs)
    trailing = int(rng.choice([0, 0, 3, nlit]))
    n = lits + trailing
    if not seqs:
        modes = list(PRE)
        n = max(n, 1)                                   # (libzstd takes no compressed block below 3 bytes)
    for t in range(3):
        if seqs:
            prev[t] = ("rle", fixed[t]) if modes[t] == "rle" else prev[t] if modes[t] == "rep" else (modes[t],)
    if kind == 0 or n == 0:
        lit = l_raw(R(n, int(rng.integers(1 << 30))))
    elif kind == 1:
        lit = l_rle(int(rng.integers(256)), n)
    else:
        streams = 4 if n >= 1000 or (n >= 6 and rng.random() < 0.5) else 1
        if kind == 2:
            tree = random_tree(rng, int(rng.integers(2, 60)), maxdepth=int(rng.integers(6, 12)), alphabet=int(rng.choice([64, 256])))
            nw, mixed = len(tree) - 1, len(set(tree[:-1])) > 1
            if nw > 128 and not mixed:
                tree, nw = list(T5), 4
            fse = nw > 128 or (nw >= 2 and mixed and rng.random() < 0.5)
            lit = l_huf(draw(tree, n, rng), tree, streams, desc="fse" if fse else "direct", wlog=int(rng.integers(5, 7)))
        else:
            lit = l_treeless(draw(tree, n, rng), streams)
    return comp(lit, seqs, modes, also=WIDE), n + sum(s[2] for s in seqs), tree


def fuzz(n, seed):
    """n frames of random block lists -> [(name, description)]"""
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n):
        blocks, produced, reps, prev, tree = [], 0, [1, 4, 8], [None] * 3, None
        for _ in range(int(rng.choice([1, 2, 3, 5, 9, 20]))):
            r = rng.random()
            if r < 0.15:
                b = raw(R(int(rng.choice([0, 1, 30, 500])), int(rng.integers(1 << 30))))
                produced += len(b["data"])
            elif r < 0.25:
                b = rle(int(rng.integers(256)), int(rng.choice([1, 2, 70, 3000])))
                produced += b["n"]
            else:
                b, add, tree = _fuzz_block(rng, produced, reps, prev, tree)
                produced += add
            blocks.append(b)
        single = rng.random() < 0.7
        fcs = None if single and rng.random() < 0.6 else int(rng.choice([4, 8]))
        out.append((f"fuzz-{seed}-{f}", frame(blocks, seed=int(rng.integers(1 << 30)), single=single, fcs=fcs, did=int(rng.choice([0, 0, 0, 1, 2, 4])))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# damaged frames
# ---------------------------------------------------------------------------------------------------------------------
def damaged():
    """[(name, the source text that must refuse it (file, text), frame bytes, Frame_Content_Size claimed)] — one defect each."""
    out = []
    rng = np.random.default_rng(31)
    P, B = "zstd_passes.h", "blosc1.c"

    def case(name, where, fd, patch=None):
        fb = bytearray(build(fd))
        if patch:
            patch(fb)
        n = fd.get("claim", sum(block_size(b) for b in fd["blocks"]))
        out.append((name, where, bytes(fb), n))

    lit = l_raw(R(20, 1))
    fill = (P, "off <= 0 || off > pos + s.ll - fr->base")
    case("offset-one-past-the-first-byte", fill, frame([comp(lit, [(6, O(7), 9)])]))
    case("offset-one-past-the-first-byte-later-block", fill, frame([raw(R(11, 2)), comp(lit, [(6, O(18), 9)])]))
    case("rep0-minus-1-is-0-concrete", (P, "if (off == 0) { afz_mark_bad(c, k->frame); return; }"), frame([comp(lit, [(4, O(1), 3), (0, 3, 5)])]))
    case("rep0-minus-1-is-0-symbolic", fill, frame([raw(R(5, 1)), comp(lit, [(0, 3, 5)])]))
    case("rep0-minus-1-is-0-symbolic-later-block", fill, frame([comp(lit, [(4, O(1), 3)]), comp(lit, [(0, 3, 5)])]))
    of31 = (P, "ofc > 30")
    case("offset-code-31", of31, frame([raw(R(30, 1)), comp(lit, [(4, 1 << 31, 5)], ("pre", "rle", "pre"))]))
    case("offset-code-31-reads-as-rep0-minus-1", of31,
         frame([comp(lit, [(9, O(4), 5)]), comp(lit, [(4, 0xFFFFFFFF, 5)], ("pre", "rle", "pre"))]))
    case("offset-code-31-from-an-fse-table", of31,
         frame([comp(lit, [(9, O(4), 5)]), comp(lit, [(4, 0xFFFFFFFF, 5)], ("pre", "fse", "pre"), norms={1: [1] * 32}, logs={1: 5})]))
    case("match-overruns-128KiB", (P, "k->lit_size + sum_ml > AFZ_BLOCK_MAX"), frame([comp(lit, [(3, O(2), BLOCK_MAX - 19)])]))
    case("more-literal-lengths-than-literals", (P, "sum_ll > k->lit_size"), frame([comp(lit, [(12, O(2), 4), (9, O(3), 4)])]))
    size = (P, "if (pos - fr->base != fr->size) afz_mark_bad(c, (int32_t)f);")
    case("decoded-size-below-fcs", size, frame([comp(lit, [(6, O(2), 9)])], claim=30))
    case("decoded-size-above-fcs", size, frame([comp(lit, [(6, O(2), 9)])], claim=28))
    case("left-over-bits-sequences", (P, "br.pos != 0 || sum_ll"), frame([comp(lit, [(6, O(2), 9)], seq_pad=3)]))
    case("left-over-byte-sequences", (P, "br.pos != 0 || sum_ll"), frame([comp(lit, [(6, O(2), 9)], seq_pad=8)]))
    case("left-over-bits-huffman", (P, "if (br.pos != 0) afz_mark_bad(c, k->frame);"), frame([comp(l_huf(draw(T5, 40, rng), T5, pad=2))]))
    case("left-over-bits-huffman-stream-2-of-4", (P, "if (br.pos != 0) afz_mark_bad(c, k->frame);"), frame([comp(l_huf(draw(T5, 40, rng), T5, streams=4, pad=5))]))
    case("sequences-stream-ends-in-0", (P, "if (!last) return -1;"), frame([comp(lit, [(6, O(2), 9)], zero_mark=True)]))
    case("huffman-stream-ends-in-0", (P, "if (!last) return -1;"), frame([comp(l_huf(draw(T5, 40, rng), T5, zero_mark=True), [(6, O(2), 9)])]))
    case("accuracy-log-above-limit-LL", (B, "malformed FSE table description"), frame([comp(lit, [(6, O(2), 9)], ("fse", "pre", "pre"), logs={0: 10})]))
    case("accuracy-log-above-limit-OF", (B, "malformed FSE table description"), frame([comp(lit, [(6, O(2), 9)], ("pre", "fse", "pre"), logs={1: 9})]))
    case("accuracy-log-above-limit-huffman-weights", (P, "afz_read_ncount(c->comp + d + 1, h, norm, 15, 6, &nsym, &lg)"),
         frame([comp(l_huf(draw(T12, 60, rng), T12, desc="fse", wlog=7))]))
    case("distribution-short-of-the-table", (B, "malformed FSE table description"),
         frame([comp(lit, [(6, O(2), 9)], ("fse", "pre", "pre"), norms={0: [1] * 36}, raw_table=True)]))
    case("weight-above-11", (P, "if (w[i] > 11) return -1;"), frame([comp(l_huf(draw([1, 1], 30, rng), [1, 1], desc_bytes=bytes([128, 0xC0])))]))
    case("weights-complete-no-tree", (P, "if (rest & (rest - 1)) return -1;"), frame([comp(l_huf(draw(T4, 30, rng), T4, desc_bytes=bytes([132, 0x11, 0x11, 0x10])))]))
    case("jump-table-longer-than-section", (P, "if (l4 < 1 || seg * 3 > n)"), frame([comp(l_huf(draw(T5, 80, rng), T5, streams=4, jump=[9, 9, 40]))]))
    case("treeless-with-nothing-before", (B, "treeless literals without an earlier Huffman table"), frame([comp(l_treeless(draw(T5, 30, rng), weights=T5))]))
    case("repeat-mode-with-nothing-before", (B, "repeat mode without an earlier table"), frame([comp(lit, [(6, O(2), 9)], ("pre", "rep", "pre"))]))
    case("repeat-mode-after-a-sequence-free-block-only", (B, "repeat mode without an earlier table"), frame([comp(lit), comp(lit, [(6, O(2), 9)], ("rep", "pre", "pre"))]))
    case("reserved-bit-frame-header", (B, "reserved frame header bit set"), frame([raw(R(20, 1))], reserved=8))
    case("reserved-bits-modes", (B, "reserved bits of the compression modes set"), frame([comp(lit, [(6, O(2), 9)], modes_reserved=1)]))
    case("block-type-3", (B, "reserved block type"), frame([raw(R(20, 1))]), patch=lambda fb: fb.__setitem__(6, fb[6] | 6))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# one batch
# ---------------------------------------------------------------------------------------------------------------------
def layout(frames, sizes, gap=40, fill=0xAB):
    """Frames back to back — the first starts at byte 0 of the compressed buffer, the last ends on its last byte, nothing is
    padded — and destinations between canaries of `gap` bytes -> (base, comp_off, comp_size, out_off, out bytes)."""
    cs = np.array([len(f) for f in frames], dtype=np.int64)
    co = np.concatenate([[0], np.cumsum(cs)[:-1]]).astype(np.int64)
    base = np.frombuffer(b"".join(frames), dtype=np.uint8).copy()
    sizes = np.asarray(sizes, dtype=np.int64)
    oo = (gap + np.concatenate([[0], np.cumsum(sizes + gap)[:-1]])).astype(np.int64)
    return base, co, cs, oo, int(gap + (sizes + gap).sum())


# ---------------------------------------------------------------------------------------------------------------------
# the file of tests/zstd_frames_check.c
# ---------------------------------------------------------------------------------------------------------------------
FUZZ_SEED, FUZZ_COUNT, MUTATED_COUNT = 8878, 300, 2000


def mutated(frames, n, seed):
    """n copies of small frames with one to three bytes changed, or cut short -> [(frame bytes, the size its source decodes to)]"""
    rng = np.random.default_rng(seed)
    small = [(f, size) for f, size in frames if 8 < len(f) < 20000 and size < 100000]
    out = []
    for it in range(n):
        f, size = small[int(rng.integers(len(small)))]
        b = bytearray(f)
        if it % 5 == 0:
            b = b[:int(rng.integers(5, len(b)))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                j = int(rng.integers(4, len(b))) if it % 5 < 3 else int(rng.integers(4, min(len(b), 40)))
                b[j] = int(rng.integers(256)) if it % 2 else b[j] ^ (1 << int(rng.integers(8)))
        out.append((bytes(b), size))
    return out


def valid_frames():
    """[(name, frame bytes, decoded bytes)] of the catalogue and the fuzz."""
    out = []
    for name, fd in [(n, fd) for n, _, fd in catalogue()] + fuzz(FUZZ_COUNT, FUZZ_SEED):
        out.append((name, build(fd), expand(fd)))
    return out


def write_check_file(path, valid=None):
    valid = valid or valid_frames()
    recs = [(0, fb, len(raw_), raw_) for _, fb, raw_ in valid]
    recs += [(1, fb, n, b"") for _, _, fb, n in damaged()]
    recs += [(2, fb, n, b"") for fb, n in mutated([(fb, len(r)) for _, fb, r in valid], MUTATED_COUNT, 4)]
    with open(path, "wb") as f:
        f.write(len(recs).to_bytes(4, "little"))
        for kind, fb, n, want in recs:
            f.write(kind.to_bytes(4, "little") + len(fb).to_bytes(4, "little") + n.to_bytes(4, "little") + fb + want)
    return len(recs)


if __name__ == "__main__":
    import sys
    print("zstd_frames: wrote", write_check_file(sys.argv[1]), "frames to", sys.argv[1])
