"""Hand-built zlib streams (RFC 1950 around RFC 1951) for the deflate route — `afcodec_inflate_plan`, the passes of
aggfly_amd/csrc/inflate_passes.h run on the host by `afcodec_inflate_emulate` and on the GPU by afhip_inflate_kernels.h.

A stream description is a list of blocks, `stored(data)`, `fixed(items)` and `dynamic(litlen_lengths, dist_lengths, items, ...)`,
or a dict {"blocks": [...], "tail": bytes after the trailer}.  Items are a literal (an int), a match `(length, distance)` or
`(length, distance, length symbol)`, and `EOB` (appended when the items do not end in it).  `build` writes the stream, `expand`
computes the bytes it means from the description alone, `strict_decode` is a strict decoder that refuses what zlib refuses and
names the classes (`CLASSES`) a stream passes through.  `catalogue`, `fuzz` and `damaged` are the permanent set; `layout` places a
batch with no padding; `write_check_file` dumps everything for tests/deflate_streams_check.c.

The pseudo-block classes follow the rule of inflate_passes.h: the front end cuts a stream's output into pseudo-blocks of at most
AFZ_BLOCK_MAX = 131,072 bytes; a block closes when it reaches 131,072 bytes exactly, or before a match that would pass them (then it
holds at least AFI_PBLOCK_MIN = 130,815 bytes, and literals that were pending stay with it as its rest).

HCLEN = 4 cannot occur in a valid stream (only the code length symbols 16, 17, 18 and 0 would have codes: every length is 0 and
there is no end-of-block code), so the catalogue reaches HCLEN 5 ... 19 and `damaged` holds the HCLEN = 4 stream."""
import bisect
import zlib

import numpy as np

import inflate_cases as ic
from inflate_cases import DIST_BASE, DIST_BITS, LEN_BASE, LEN_BITS

BLOCK_MAX = 131072                               # AFZ_BLOCK_MAX
PBLOCK_MIN = BLOCK_MAX - 257                     # AFI_PBLOCK_MIN
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
EOB = "eob"


class Invalid(Exception):
    pass


# ---------------------------------------------------------------------------------------------------------------------
# descriptions
# ---------------------------------------------------------------------------------------------------------------------
def stored(data, nlen=None, final=None, pad_value=0):
    return {"type": 0, "data": bytes(data), "nlen": nlen, "final": final, "pad_value": pad_value}


def _items(items, eob):
    items = list(items)
    if eob and (not items or items[-1] != EOB):
        items.append(EOB)
    return items


def fixed(items, eob=True, final=None):
    return {"type": 1, "items": _items(items, eob), "final": final}


def table(n, lengths):
    """n code lengths, {symbol: length} the ones that are not 0."""
    out = [0] * n
    for s, l_ in lengths.items():
        out[s] = l_
    return out


def dynamic(litlen_lengths, dist_lengths, items, hclen=None, cl_lengths=None, cl_syms=None, eob=True, final=None, hlit=None, hdist=None):
    """hclen: the count of code length code lengths written (4 ... 19); cl_lengths: {code length symbol: length} of the code length
    code; cl_syms: the exact symbols that write the lengths, plain ones as ints, 16 / 17 / 18 as (symbol, extra value).  Each
    default derives a valid one."""
    return {"type": 2, "ll": list(litlen_lengths), "dl": list(dist_lengths), "items": _items(items, eob), "hclen": hclen,
            "cl_lengths": cl_lengths, "cl_syms": cl_syms, "final": final, "hlit": hlit, "hdist": hdist}


def _norm(desc):
    return desc if isinstance(desc, dict) else {"blocks": desc}


def R(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def len_symbol(length):
    return 285 if length == 258 else 256 + bisect.bisect_right(LEN_BASE, length, 0, 28)


def dist_symbol(dist):
    return bisect.bisect_right(DIST_BASE, dist) - 1


def balanced(symbols):
    """{symbol: length} of a complete code over the symbols, lengths differing by one at the most (a lone symbol: one bit)."""
    symbols = list(symbols)
    k = len(symbols)
    if k == 1:
        return {symbols[0]: 1}
    m = max(1, (k - 1).bit_length())
    short = (1 << m) - k
    return {s: (m - 1 if i < short else m) for i, s in enumerate(symbols)}


def used_symbols(items):
    ll, dd = set(), set()
    for it in items:
        if it.__class__ is int:
            ll.add(it)
        elif it == EOB:
            ll.add(256)
        elif not isinstance(it[0], str):
            ll.add(it[2] if len(it) > 2 else len_symbol(it[0]))
            dd.add(dist_symbol(it[1]))
    return ll, dd


def auto_dynamic(items, code=balanced, nl=None, nd=None, **kw):
    """A dynamic block whose tables hold exactly the symbols the items use: no distance code when there is no match, one code of
    one bit for a single distance symbol."""
    items = _items(items, True)
    ll, dd = used_symbols(items)
    lt = code(sorted(ll))
    dt = code(sorted(dd)) if dd else {}
    return dynamic(table(nl or max(257, max(ll) + 1), lt), table(nd or (max(dd) + 1 if dd else 1), dt), items, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# expand: the bytes a description means
# ---------------------------------------------------------------------------------------------------------------------
def _copy(out, length, dist):
    n = len(out)
    if dist < 1 or dist > n:
        raise ValueError("distance before the start")
    if dist >= length:
        out += out[n - dist:n - dist + length]
    else:
        out += (bytes(out[n - dist:]) * (length // dist + 1))[:length]


def expand(desc):
    out = bytearray()
    for b in _norm(desc)["blocks"]:
        if b["type"] == 0:
            out += b["data"]
            continue
        for it in b["items"]:
            if it.__class__ is int:
                out.append(it)
            elif it == EOB:
                break
            elif not isinstance(it[0], str):
                _copy(out, it[0], it[1])
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------------
# build: the writer
# ---------------------------------------------------------------------------------------------------------------------
class Writer(ic.Bits):
    """`inflate_cases.Bits` with the finished bytes moved out of the accumulator (a stream of 400 KB stays linear), and the bit
    ranges of the fields it wrote (`marks`: name, first bit, bit after)."""

    def __init__(self):
        super().__init__()
        self.buf, self.marks = bytearray(), []

    def put(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        if self.n >= 512:
            self.flush()

    def flush(self):
        k = self.n >> 3
        self.buf += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
        self.acc >>= 8 * k
        self.n -= 8 * k

    @property
    def pos(self):
        return 8 * len(self.buf) + self.n

    def mark(self, name, start):
        self.marks.append((name, start, self.pos))

    def bytes(self):
        self.flush()
        return bytes(self.buf) + self.acc.to_bytes((self.n + 7) // 8, "little")


def codes(lengths):
    """{symbol: (the canonical code's bits in stream order, length)} (RFC 1951 §3.2.2)"""
    cnt = [0] * 17
    for l_ in lengths:
        cnt[l_] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for l_ in range(1, 16):
        code = (code + cnt[l_ - 1]) << 1
        nxt[l_] = code
    out = {}
    for s, l_ in enumerate(lengths):
        if l_:
            c = nxt[l_] & ((1 << l_) - 1)
            nxt[l_] += 1
            out[s] = (int(format(c, "0%db" % l_)[::-1], 2), l_)
    return out


FIXED_CODES = (codes(FIXED_LL), codes(FIXED_D))


def cl_symbols(lengths):
    """A valid list of code length symbols for the lengths: [(symbol, extra value or None)], runs taken greedily."""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, None))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
        out += [(v, None)] * run
        i = j
    return out


def _cl_norm(cl_syms):
    return [(s, None) if s.__class__ is int else (s[0], s[1]) for s in cl_syms]


def lengths_of(cl_syms):
    """The code lengths that a list of code length symbols writes."""
    out = []
    for sy, ex in _cl_norm(cl_syms):
        if sy < 16:
            out.append(sy)
        elif sy == 16:
            out += [out[-1]] * (3 + ex)
        else:
            out += [0] * ((3 if sy == 17 else 11) + ex)
    return out


def from_cl(cl_syms, nl, items, **kw):
    """A dynamic block described by its code length symbols: the first nl lengths are the literal/length table."""
    lens = lengths_of(cl_syms)
    return dynamic(lens[:nl], lens[nl:], items, cl_syms=cl_syms, **kw)


def _write_items(w, items, lenc, denc):
    put = w.put
    for it in items:
        if it.__class__ is int:
            c, l_ = lenc[it]
            put(c, l_)
        elif it == EOB:
            s = w.pos
            put(*lenc[256])
            w.mark("eob", s)
        elif it[0] == "L":                        # a literal/length symbol as it stands
            s = w.pos
            put(*lenc[it[1]])
            w.mark("raw_sym", s)
        elif it[0] == "D":                        # a distance code as it stands
            put(*denc[it[1]])
        elif it[0] == "bits":
            put(it[1], it[2])
        else:
            length, dist = it[0], it[1]
            ls = it[2] if len(it) > 2 else len_symbol(length)
            extra = length - LEN_BASE[ls - 257]
            assert 0 <= extra < (1 << LEN_BITS[ls - 257]) or (extra == 0 and LEN_BITS[ls - 257] == 0), it
            s = w.pos
            put(*lenc[ls])
            w.mark("len_sym", s)
            if LEN_BITS[ls - 257]:
                s = w.pos
                put(extra, LEN_BITS[ls - 257])
                w.mark("len_extra", s)
            ds = dist_symbol(dist)
            s = w.pos
            put(*denc[ds])
            w.mark("dist_sym", s)
            if DIST_BITS[ds]:
                s = w.pos
                put(dist - DIST_BASE[ds], DIST_BITS[ds])
                w.mark("dist_extra", s)


def _write_dynamic(w, b):
    ll, dl = b["ll"], b["dl"]
    nl = len(ll) if b["hlit"] is None else b["hlit"]
    nd = len(dl) if b["hdist"] is None else b["hdist"]
    syms = _cl_norm(b["cl_syms"]) if b["cl_syms"] is not None else cl_symbols(ll + dl)
    cll = b["cl_lengths"]
    if cll is None:
        used = sorted({s for s, _ in syms})
        if len(used) < 2:                                          # zlib refuses an incomplete code length code
            used.append(next(s for s in CL_ORDER if s not in used))
        cll = balanced(used)
    cll = table(19, cll) if isinstance(cll, dict) else list(cll)
    hclen = b["hclen"]
    if hclen is None:
        hclen = max([4] + [i + 1 for i in range(19) if cll[CL_ORDER[i]]])
    s = w.pos
    w.put(nl - 257, 5)
    w.mark("hlit", s)
    s = w.pos
    w.put(nd - 1, 5)
    w.mark("hdist", s)
    s = w.pos
    w.put(hclen - 4, 4)
    w.mark("hclen", s)
    s = w.pos
    for i in range(hclen):
        w.put(cll[CL_ORDER[i]], 3)
    w.mark("cl_lengths", s)
    cenc = codes(cll)
    s = w.pos
    for sy, ex in syms:
        w.put(*cenc[sy])
        if sy >= 16:
            w.put(ex, {16: 2, 17: 3, 18: 7}[sy])
    w.mark("code_lengths", s)
    if b["items"]:
        _write_items(w, b["items"], codes(ll), codes(dl))


def deflate(desc):
    """-> (the deflate bytes, the writer's marks)"""
    blocks = _norm(desc)["blocks"]
    w = Writer()
    for i, b in enumerate(blocks):
        final = b["final"] if b["final"] is not None else int(i == len(blocks) - 1)
        s = w.pos
        w.put(final, 1)
        w.put(b["type"], 2)
        w.mark("block_header", s)
        if b["type"] == 0:
            pad = -w.pos % 8
            w.put(b["pad_value"], pad)
            s = w.pos
            n = b.get("len", len(b["data"]))
            w.put(n, 16)
            w.put((~n & 0xffff) if b["nlen"] is None else b["nlen"], 16)
            w.mark("stored_header", s)
            w.flush()
            w.buf += b["data"]
        elif b["type"] == 1:
            _write_items(w, b["items"], *FIXED_CODES)
        elif b["type"] == 2:
            _write_dynamic(w, b)
    return w.bytes(), w.marks


def build(desc):
    """The zlib stream: 78 9C, the deflate blocks, the Adler-32 of `expand(desc)`, the description's "tail" behind it."""
    d = _norm(desc)
    body, _ = deflate(d)
    means = d["means"] if "means" in d else expand(d)
    return b"\x78\x9c" + body + zlib.adler32(means).to_bytes(4, "big") + d.get("tail", b"")


# ---------------------------------------------------------------------------------------------------------------------
# strict_decode: RFC 1950 / 1951 as zlib enforces them
# ---------------------------------------------------------------------------------------------------------------------
_FB = 9


def _decoder(lengths, kind):
    """Decode tables of a code -> (fast, slow, lengths used).  kind "cl": must be complete; "ll": incomplete only as one code of
    one bit; "d": the same, or no code at all (zlib: inflate_table)."""
    cnt = [0] * 16
    for l_ in lengths:
        cnt[l_] += 1
    left = 1
    for l_ in range(1, 16):
        left = (left << 1) - cnt[l_]
        if left < 0:
            raise Invalid("over-subscribed code")
    ncodes = len(lengths) - cnt[0]
    if left > 0:
        lone = ncodes == 1 and cnt[1] == 1
        if kind == "cl" or not (lone or (kind == "d" and ncodes == 0)):
            raise Invalid("incomplete code")
    fast, slow = [None] * (1 << _FB), {}
    for s, (c, l_) in codes(lengths).items():
        if l_ <= _FB:
            e = (s, l_)
            for k in range(c, 1 << _FB, 1 << l_):
                fast[k] = e
        else:
            slow[(l_, c)] = s
    return fast, slow


_FIXED_DEC = None


def strict_decode(stream, info=None):
    """-> (the decoded bytes, the set of classes the stream passed through); raises `Invalid` for everything zlib refuses.
    info (a dict) receives "unused" (the bytes behind the trailer) and "pblocks" (the sizes of the pseudo-blocks by the rule of
    the module's docstring)."""
    global _FIXED_DEC
    if len(stream) < 2:
        raise Invalid("shorter than a zlib header")
    if stream[0] & 15 != 8 or stream[0] >> 4 > 7 or ((stream[0] << 8) | stream[1]) % 31:
        raise Invalid("not a zlib header")
    if stream[1] & 0x20:
        raise Invalid("preset dictionary")
    body = stream[2:]
    total = 8 * len(body)
    padded = body + b"\0\0\0\0"
    pos = 0
    cls = set()
    out = bytearray()
    cur = pend = pb_start = 0                      # the pseudo-block model
    pblocks = []
    stored_ranges = []

    def take(n):
        nonlocal pos
        v = (int.from_bytes(padded[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        if pos > total:
            raise Invalid("the input ends too soon")
        return v

    def symbol(dec):
        nonlocal pos
        v = (int.from_bytes(padded[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7))
        e = dec[0][v & ((1 << _FB) - 1)]
        if e is None:
            slow = dec[1]
            for l_ in range(_FB + 1, 16):
                s = slow.get((l_, v & ((1 << l_) - 1)))
                if s is not None:
                    e = (s, l_)
                    break
            else:
                raise Invalid("bits that are no code")
        pos += e[1]
        if pos > total:
            raise Invalid("the input ends too soon")
        return e

    def close():
        nonlocal cur, pend, pb_start
        pblocks.append(cur)
        cur = pend = 0
        pb_start = len(out)

    def literals(n, is_stored):
        nonlocal cur, pend
        left = n
        while left:
            k = min(left, BLOCK_MAX - cur)
            cur += k
            pend += k
            left -= k
            if cur == BLOCK_MAX:
                cls.add(("cut", "literal-reaches-131072"))
                close()
                if left and is_stored:
                    cls.add(("stored", "across-cut"))

    final, kinds = 0, []
    tot_lit = tot_match = 0
    all3 = True
    while not final:
        final, btype = take(1), take(2)
        kinds.append(btype)
        if btype == 3:
            raise Invalid("block type 3")
        if btype == 0:
            cls.add(("stored_pad", -pos % 8))
            pos += -pos % 8
            n, nn = take(16), take(16)
            if n != (~nn & 0xffff):
                raise Invalid("LEN != ~NLEN")
            if pos + 8 * n > total:
                raise Invalid("the input ends too soon")
            if n in (0, 1, 65535):
                cls.add(("stored_len", n))
            stored_ranges.append((len(out), len(out) + n))
            out += body[pos >> 3:(pos >> 3) + n]
            literals(n, True)
            tot_lit += n
            pos += 8 * n
            continue
        if btype == 1:
            if _FIXED_DEC is None:
                _FIXED_DEC = (_decoder(FIXED_LL, "fixed"), _decoder(FIXED_D, "fixed"))
            ldec, ddec = _FIXED_DEC
            if len(kinds) >= 2 and kinds[-2] == 1:
                cls.add(("tables", "fixed-after-fixed"))
            coded = [k for k in kinds if k]
            if len(coded) >= 3 and coded[-3:] == [1, 2, 1]:
                cls.add(("tables", "fixed-after-dynamic-after-fixed"))
            one_d = no_d = False
        else:
            nl, nd, nc = take(5) + 257, take(5) + 1, take(4) + 4
            if nl > 286 or nd > 30:
                raise Invalid("too many length or distance symbols")
            cls.update((("hlit", nl), ("hdist", nd), ("hclen", nc)))
            cl = [0] * 19
            for i in range(nc):
                cl[CL_ORDER[i]] = take(3)
            if not any(cl):
                raise Invalid("no code length code")       # (zlib reads every length as 0 then and misses the end-of-block code)
            cdec = _decoder(cl, "cl")
            lens = []
            while len(lens) < nl + nd:
                sy, l_ = symbol(cdec)
                cls.add(("cl_len", l_))
                at = len(lens)
                if sy < 16:
                    lens.append(sy)
                    continue
                if sy == 16:
                    if not lens:
                        raise Invalid("repeat with no length before it")
                    ex = take(2)
                    lens += [lens[-1]] * (3 + ex)
                    if at == nl:
                        cls.add(("cl16_first_distance",))
                else:
                    ex = take(3) if sy == 17 else take(7)
                    lens += [0] * ((3 if sy == 17 else 11) + ex)
                    if at < nl < len(lens):
                        cls.add(("cl_run_across", sy))
                cls.add(("cl_sym", sy, ex))
                if len(lens) > nl + nd:
                    raise Invalid("repeat past the announced counts")
                if len(lens) == nl + nd:
                    cls.add(("cl_run_ends_at_total",))
            if lens[256] == 0:
                raise Invalid("no end-of-block code")
            ldec, ddec = _decoder(lens[:nl], "ll"), _decoder(lens[nl:], "d")
            dn = [x for x in lens[nl:] if x]
            no_d, one_d = not dn, dn == [1]
            if dn == [1, 1]:
                cls.add(("dtable", "two-1bit"))
            if len(dn) == 30:
                cls.add(("dtable", "30-codes"))
            if sum(1 for x in lens[:nl] if x) == 1:
                cls.add(("ltable", "eob-only"))
            if len(kinds) >= 2 and kinds[-2] == 2:
                cls.add(("tables", "dynamic-after-dynamic"))
        n_match = 0
        while True:
            sy, l_ = symbol(ldec)
            cls.add(("ll_len", l_))
            if sy < 256:
                out.append(sy)
                tot_lit += 1
                cur += 1
                pend += 1
                if cur == BLOCK_MAX:
                    cls.add(("cut", "literal-reaches-131072"))
                    close()
                continue
            if sy == 256:
                break
            if sy > 285:
                raise Invalid("length symbol 286 or 287")
            i = sy - 257
            ex = take(LEN_BITS[i])
            length = LEN_BASE[i] + ex
            if ex == 0:
                cls.add(("len_sym", sy, "min"))
            if ex == (1 << LEN_BITS[i]) - 1:
                cls.add(("len_sym", sy, "max"))
            if length == 258:
                cls.add(("len258", sy))
            ds, l_ = symbol(ddec)
            cls.add(("d_len", l_))
            if ds > 29:
                raise Invalid("distance code 30 or 31")
            ex = take(DIST_BITS[ds])
            dist = DIST_BASE[ds] + ex
            if ex == 0:
                cls.add(("dist_sym", ds, "min"))
            if ex == (1 << DIST_BITS[ds]) - 1:
                cls.add(("dist_sym", ds, "max"))
            have = len(out)
            if dist > have:
                raise Invalid("distance before the start")
            n_match += 1
            tot_match += 1
            all3 = all3 and length == 3
            if dist == have:
                cls.add(("match", "distance-is-all-decoded"))
            if dist == 1 and length == 258:
                cls.add(("match", "distance-1-length-258"))
            if dist < length:
                cls.add(("match", "overlap"))
            if dist == 32768:
                cls.add(("match", "distance-32768"))
            if any(a <= have - dist and have - dist + min(length, dist) <= b_ for a, b_ in stored_ranges):
                cls.add(("match", "source-in-stored"))
            if btype == 2 and one_d:
                cls.add(("dtable", "one-1bit-used"))
            if cur + length > BLOCK_MAX:
                cls.add(("cut", "match-closes-at", cur))
                if pend:
                    cls.add(("cut", "pending-literals-rest"))
                close()
            if dist > have - pb_start:
                cls.add(("match", "source-in-previous-pblock"))
            _copy(out, length, dist)
            cur += length
            pend = 0
            if cur == BLOCK_MAX:
                cls.add(("cut", "match-reaches-131072"))
                close()
        if btype == 2 and no_d and n_match == 0 and sum(1 for x in lens[:nl] if x) > 1:
            cls.add(("dtable", "none-literals-only"))
        if final:
            cls.add(("eob_bit", pos % 8))
    pblocks.append(cur)
    for i, k in enumerate(kinds):
        where = []
        if i == 0:
            where.append("first")
        if i == len(kinds) - 1:
            where.append("final")
        if 0 < i < len(kinds) - 1:
            where.append("middle")
        if len(kinds) >= 3:
            cls.update(("block", k, w_) for w_ in where)
    pos += -pos % 8
    if pos + 32 > total:
        raise Invalid("the input ends before the trailer")
    if int.from_bytes(body[pos >> 3:(pos >> 3) + 4], "big") != zlib.adler32(bytes(out)):
        raise Invalid("Adler-32")
    unused = body[(pos >> 3) + 4:]
    n = len(out)
    if unused:
        cls.add(("trailing-bytes",))
    if n in SIZES:
        cls.add(("size", n))
    if len(stream) - len(unused) <= 12:
        cls.add(("csize", len(stream) - len(unused)))
    if tot_lit == 1 and tot_match and all3:
        cls.add(("records-at-most",))
    for p0 in range(0, n - 65535, 65536):
        if out[p0:p0 + 65536] == b"\xff" * 65536:
            cls.add(("adler", "piece-of-0xff"))
    if info is not None:
        info["unused"] = bytes(unused)
        info["pblocks"] = pblocks
    return bytes(out), cls


SIZES = (0, 65535, 65536, 65537, BLOCK_MAX, 2 * BLOCK_MAX, PBLOCK_MIN - 1, PBLOCK_MIN, 2 * PBLOCK_MIN - 1, 2 * PBLOCK_MIN)

CLASSES = (
    [("block", t, w) for t in (0, 1, 2) for w in ("first", "middle", "final")] +
    [("tables", k) for k in ("fixed-after-fixed", "fixed-after-dynamic-after-fixed", "dynamic-after-dynamic")] +
    [("stored_pad", k) for k in range(8)] + [("stored_len", k) for k in (0, 1, 65535)] + [("stored", "across-cut")] +
    [("ll_len", k) for k in range(1, 16)] + [("d_len", k) for k in range(1, 16)] + [("cl_len", k) for k in range(1, 8)] +
    [("len_sym", s, e) for s in range(257, 286) for e in ("min", "max")] + [("len258", 285), ("len258", 284)] +
    [("dist_sym", s, e) for s in range(30) for e in ("min", "max")] +
    [("hlit", k) for k in (257, 259, 262, 286)] + [("hdist", 1), ("hdist", 30)] + [("hclen", k) for k in range(5, 20)] +
    [("cl_sym", 16, 0), ("cl_sym", 16, 3), ("cl_sym", 17, 0), ("cl_sym", 17, 7), ("cl_sym", 18, 0), ("cl_sym", 18, 127)] +
    [("cl16_first_distance",), ("cl_run_across", 17), ("cl_run_across", 18), ("cl_run_ends_at_total",)] +
    [("dtable", k) for k in ("none-literals-only", "one-1bit-used", "two-1bit", "30-codes")] + [("ltable", "eob-only")] +
    [("match", k) for k in ("distance-is-all-decoded", "distance-1-length-258", "overlap", "distance-32768", "source-in-stored",
                            "source-in-previous-pblock")] +
    [("cut", "literal-reaches-131072"), ("cut", "match-closes-at", PBLOCK_MIN), ("cut", "match-closes-at", BLOCK_MAX - 1),
     ("cut", "pending-literals-rest"), ("cut", "match-reaches-131072")] +
    [("size", n) for n in SIZES] + [("records-at-most",), ("adler", "piece-of-0xff")] +
    [("eob_bit", k) for k in range(8)] + [("csize", k) for k in range(8, 13)] + [("trailing-bytes",)])


# ---------------------------------------------------------------------------------------------------------------------
# catalogue
# ---------------------------------------------------------------------------------------------------------------------
LAUNCH_GEOMETRY = ("size-0-smallest-chunk", "cut-literal-reaches-131072", "cut-match-closes-at-130815", "cut-match-closes-at-131071",
                   "cut-pending-literals-rest", "cut-match-reaches-131072", "stored-across-two-cuts", "adler-65535", "adler-65536",
                   "adler-65537")
JUMP_BOUND = ("jump-bound-2^18", "jump-bound-2^18+1")
MULTI_PBLOCK = ("cut-literal-reaches-131072", "size-2x130815")          # the two that go through the shuffle scratch on the GPU


def text(s):
    return list(s.encode())


def chain(n, byte=0x5A):
    """One literal, then matches of length 258 at distance 1 (and one shorter to land on n bytes)."""
    full, rest = divmod(n - 1, 258)
    return [byte] + [(258, 1)] * full + ([(rest, 1)] if rest >= 3 else [byte] * rest)


def catalogue():
    """[(name, what it is there for, description)]"""
    out = []

    def add(name, why, desc):
        out.append((name, why, desc))

    abc = text("abcabc")
    dyn = auto_dynamic
    # block kinds at every place of a stream
    add("stored-fixed-dynamic", "types 0 / 1 / 2 as first / middle / final", [stored(b"first"), fixed(text("mid") + [(5, 3)]), dyn(text("end") + [(4, 8)])])
    add("dynamic-stored-fixed", "types 2 / 0 / 1", [dyn(text("hello hello") + [(6, 6)]), stored(b"middle"), fixed([(9, 6), 33])])
    add("fixed-dynamic-stored", "types 1 / 2 / 0", [fixed(abc + [(3, 3)]), dyn([(7, 2)] + text("xyz")), stored(b"the end")])
    add("fixed-fixed", "the fixed tables built once and used again", [fixed(abc), fixed([(6, 3), 200]), fixed([(30, 7), 255, 0])])
    add("fixed-dynamic-fixed", "the fixed tables built again after a dynamic block took the slot",
        [fixed(abc + [(4, 2)]), dyn(text("qrs") + [(5, 9)]), fixed([(258, 12), 143, 144, 255, (3, 1)])])
    add("dynamic-dynamic", "two dynamic blocks in a row, other tables", [dyn(text("aabbcc") + [(4, 2)]), dyn(text("zyxwvut") + [(12, 5), (3, 13)]), fixed([])])
    add("fixed-stored-fixed", "a stored block between does not touch the fixed tables", [fixed(abc), stored(b"--"), fixed([(8, 8), 1])])
    # stored blocks
    for b in range(8):
        add("stored-padding-%d" % ((-(10 + 9 * b + 3)) % 8), "padding bits before LEN", [fixed([200] * b), stored(b"padded"), fixed([(6, 6)])])
    add("stored-padding-of-ones", "the padding bits are not looked at", [fixed([200] * 3), stored(b"ones", pad_value=0xff), fixed([7])])
    add("stored-len-0-first-middle-final", "LEN 0 at every place", [stored(b""), fixed(abc), stored(b""), fixed([(3, 3)]), stored(b"")])
    add("stored-len-1", "LEN 1", [stored(b"x"), stored(b"y"), fixed([(3, 2)])])
    add("stored-len-65535", "the largest stored block", [stored(R(65535, 1))])
    add("stored-across-two-cuts", "stored blocks that lie across pseudo-block cuts", [stored(R(65535, 2)), stored(R(65535, 3)), stored(R(65535, 4)), stored(R(65535, 5)), stored(R(9, 6))])
    # code lengths
    lits = list(range(97, 111))
    for name, order in (("ascending", lits + [257, 256]), ("descending", [256, 257] + lits[::-1])):
        lt = {s: min(i + 1, 15) for i, s in enumerate(order)}
        dorder = list(range(16)) if name == "ascending" else list(range(15, -1, -1))
        dt = {s: min(i + 1, 15) for i, s in enumerate(dorder)}
        items = lits + [(3, DIST_BASE[s]) for s in range(16)] + lits
        add("code-lengths-1-to-15-" + name, "literal/length and distance codes of every length, past AFI_FAST on both tables",
            [stored(R(300, 7)), dynamic(table(258, lt), table(16, dt), items)])
    cl7 = {0: 1, 18: 2, 1: 3, 2: 4, 3: 5, 4: 6, 5: 7, 6: 7}
    add("cl-lengths-1-to-7", "code length codes of every length",
        [dynamic(table(262, {97: 1, 98: 2, 256: 3, 257: 4, 258: 5, 260: 6, 261: 6}), [0], text("abba"), cl_lengths=cl7)])
    add("cl-lengths-7-to-1", "the same, the long codes on the plain lengths", [dynamic(table(262, {97: 1, 98: 2, 256: 3, 257: 4, 258: 5, 260: 6, 261: 6}), [0], text("baab"),
                                                                                        cl_lengths={6: 1, 5: 2, 4: 3, 3: 4, 2: 5, 1: 6, 0: 7, 18: 7})])
    # every length and distance symbol with its least and greatest extra value
    pairs = [(s, e) for s in range(30) for e in (0, (1 << DIST_BITS[s]) - 1)]
    lpairs = [(s, e) for s in range(29) for e in (0, (1 << LEN_BITS[s]) - 1)]
    items = [(LEN_BASE[lpairs[i % len(lpairs)][0]] + lpairs[i % len(lpairs)][1], DIST_BASE[s] + e, 257 + lpairs[i % len(lpairs)][0]) for i, (s, e) in enumerate(pairs)]
    add("every-symbol-fixed", "length symbols 257 ... 285 and distance symbols 0 ... 29, least and greatest extra", [stored(R(32768, 8)), fixed(items)])
    add("every-symbol-dynamic-hlit-286-hdist-30", "the same under tables of 286 and 30 codes",
        [stored(R(32768, 9)), dynamic(table(286, balanced(range(286))), table(30, balanced(range(30))), items[::-1] + [0, 255])])
    add("length-258-as-284-plus-31", "the form zlib never writes", [fixed(abc + [(258, 3, 284), (258, 3), (258, 1, 284)]), dyn(abc + [(258, 2, 284), (258, 6)])])
    # header counts
    add("hlit-257-hdist-1", "the smallest tables", [dynamic(table(257, balanced([65, 66, 67, 256])), [0], text("ABCCBA"))])
    add("hlit-259", "HLIT between the ends, one distance code", [dynamic(table(259, balanced([65, 256, 258])), [1], [65, (4, 1), 65])])
    for k in range(5, 20):
        v = CL_ORDER[k - 1]
        if v < 8:
            lt = {s: 8 for s in range(256 - (1 << (8 - v)))}
            lt[256] = v
        elif v == 8:
            lt = {s: 8 for s in range(255)}
            lt[256] = 8
        else:
            lt = {s: 8 for s in range(255)}
            for j, l_ in enumerate(list(range(9, v)) + [v, v]):
                lt[256 + j] = l_
        plain = [(x, None) for x in table(max(lt) + 1, lt) + [0]]
        add("hclen-%d" % k, "HCLEN %d: the last code length code length written is that of %d" % (k, v),
            [dynamic(table(max(lt) + 1, lt), [0], [0, 1, 2, 100], hclen=k, cl_syms=plain if k % 2 else None)])
    # code length symbols
    add("cl-16-first-distance-length", "16 as the first distance length copies the last literal/length length; the run ends at nl + nd",
        [from_cl([(18, 86), 1, (18, 127), (18, 9), 3, 3, 2, (16, 1)], 259, [97, (3, 1), (4, 2), (3, 3), (4, 4)])])
    add("cl-17-across-the-boundary", "a run of 17 over the last literal/length and the first distance lengths",
        [from_cl([(18, 86), 1, (18, 127), (18, 9), 2, 3, 3, (17, 2), 1, 1], 262, [97, 97, 97, 97, (3, 3), (4, 4)])])
    add("cl-18-across-the-boundary", "a run of 18 over the boundary",
        [from_cl([(18, 86), 1, (18, 127), (18, 9), 2, 2, (18, 7), 1, 1], 270, [97] * 16 + [(3, 9), (3, 13), (3, 16)])])
    add("cl-repeat-extremes", "16 with 0 and 3, 17 with 0 and 7, 18 with 0 and 127; the last symbol is a run that ends at nl + nd",
        [from_cl([(18, 127), 8, (16, 3), (17, 7), 8, (16, 0), (18, 0), (17, 0), (18, 72), 1, 2, 3, 4, 0, 6, 8, 1, 1, (17, 0)], 263,
                 [138, 144, 155, 158, (3, 1), (4, 2), (5, 1), (7, 2), (8, 1)])])
    # small and odd tables
    add("no-distance-code-literals-only", "HDIST 1 with a length of 0", [dynamic(table(257, balanced([48, 49, 256])), [0], text("0110100"))])
    add("one-distance-code-of-one-bit", "the incomplete table zlib lets through, used", [dynamic(table(258, balanced([120, 256, 257])), [1], [120, (3, 1), 120, (3, 1)])])
    add("one-distance-code-of-one-bit-symbol-3", "the lone code on distance symbol 3", [dynamic(table(259, balanced([1, 2, 3, 4, 256, 258])), [0, 0, 0, 1], [1, 2, 3, 4, (4, 4), (4, 4)])])
    add("two-distance-codes-of-one-bit", "the smallest complete distance table", [dynamic(table(260, balanced([7, 8, 256, 259])), [1, 1], [7, 8, (5, 1), (5, 2)])])
    add("thirty-distance-codes", "every distance symbol has a code", [stored(R(700, 10)), dynamic(table(258, balanced([9, 256, 257])), table(30, balanced(range(30))), [9, (3, 600), (3, 1), (3, 24)])])
    eob_only = lambda: dynamic(table(257, {256: 1}), [0], [])                                     # noqa: E731
    add("empty-dynamic-blocks", "a literal/length table of the end-of-block code alone, first, middle and final", [eob_only(), fixed(abc), eob_only(), stored(b"z"), eob_only()])
    add("empty-dynamic-block-alone", "decoded size 0 from a dynamic block", [eob_only()])
    # matches
    add("match-distance-is-all-decoded", "the source is the stream's first byte", [fixed(text("wxyz") + [(4, 4), (8, 8), (16, 16), (258, 32)])])
    add("match-distance-1-length-258", "the longest run of one byte", [fixed([0, (258, 1), 1, (258, 1)])])
    add("matches-overlapping", "distances below the length", [fixed(text("abcde") + [(10, 2), (7, 3), (258, 5), (5, 4), (100, 99), (258, 257)])])
    add("match-distance-32768", "the farthest source, inside a stored block", [stored(R(32768, 11)), fixed([(258, 32768), (3, 32768), (200, 32768)]), dyn([(17, 32768), 4])])
    add("match-source-in-stored", "matches that read the bytes of stored blocks", [stored(b"0123456789"), fixed([(5, 10), (3, 7)]), stored(b"ab"), fixed([(4, 2)])])
    # pseudo-block cuts
    a, b_ = R(65535, 12), R(65535, 13)
    add("cut-literal-reaches-131072", "a literal closes the block; the next match reads the block before",
        [stored(a), stored(b_), fixed([1, 2, 3, 4, 5, (10, 100), (258, 30000), 6]), stored(R(60000, 14)), fixed([(258, 32768), (40, 1)])])
    add("size-131072", "a stream that ends on the cut: its last pseudo-block is empty", [stored(a), stored(b_), fixed([7, 9])])
    add("cut-match-closes-at-130815", "a match of 258 that would pass the limit closes the smallest block there is; its literals are the block's rest",
        [stored(a), stored(b_[:65280]), fixed([(258, 1), 5])])
    add("cut-match-closes-at-131071", "a match of 3 one byte before the limit, no literal pending", [stored(a), stored(b_[:65533]), fixed([(3, 5), (3, 1), 8])])
    add("cut-pending-literals-rest", "literals of a stored and a fixed block pending when the block closes", [stored(a), stored(b_[:65465]), fixed([1, 2, 3, 4, 5, (258, 7), (9, 300)])])
    add("cut-match-reaches-131072", "a match ends on the limit and literals follow", [stored(a), stored(b_[:65534]), fixed([(3, 9), 1, 2, 3, 4, 5, (4, 6), 9, (20, 12)])])
    add("size-130814", "one byte short of AFI_PBLOCK_MIN: one pseudo-block slot", [stored(a), stored(b_[:65279]), fixed([])])
    add("size-130815", "AFI_PBLOCK_MIN exactly: two slots, the second stays empty", [stored(a), stored(b_[:65280]), fixed([])])
    add("size-2x130815-1", "both pseudo-block slots used, the first closed at 130,815", [stored(a), stored(b_[:65280]), fixed([(258, 3)]), stored(a), stored(b_[:65021])])
    add("size-2x130815", "three slots, two used", [stored(a), stored(b_[:65280]), fixed([(258, 3)]), stored(a), stored(b_[:65022])])
    add("records-at-most-small", "one literal, then matches of 3 alone", [fixed([0x41] + [(3, 1)] * 200)])
    add("records-at-most-across-a-cut", "the same over a cut: the sequence records sit at dsize / 3", [fixed([0x42] + [(3, 1)] * 43700)])
    for n in (1 << 18, (1 << 18) + 1):
        add("jump-bound-2^18" + ("+1" if n & 1 else ""), "a distance-1 chain as long as the stream (2 x 131,072 bytes and one more)", [fixed(chain(n))])
    # Adler-32
    add("adler-65535", "one piece, one byte short", [stored(R(65535, 15))])
    add("adler-65536", "exactly one piece", [stored(R(65535, 16)), fixed([0x55])])
    add("adler-65537", "one byte in the second piece", [stored(R(65535, 17)), fixed([0x55, 0xAA])])
    add("adler-piece-of-0xff", "the largest partial sums", [fixed(chain(65536, 0xFF) + [0xFF, 0xFE, (20, 1)])])
    # the bit reader
    add("size-0-smallest-chunk", "an empty fixed block: a chunk of 8 bytes, read by afi_ld64's byte-wise arm", [fixed([])])
    for k in range(1, 8):
        add("eob-bit-%d-chunk-%d" % ((2 + k) % 8, 8 + (10 + 9 * k + 7) // 8 - 2), "the final end-of-block ends on this bit of its byte", [fixed([144 + k] * k)])
    add("eob-bit-2-long", "eight literals of 9 bits bring the end back to bit 2", [fixed([150] * 8)])
    add("chunk-9", "one literal: 9 bytes", [fixed([3])])
    add("chunk-11-stored-empty", "decoded size 0 from a stored block", [stored(b"")])
    add("bytes-after-the-trailer", "anything after the trailer is ignored", {"blocks": [fixed(abc + [(5, 2)])], "tail": b"\x01\x02\x03trailing"})
    add("one-byte-after-the-trailer", "a single byte behind the trailer", {"blocks": [stored(b"s")], "tail": b"\xff"})
    return out


# ---------------------------------------------------------------------------------------------------------------------
# fuzz
# ---------------------------------------------------------------------------------------------------------------------
FUZZ_SEED, FUZZ_COUNT, MUTATED_COUNT = 1951, 300, 2000


def random_code(rng, maxbits=15):
    def code(symbols):
        n = len(symbols)
        if n == 1:
            return {symbols[0]: 1}
        leaves = [1, 1]
        while len(leaves) < n:
            ok = [i for i, d in enumerate(leaves) if d < maxbits]
            i = max(ok, key=lambda j: leaves[j]) if rng.random() < 0.45 else ok[int(rng.integers(len(ok)))]
            leaves[i] += 1
            leaves.append(leaves[i])
        order = rng.permutation(n)
        return {symbols[int(j)]: leaves[i] for i, j in enumerate(order)}
    return code


def _fuzz_items(rng, produced, n):
    items = []
    alphabet = [int(x) for x in rng.integers(0, 256, int(rng.integers(1, 40)))]
    for _ in range(n):
        if produced == 0 or rng.random() < 0.5:
            items.append(alphabet[int(rng.integers(len(alphabet)))])
            produced += 1
            continue
        k = rng.random()
        far = min(produced, 32768)
        dist = 1 if k < 0.15 else int(rng.integers(1, min(far, 9) + 1)) if k < 0.45 else far if k < 0.5 else int(rng.integers(1, far + 1))
        k = rng.random()
        length = int(rng.integers(3, 11)) if k < 0.5 else 258 if k < 0.6 else int(rng.integers(3, 259))
        items.append((258, dist, 284) if length == 258 and rng.random() < 0.3 else (length, dist))
        produced += length
    return items, produced


def _fuzz_block(rng, produced):
    kind = int(rng.integers(0, 10))
    if kind < 2:
        data = R(int(rng.choice([0, 1, 2, 17, 300, 2000])), int(rng.integers(1 << 30)))
        return stored(data, pad_value=int(rng.integers(256))), produced + len(data)
    items, produced = _fuzz_items(rng, produced, int(rng.choice([0, 1, 3, 12, 60, 250])))
    if kind < 4:
        return fixed(items), produced
    ll, dd = used_symbols(items + [EOB])
    ll |= {int(x) for x in rng.integers(0, 286, int(rng.choice([0, 0, 3, 30, 200])))}
    if dd or rng.random() < 0.5:
        dd |= {int(x) for x in rng.integers(0, 30, int(rng.choice([0, 1, 4, 25])))}
    code = random_code(rng, int(rng.choice([15, 15, 15, 11, 9, 7])))
    if len(ll) > 128:
        code = random_code(rng, 15)
    lt, dt = code(sorted(ll)), (code(sorted(dd)) if dd else {})
    nl = int(rng.integers(max(257, max(ll) + 1), 287))
    nd = int(rng.integers(max(dd) + 1 if dd else 1, 31))
    return dynamic(table(nl, lt), table(nd, dt), items), produced


def fuzz(n, seed):
    """n seeded random descriptions, valid by construction -> [(name, description)]"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        blocks, produced = [], 0
        if i % 75 == 7:                                             # a few cross a pseudo-block cut
            for _ in range(2):
                blocks.append(stored(R(int(rng.integers(65300, 65536)), int(rng.integers(1 << 30)))))
            produced = sum(len(b["data"]) for b in blocks)
        for _ in range(int(rng.integers(1, 5))):
            b, produced = _fuzz_block(rng, produced)
            blocks.append(b)
        out.append(("fuzz-%03d" % i, blocks))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# damaged streams
# ---------------------------------------------------------------------------------------------------------------------
def cut_inside(blocks, mark, which=-1):
    """The stream of the blocks cut so that the deflate bytes end inside the marked field (the trailer's place then lies in the
    blocks): fixed blocks of one literal are put in front until a byte boundary falls inside the field."""
    for pre in range(8):
        for nine in range(pre + 1):
            lead = [fixed([200 if j < nine else 65], final=0) for j in range(pre)]
            d = {"blocks": lead + blocks}
            body, marks = deflate(d)
            _, s, e = [m for m in marks if m[0] == mark][which]
            cutbit = (e - 1) // 8 * 8
            if s <= cutbit < e:
                full = b"\x78\x9c" + body + zlib.adler32(expand(d)).to_bytes(4, "big")
                return full[:2 + cutbit // 8 + 4], len(expand(d))
    raise AssertionError("no cut inside " + mark)


def damaged():
    """[(name, the text of inflate_passes.h that must refuse it, stream, planned size, zlib refuses it, what the passes leave in
    its destination)] — one defect each.  The front end refuses all but the last four before a byte is written (the destination is
    left as it was: None); a wrong Adler-32 is found by pass 6, which sums the decoded bytes where pass 4 put them, in the
    destination: there the decoded bytes stay, and the stream is counted."""
    out = []
    nbits = "if (br.pos > nbits) return -1;"
    size_more = "if (e->outn >= e->dsize) return -1;"
    match_chk = "if (dist > e->outn || e->outn + len > e->dsize) return -1;"
    size_less = "if (afi_close(e, 1) || e->outn != e->dsize) return -1;"
    ll_chk = "if (r < 0 || (r > 0 && !(lcnt[1] == 1 && lcnt[0] == nl - 1))) return -1;"
    d_chk = "if (r < 0 || (r > 0 && !(dcnt[0] == nd || (dcnt[1] == 1 && dcnt[0] == nd - 1)))) return -1;"
    cl_chk = "if (afi_build(cl, 19, 7, cfast, dcnt, dsym)) return -1;"
    dcode = "if (ds < 0 || ds > 29) return -1;"
    sym_chk = "if (sy < 0 || br.pos > nbits) return -1;"
    past = "if (idx + rep > nl + nd) return -1;"

    def case(name, where, blocks, planned=None, means=b"", zlib_refuses=True, patch=None, **opts):
        d = dict(blocks=blocks, means=means)
        s = bytearray(build(d))
        if patch:
            patch(s)
        out.append((name, where, bytes(s), len(means) if planned is None else planned, zlib_refuses, opts.get("left")))

    def valid(name, where, blocks, delta):
        """A valid stream planned `delta` bytes off."""
        raw = expand(blocks)
        out.append((name, where, build(blocks), len(raw) + delta, False, None))

    pad = ("bits", 0, 32)
    # block and stored headers
    case("block-type-3", "if (type == 3) return -1;", [fixed(text("ab"), final=0), {"type": 3, "final": 1}], means=b"ab")
    case("len-is-not-the-complement-of-nlen", "len != (int64_t)((~v >> 16) & 0xffff)", [stored(b"hello", nlen=0x1234)], means=b"hello")
    case("len-one-bit-off-nlen", "len != (int64_t)((~v >> 16) & 0xffff)", [stored(b"hello", nlen=(~5 & 0xffff) ^ 0x8000)], means=b"hello")
    b = stored(b"short")
    b["len"] = 9                                                    # LEN reaches into the trailer: 5 data bytes and 4 of Adler-32
    case("stored-len-past-the-input", "br.pos + 8 * len > nbits", [b], planned=9, means=b"short")
    # header counts
    eight = {s: 8 for s in list(range(255)) + [256]}
    for nl in (287, 288):
        case("hlit-%d" % nl, "if (nl > 286 || nd > 30) return -1;", [dynamic(table(nl, eight), [0], [1, 2])], means=b"\x01\x02")
    for nd in (31, 32):
        case("hdist-%d" % nd, "if (nl > 286 || nd > 30) return -1;", [dynamic(table(257, eight), table(nd, {0: 1, nd - 1: 1}), [1, 2])], means=b"\x01\x02")
    case("hclen-4", "if (lens[256] == 0) return -1;", [dynamic([0] * 257, [0], [], hclen=4, cl_lengths={0: 1, 18: 1}, eob=False), fixed([pad], eob=False)], planned=1)
    # the code length code
    simple = table(257, balanced([1, 2, 256]))
    case("code-length-code-over-subscribed", cl_chk, [dynamic(simple, [0], [pad], cl_lengths={0: 1, 1: 1, 2: 1, 18: 2}, cl_syms=[], eob=False)], planned=1)
    case("code-length-code-incomplete", cl_chk, [dynamic(simple, [0], [pad], cl_lengths={0: 2, 1: 2, 2: 2}, cl_syms=[], eob=False)], planned=1)
    case("code-length-code-of-one-code", cl_chk, [dynamic(simple, [0], [pad], cl_lengths={0: 1}, cl_syms=[], eob=False)], planned=1)
    case("code-length-code-all-zero", cl_chk, [dynamic(simple, [0], [pad], cl_lengths={}, cl_syms=[], hclen=19, eob=False)], planned=1)
    # code length repeats
    rep = {0: 2, 1: 2, 2: 3, 16: 3, 17: 3, 18: 3}
    case("repeat-16-as-the-first-symbol", "if (!idx) return -1;", [dynamic(simple, [0], [pad], cl_lengths=rep, cl_syms=[(16, 0), 1], eob=False)], planned=1)
    over = [(18, 127), (18, 90)]                                   # 239 of 257 + 1 lengths
    case("repeat-16-past-the-counts", past, [dynamic(simple, [0], [pad], cl_lengths=rep, cl_syms=over + [1, 1] + [(16, 3)] * 3, eob=False)], planned=1)
    case("repeat-17-past-the-counts", past, [dynamic(simple, [0], [pad], cl_lengths=rep, cl_syms=over + [1, 1, 2] + [(17, 7), (17, 4)], eob=False)], planned=1)
    case("repeat-18-past-the-counts", past, [dynamic(simple, [0], [pad], cl_lengths=rep, cl_syms=over + [1, 1, 2, (18, 6)], eob=False)], planned=1)
    # literal/length tables
    case("no-end-of-block-code", "if (lens[256] == 0) return -1;", [dynamic(table(257, {0: 1, 1: 1}), [0], [0, 1], eob=False), fixed([pad], eob=False)], planned=2)
    case("litlen-over-subscribed", ll_chk, [dynamic(table(257, {0: 1, 1: 1, 256: 1}), [0], [], eob=False), fixed([pad], eob=False)], planned=1)
    case("litlen-incomplete-two-codes-of-2-bits", ll_chk, [dynamic(table(257, {0: 2, 256: 2}), [0], [0]), fixed([pad], eob=False)], planned=1, means=b"\0")
    case("litlen-incomplete-lone-code-of-2-bits", ll_chk, [dynamic(table(257, {256: 2}), [0], []), fixed([pad], eob=False)], planned=0)
    # distance tables
    lm = table(258, balanced([5, 256, 257]))
    case("distance-over-subscribed", d_chk, [dynamic(lm, [1, 1, 1], [5], eob=False), fixed([pad], eob=False)], planned=4)
    case("distance-lone-code-of-2-bits", d_chk, [dynamic(lm, [2], [5, (3, 1)]), fixed([pad], eob=False)], planned=4, means=b"\5\5\5\5")
    case("distance-incomplete-1-and-2-bits", d_chk, [dynamic(lm, [1, 2], [5, (3, 1)]), fixed([pad], eob=False)], planned=4, means=b"\5\5\5\5")
    # invalid symbols and codes
    case("symbol-286", "if (sy > 285) return -1;", [fixed([97, ("L", 286), ("D", 0)])], planned=4, means=b"aaaa")
    case("symbol-287", "if (sy > 285) return -1;", [fixed([97, ("L", 287), ("D", 0)])], planned=4, means=b"aaaa")
    case("distance-code-30", dcode, [fixed([97, ("L", 257), ("D", 30), ("bits", 0, 13)])], planned=4, means=b"aaaa")
    case("distance-code-31", dcode, [fixed([97, ("L", 257), ("D", 31), ("bits", 0, 13)])], planned=4, means=b"aaaa")
    case("one-code-distance-table-the-other-bit", dcode, [dynamic(lm, [1], [5, ("L", 257), ("bits", 1, 1)])], planned=4, means=b"\5\5\5\5")
    case("match-with-no-distance-code", dcode, [dynamic(lm, [0], [5, ("L", 257), ("bits", 0, 1)])], planned=4, means=b"\5\5\5\5")
    case("match-with-no-distance-code-bit-1", dcode, [dynamic(lm, [0], [5, ("L", 257), ("bits", 1, 1)])], planned=4, means=b"\5\5\5\5")
    # distances before the start
    case("distance-1-at-the-first-byte", match_chk, [fixed([(3, 1), 7])], planned=4, means=b"\7\7\7\7")
    case("distance-one-before-its-start", match_chk, [fixed(text("abcde") + [(3, 6)])], planned=8, means=b"abcdeabc")
    case("distance-one-before-its-start-after-stored", match_chk, [stored(b"0123456"), fixed([8, (200, 9)])], planned=208, means=b"0" * 208)
    # the planned size is another: valid streams
    valid("one-byte-more-than-planned-by-a-literal", size_more, [fixed(text("abc") + [(3, 2), 9])], -1)
    valid("one-byte-more-than-planned-by-a-match", match_chk, [fixed(text("abc") + [9, (3, 2)])], -1)
    valid("one-byte-more-than-planned-by-a-stored-block", size_more, [fixed(text("abc")), stored(b"xyz")], -1)
    valid("one-byte-fewer-than-planned-by-a-literal", size_less, [fixed(text("abc") + [(3, 2), 9])], 1)
    valid("one-byte-fewer-than-planned-by-a-match", size_less, [fixed(text("abc") + [9, (3, 2)])], 1)
    valid("one-byte-fewer-than-planned-by-a-stored-block", size_less, [fixed(text("abc")), stored(b"xyz")], 1)
    # the input ends too soon
    hdr3 = "const uint32_t h = afi_take(&br, 3);\n        if (br.pos > nbits) return -1;"
    dynb = lambda: dynamic(table(266, {97: 1, 256: 2, 259: 3, 265: 3}), [2, 2, 2, 3, 3], [97, 97, 97, (5, 2), (12, 5), 97])          # noqa: E731
    cl_end = "cl[afi_cl_order[i]] = (uint8_t)afi_take(&br, 3);\n            if (br.pos > nbits) return -1;"
    for name, where, blocks, mark in (
            ("a-block-header", hdr3, [fixed(text("ab"), final=0), fixed(text("cd"))], "block_header"),
            ("a-stored-header", "br.pos > nbits || len != (int64_t)((~v >> 16) & 0xffff)", [fixed(text("ab"), final=0), stored(b"cdef")], "stored_header"),
            ("hlit", cl_end, [dynb()], "hlit"), ("hdist", cl_end, [dynb()], "hdist"), ("hclen", cl_end, [dynb()], "hclen"),
            ("the-code-length-code-lengths", cl_end, [dynb()], "cl_lengths"), ("the-code-lengths", nbits, [dynb()], "code_lengths"),
            ("a-symbol", sym_chk, [dynb()], "len_sym"), ("the-length-extra-bits", "if (br.pos > nbits || afi_match(e, len, dist)) return -1;", [dynb()], "len_extra"),
            ("a-distance-symbol", "if (br.pos > nbits || afi_match(e, len, dist)) return -1;", [dynb()], "dist_sym"),
            ("the-distance-extra-bits", "if (br.pos > nbits || afi_match(e, len, dist)) return -1;", [fixed(text("abcdefghijkl") + [(9, 12)])], "dist_extra"),
            ("the-end-of-block", sym_chk, [dynb()], "eob")):
        s, n = cut_inside(blocks, mark)
        out.append(("input-ends-inside-" + name, where, s, n, True, None))
    case("no-final-block", hdr3, [fixed(text("ab"), final=0), fixed(text("ef"), final=0), stored(b"cd", final=0)], means=b"abefcd")
    good = next(g for g in (build([fixed(text("the end-of-block code ends on the last bit of its byte") + [(9, 4)] + [200] * j)]) for j in range(8))
                if ("eob_bit", 0) in strict_decode(g)[1])
    for k in range(1, 5):
        out.append(("end-of-block-in-the-trailer-cut-by-%d" % k, sym_chk, good[:-k], len(zlib.decompress(good)), True, None))
    raw = text("Adler-32 of these bytes")
    for k in range(4):
        case("adler-byte-%d-one-bit" % k, "if ((uint32_t)((B << 16) | A) != c->want[s]) afi_mark_bad(c, s);", [fixed(raw + [(7, 5)])], means=expand([fixed(raw + [(7, 5)])]), left=expand([fixed(raw + [(7, 5)])]),
             patch=lambda s, k=k: s.__setitem__(len(s) - 4 + k, s[len(s) - 4 + k] ^ (1 << (2 * k + 1))))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# one batch
# ---------------------------------------------------------------------------------------------------------------------
GAP, FILL = 40, 0xAB


def layout(streams, sizes, gap=GAP):
    """Streams back to back — the first starts at byte 0 of the compressed buffer, the last ends on its last byte, nothing is
    padded, so odd start addresses occur — and destinations between canaries of `gap` bytes
    -> (base, comp_off, comp_size, out_off, out bytes)."""
    cs = np.array([len(s) for s in streams], dtype=np.int64)
    co = np.concatenate([[0], np.cumsum(cs)[:-1]]).astype(np.int64)
    base = np.frombuffer(b"".join(streams), dtype=np.uint8).copy()
    sizes = np.asarray(sizes, dtype=np.int64)
    oo = (gap + np.concatenate([[0], np.cumsum(sizes + gap)[:-1]])).astype(np.int64)
    return base, co, cs, oo, int(gap + (sizes + gap).sum())


def restore(raw, blocks_of=60000):
    """The bytes written again by the writer as stored plus fixed blocks (for shuffled copies of catalogue streams)."""
    blocks = []
    for p in range(0, len(raw), blocks_of):
        part = raw[p:p + blocks_of]
        blocks += [stored(part[:-40]), fixed(list(part[-40:]))]
    return blocks or [fixed([])]


# ---------------------------------------------------------------------------------------------------------------------
# the file of tests/deflate_streams_check.c
# ---------------------------------------------------------------------------------------------------------------------
def mutated(streams, n, seed):
    """n copies of small streams with one to three bytes or bits changed, or cut short, the two header bytes left alone
    -> [(stream, the size its source decodes to)]"""
    rng = np.random.default_rng(seed)
    small = [(s, size) for s, size in streams if 8 < len(s) < 20000 and size < 100000]
    out = []
    for it in range(n):
        s, size = small[int(rng.integers(len(small)))]
        b = bytearray(s)
        if it % 5 == 0:
            b = b[:int(rng.integers(3, len(b)))]
        else:
            for _ in range(int(rng.integers(1, 4))):
                j = int(rng.integers(2, len(b))) if it % 5 < 3 else int(rng.integers(2, min(len(b), 40)))
                b[j] = int(rng.integers(256)) if it % 2 else b[j] ^ (1 << int(rng.integers(8)))
        out.append((bytes(b), size))
    return out


def valid_streams():
    """[(name, stream, decoded bytes)] of the catalogue and the fuzz."""
    return [(name, build(d), expand(d)) for name, d in [(n, d) for n, _, d in catalogue()] + fuzz(FUZZ_COUNT, FUZZ_SEED)]


def write_check_file(path, valid=None):
    """u32 n, then per stream u32 kind (0 valid, 1 damaged, 2 mutated, 3 valid but planned another size), u32 stream bytes, u32
    planned size, the stream, and for kind 0 the decoded bytes."""
    valid = valid or valid_streams()
    recs = [(0, s, len(raw), raw) for _, s, raw in valid]
    recs += [(1 if refused else 3, s, n, b"") for _, _, s, n, refused, _ in damaged()]
    recs += [(2, s, n, b"") for s, n in mutated([(s, len(r)) for _, s, r in valid], MUTATED_COUNT, 4)]
    with open(path, "wb") as f:
        f.write(len(recs).to_bytes(4, "little"))
        for kind, s, n, want in recs:
            f.write(kind.to_bytes(4, "little") + len(s).to_bytes(4, "little") + n.to_bytes(4, "little") + s + want)
    return len(recs)


if __name__ == "__main__":
    import sys
    print("deflate_streams: wrote", write_check_file(sys.argv[1]), "streams to", sys.argv[1])
