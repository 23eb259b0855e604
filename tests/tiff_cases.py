"""An independent TIFF writer and the catalogues the TIFF tests share: files (strips and tiles, II / MM, classic / BigTIFF, the three
compressions, the three predictors, geo tags, nodata, overview and mask pages), hand-built LZW streams, damaged streams and one file per
refusal of `aggfly_amd/tiff.py`.  Nothing here imports the package: the LZW encoder is Python (libtiff's early change, Clear when the
table holds 4,094 entries, EndOfInformation optional), Deflate is the standard library's zlib, the predictors are numpy.

Run as a program it writes the stream catalogue and 2,000 byte- and bit-mutated streams into one file for tests/lzw_streams_check.c:
    python3 tests/tiff_cases.py OUT.bin
    record = int32 kind (0 good, 1 damaged, 2 mutated: whatever it does, it must stay in bounds) | int32 stream bytes | int32 decoded bytes |
             stream | expected bytes (kind 0 only)
"""
from __future__ import annotations

import os
import struct
import sys
import zlib

import numpy as np

CLEAR, EOI, FIRST = 256, 257, 258


# ---- LZW ----
class BitWriter:
    def __init__(self):
        self.acc, self.nb, self.out = 0, 0, bytearray()

    def put(self, code, width):
        self.acc = (self.acc << width) | code
        self.nb += width
        while self.nb >= 8:
            self.nb -= 8
            self.out.append((self.acc >> self.nb) & 255)
        self.acc &= (1 << self.nb) - 1

    def done(self) -> bytes:
        if self.nb:
            self.out.append((self.acc << (8 - self.nb)) & 255)
            self.acc = self.nb = 0
        return bytes(self.out)


def pack_codes(codes) -> bytes:
    """[(code, width), ...] most significant bit first."""
    w = BitWriter()
    for c, n in codes:
        w.put(c, n)
    return w.done()


def lzw_encode(data: bytes, eoi: bool = True, count_codes: list | None = None) -> bytes:
    """TIFF LZW as libtiff's encoder writes it: a Clear first, codes of 9..12 bits, the width grown as soon as the next free code exceeds
    2^width - 1 on the encoder's side (one code early for the decoder), a Clear and a new table once code 4093 has been given out."""
    w, width, nxt, table, n_codes = BitWriter(), 9, FIRST, {}, 0
    w.put(CLEAR, width)
    data = bytes(data)
    if data:
        cur = data[0]
        for c in data[1:]:
            key = (cur << 8) | c
            got = table.get(key)
            if got is not None:
                cur = got
                continue
            w.put(cur, width)
            n_codes += 1
            table[key] = nxt
            nxt += 1
            if nxt == 4094:
                w.put(CLEAR, width)
                table, nxt, width = {}, FIRST, 9
            elif nxt > (1 << width) - 1:
                width += 1
            cur = c
        w.put(cur, width)
        n_codes += 1
        nxt += 1
        if nxt == 4094:
            w.put(CLEAR, width)
            width = 9
        elif nxt > (1 << width) - 1:
            width += 1
    if eoi:
        w.put(EOI, width)
    if count_codes is not None:
        count_codes.append(n_codes)
    return w.done()


def prefix_with_codes(data: bytes, n_codes: int) -> bytes:
    """The longest prefix of ``data`` whose stream holds ``n_codes`` data codes (the count grows by at most one per byte)."""
    lo, hi = 1, len(data)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        cnt = []
        lzw_encode(data[:mid], count_codes=cnt)
        if cnt[0] <= n_codes:
            lo = mid
        else:
            hi = mid - 1
    cnt = []
    lzw_encode(data[:lo], count_codes=cnt)
    assert cnt[0] == n_codes, (cnt, n_codes)
    return data[:lo]


def stream_catalogue():
    """[(name, stream, decoded bytes, expected or None)]: None marks a damaged stream, which the decoder must refuse."""
    rng = np.random.default_rng(20261021)
    rnd = rng.integers(0, 256, 16384, dtype=np.uint8).tobytes()
    smooth = (np.cumsum(rng.integers(-2, 3, 6000)) & 255).astype(np.uint8).tobytes()
    good = [("one byte", b"\x5a"), ("run of 70000", b"\x07" * 70000), ("random 16 KiB", rnd), ("smooth 6000", smooth),
            ("two values", bytes([1, 2]) * 3000), ("abab", b"ab" * 700 + b"abc" * 500), ("all bytes", bytes(range(256)) * 3)]
    out = [(name, lzw_encode(d), len(d), d) for name, d in good]
    # streams that cross each width switch exactly: the decoder's next free code reaches 511 / 1023 / 2047 while it reads data code
    # number 254 / 766 / 1790 (the first code after a Clear makes no entry); one code fewer, that many, one more
    for switch in (511, 1023, 2047):
        for delta in (-1, 0, 1):
            d = prefix_with_codes(rnd, switch - FIRST + 1 + delta)
            out.append((f"switch {switch}{delta:+d}", lzw_encode(d), len(d), d))
            out.append((f"switch {switch}{delta:+d} no EOI", lzw_encode(d, eoi=False), len(d), d))
    # a stream that stops at the segment size without EndOfInformation, and one whose EndOfInformation is followed by junk
    out.append(("no EOI", lzw_encode(smooth, eoi=False), len(smooth), smooth))
    out.append(("junk after EOI", lzw_encode(smooth) + b"\xff\x00\xff", len(smooth), smooth))
    # a stream without the leading Clear (the specification asks for one; old writers leave it out)
    out.append(("no leading Clear", pack_codes([(65, 9), (66, 9), (258, 9), (EOI, 9)]), 4, b"ABAB"))
    # KwKwK by hand: A, then 258 before it is complete = AA, then 259 likewise = AAA
    out.append(("KwKwK", pack_codes([(CLEAR, 9), (65, 9), (258, 9), (259, 9), (EOI, 9)]), 6, b"A" * 6))
    # ---- damaged: each beside the line of lzw_passes.h that refuses it ----
    out.append(("L1 code above the next free one", pack_codes([(CLEAR, 9), (65, 9), (300, 9), (EOI, 9)]), 4, None))
    out.append(("L1 code one above the next free one", pack_codes([(CLEAR, 9), (65, 9), (66, 9), (260, 9), (EOI, 9)]), 6, None))
    out.append(("L2 no literal after Clear", pack_codes([(CLEAR, 9), (258, 9), (EOI, 9)]), 2, None))
    out.append(("L2 no literal after the second Clear", pack_codes([(CLEAR, 9), (65, 9), (66, 9), (CLEAR, 9), (258, 9), (EOI, 9)]), 4, None))
    out.append(("L3 span beyond the decoded size", pack_codes([(CLEAR, 9), (65, 9), (258, 9), (EOI, 9)]), 2, None))
    full = lzw_encode(rnd)
    out.append(("L4 cut short", full[:len(full) // 2], len(rnd), None))
    out.append(("L4 empty stream", b"", 5, None))
    out.append(("L5 EndOfInformation before the decoded size", lzw_encode(smooth), len(smooth) + 1, None))
    return out


# ---- predictors (forward) ----
def apply_predictor(a: np.ndarray, predictor: int, byteorder: str) -> bytes:
    """(rows, pitch) native samples -> the bytes a writer hands to the compressor."""
    rows, pitch = a.shape
    E = a.dtype.itemsize
    if predictor == 3:
        b = np.ascontiguousarray(a.astype(a.dtype.newbyteorder(">"))).view(np.uint8).reshape(rows, pitch, E)
        planes = np.ascontiguousarray(b.transpose(0, 2, 1)).reshape(rows, E * pitch)
        d = planes.copy()
        d[:, 1:] = planes[:, 1:] - planes[:, :-1]
        return d.tobytes()
    if predictor == 2:
        u = a.view(np.dtype(f"u{E}"))
        d = u.copy()
        d[:, 1:] = u[:, 1:] - u[:, :-1]
        a = d
    return np.ascontiguousarray(a.astype(a.dtype.newbyteorder(byteorder))).tobytes()


def compress(raw: bytes, compression: int, eoi: bool = True) -> bytes:
    if compression == 5:
        return lzw_encode(raw, eoi=eoi)
    if compression in (8, 32946):
        return zlib.compress(raw, 6)
    return raw


# ---- the container ----
_TYPE_FMT = {1: "B", 2: "s", 3: "H", 4: "I", 11: "f", 12: "d", 16: "Q"}


def geo_tags(lon0=-100.0, lat0=50.0, dx=0.25, dy=0.25, point=False, transformation=False, model=2, rot=0.0):
    """The tags of a geographic grid whose upper-left corner (or first grid point, ``point``) is (lon0, lat0)."""
    keys = [1, 1, 0, 2, 1024, 0, 1, model, 1025, 0, 1, 2 if point else 1]
    tags = {34735: (3, keys)}
    if transformation:
        tags[34264] = (12, [dx, rot, 0, lon0, rot, -dy, 0, lat0, 0, 0, 0, 0, 0, 0, 0, 1])
    else:
        tags[33550] = (12, [dx, dy, 0.0])
        tags[33922] = (12, [0.0, 0.0, 0.0, lon0, lat0, 0.0])
    return tags


def expected_coords(width, height, lon0=-100.0, lat0=50.0, dx=0.25, dy=0.25, point=False):
    half = 0.0 if point else 0.5
    return lon0 + (np.arange(width) + half) * dx, lat0 - (np.arange(height) + half) * dy


def page(array, compression=1, predictor=1, tile=None, rows_per_strip=None, nodata=None, subfile=0, geo=True, eoi=True, tags=None,
         junk_seed=7):
    """One page for `write_tiff`: ``tile`` = (width, length) or None for strips; ``geo``: True (the default grid), False, or a dict
    of tags; ``tags``: {tag: (type, values) or None} that replace or remove what the writer would write (the refusal files)."""
    return dict(array=np.ascontiguousarray(array), compression=compression, predictor=predictor, tile=tile, rows_per_strip=rows_per_strip,
                nodata=nodata, subfile=subfile, geo=geo, eoi=eoi, tags=dict(tags or {}), junk_seed=junk_seed)


def write_tiff(path, pages, byteorder="<", bigtiff=False):
    bo = byteorder
    buf = bytearray()
    if bigtiff:
        buf += (b"II" if bo == "<" else b"MM") + struct.pack(bo + "HHHQ", 43, 8, 0, 0)
        ptr_at, ow, of, cf, otype = 8, 8, "Q", "Q", 16
    else:
        buf += (b"II" if bo == "<" else b"MM") + struct.pack(bo + "HI", 42, 0)
        ptr_at, ow, of, cf, otype = 4, 4, "I", "H", 4

    def align():
        while len(buf) % 8:
            buf.append(0)

    for pg in pages:
        a = pg["array"]
        H, W = a.shape
        E = a.dtype.itemsize
        fmt = {"u": 1, "i": 2, "f": 3}[a.dtype.kind]
        segs = []
        if pg["tile"]:
            tw, th = pg["tile"]
            rng = np.random.default_rng(pg["junk_seed"])
            PH, PW = -(-H // th) * th, -(-W // tw) * tw
            padded = rng.integers(0, 256, PH * PW * E, dtype=np.uint8).view(a.dtype).reshape(PH, PW).copy()      # junk in the padding
            if a.dtype.kind == "f":
                padded = np.nan_to_num(padded, nan=1.5, posinf=2.5, neginf=-2.5)
            padded[:H, :W] = a
            for y in range(0, PH, th):
                for x in range(0, PW, tw):
                    segs.append(padded[y:y + th, x:x + tw])
        else:
            rps = pg["rows_per_strip"] or H
            for y in range(0, H, rps):
                segs.append(a[y:y + rps])
        offsets, counts = [], []
        for s in segs:
            data = compress(apply_predictor(np.ascontiguousarray(s), pg["predictor"], bo), pg["compression"], pg["eoi"])
            align()
            offsets.append(len(buf))
            counts.append(len(data))
            buf += data
        tags = {254: (4, [pg["subfile"]]), 256: (4, [W]), 257: (4, [H]), 258: (3, [8 * E]), 259: (3, [pg["compression"]]), 262: (3, [1]),
                277: (3, [1]), 284: (3, [1]), 339: (3, [fmt])}
        if pg["predictor"] != 1:
            tags[317] = (3, [pg["predictor"]])
        if pg["tile"]:
            tags.update({322: (4, [pg["tile"][0]]), 323: (4, [pg["tile"][1]]), 324: (otype, offsets), 325: (4, counts)})
        else:
            tags.update({278: (4, [pg["rows_per_strip"] or H]), 273: (otype, offsets), 279: (4, counts)})
        if pg["geo"] is True:
            tags.update(geo_tags())
        elif pg["geo"]:
            tags.update(pg["geo"])
        if pg["nodata"] is not None:
            tags[42113] = (2, str(pg["nodata"]).encode() + b"\0")
        for t, v in pg["tags"].items():
            if v is None:
                tags.pop(t, None)
            else:
                tags[t] = v
        entries = bytearray()
        for t in sorted(tags):
            typ, vals = tags[t]
            if typ == 2:
                raw, count = bytes(vals), len(vals)
            else:
                raw, count = struct.pack(bo + str(len(vals)) + _TYPE_FMT[typ], *vals), len(vals)
            if len(raw) <= ow:
                field = raw + b"\0" * (ow - len(raw))
            else:
                align()
                field = struct.pack(bo + of, len(buf))
                buf += raw
            entries += struct.pack(bo + "HH" + of, t, typ, count) + field
        align()
        struct.pack_into(bo + of, buf, ptr_at, len(buf))            # the previous directory (or the header) points here
        buf += struct.pack(bo + cf, len(tags)) + entries
        ptr_at = len(buf)
        buf += struct.pack(bo + of, 0)
    with open(path, "wb") as f:
        f.write(buf)
    return path


# ---- the file catalogue ----
H0, W0 = 37, 70                      # 16 x 16 tiles: the right and the bottom tiles are partial; 5 rows per strip: the last strip has 2


def field(dtype, n_pages, height=H0, width=W0, seed=0, nodata=None):
    """(n_pages, height, width) of ``dtype``: smooth in space (so the predictors and LZW have something to do), every page different,
    the integers spanning their whole range (so the running sums wrap), some cells at ``nodata``."""
    rng = np.random.default_rng(1000 + seed)
    dtype = np.dtype(dtype)
    y, x = np.mgrid[0:height, 0:width]
    base = np.stack([np.sin(x / 7.0 + t) * 40 + np.cos(y / 5.0 - t) * 25 + t for t in range(n_pages)])
    if dtype.kind == "f":
        a = (base + rng.normal(0, 0.01, base.shape)).astype(dtype)
        a[:, 0, 0] = np.array([0.0, -0.0, 1e-30, 3e38, -3e38, 1.0, 2.0][:n_pages], dtype=dtype)
    else:
        info = np.iinfo(dtype)
        span = float(info.max) - float(info.min)
        a = (np.floor((base + 80) / 160 * span * 0.999) + float(info.min)).astype(np.float64)
        a = np.clip(a, info.min, info.max).astype(dtype)
        a[:, 0, 0], a[:, -1, -1] = info.max, info.min
    if nodata is not None:
        a[rng.random(a.shape) < 0.05] = nodata
    return a


def file_catalogue():
    """[dict(name, files=[(file name, [page, ...], byteorder, bigtiff)], values (T, H, W) stored type, nodata, times or None, tiff_time)]:
    what the tests write into a directory (`write_case`) and what `TiffStack.read_raw` must give back bit for bit."""
    cases = []

    def add(name, a, files, nodata=None, tiff_time=None, height=H0, width=W0):
        cases.append(dict(name=name, values=a, files=files, nodata=nodata, tiff_time=tiff_time, height=height, width=width))

    def daily(a, **kw):
        return [(f"v_{20200101 + t}.tif", [page(a[t], **kw)], "<", False) for t in range(len(a))]

    # strips and tiles x the three compressions x the predictor of the type, as daily files
    k = 0
    for dt, pred in (("f4", 3), ("f8", 3), ("u1", 2), ("i1", 2), ("u2", 2), ("i2", 2), ("u4", 2), ("i4", 2), ("u8", 2), ("i8", 2)):
        for comp in (1, 5, 8):
            for tile in (None, (16, 16)):
                k += 1
                if (k % 3) and dt not in ("f4", "u2"):                                  # every layout for f4 and u2, a third of them for the rest
                    continue
                a = field(dt, 3, seed=k)
                p = 1 if comp == 1 else pred                                            # (the predictor belongs to the LZW and Deflate codecs)
                add(f"{dt} comp{comp} pred{p} {'tiles' if tile else 'strips'}", a,
                    daily(a, compression=comp, predictor=p, tile=tile, rows_per_strip=None if tile else 5))
    # without a predictor, big-endian, BigTIFF, multi-page
    for dt, pred in (("f4", 1), ("f4", 3), ("u2", 2), ("i4", 2), ("f8", 3), ("u8", 1)):
        for bo, big in (("<", True), (">", False), (">", True)):
            k += 1
            a = field(dt, 4, seed=k)
            tile = (16, 16) if k % 2 else None
            add(f"{dt} pred{pred} {'MM' if bo == '>' else 'II'} {'BigTIFF' if big else 'classic'} multi-page {'tiles' if tile else 'strips'}", a,
                [("stack.tif", [page(a[t], compression=5 if k % 3 else 8, predictor=pred, tile=tile, rows_per_strip=None if tile else 5)
                                for t in range(4)], bo, big)],
                tiff_time=list(np.datetime64("2020-03-01") + np.arange(4)))
    # the scan's carry: row widths of 1, 63, 64, 65, 129 and 257 samples, strips (pitch = width) and one tile wider than the image
    for width in (1, 63, 64, 65, 129, 257):
        for dt, pred in (("u2", 2), ("f4", 3), ("u8", 2)):
            k += 1
            a = field(dt, 3, height=6, width=width, seed=k)
            add(f"{dt} pred{pred} width {width}", a, daily(a, compression=5, predictor=pred, rows_per_strip=4), height=6, width=width)
    a = field("f4", 3, height=6, width=65, seed=k + 1)
    add("f4 pred3 width 65 in tiles of 80", a, daily(a, compression=8, predictor=3, tile=(80, 16)), height=6, width=65)
    # nodata: floats (NaN on read) and integers (floats with NaN on read); an LZW file without EndOfInformation; 7 pages
    a = field("f4", 7, seed=90, nodata=-9999.0)
    add("f4 nodata -9999 seven days", a, daily(a, compression=5, predictor=3, tile=(16, 16), nodata="-9999"), nodata=-9999.0)
    a = field("i2", 5, seed=91, nodata=-32768)
    add("i2 nodata -32768", a, daily(a, compression=8, predictor=2, rows_per_strip=5, nodata="-32768"), nodata=-32768)
    a = field("u1", 3, seed=92, nodata=255)
    add("u1 nodata 255", a, daily(a, compression=5, predictor=2, tile=(16, 16), nodata="255"), nodata=255)
    a = field("u2", 3, seed=93, nodata=65535)
    add("u2 nodata 65535 no EOI", a, daily(a, compression=5, predictor=2, rows_per_strip=5, nodata="65535", eoi=False), nodata=65535)
    # a cloud-optimised layout: the full-resolution page, then overviews and a mask, which are skipped
    a = field("f4", 3, seed=94)
    files = []
    for t in range(3):
        over = page(a[t][::2, ::2], compression=5, predictor=3, tile=(16, 16), subfile=1, geo=False)
        mask = page((a[t] > 0).astype(np.uint8), compression=8, tile=(16, 16), subfile=4, geo=False)
        files.append((f"cog_{2021 + t}.tif", [page(a[t], compression=5, predictor=3, tile=(16, 16)), over, mask], "<", False))
    add("overviews and masks skipped", a, files)
    return cases


def write_case(case, directory):
    """Writes the files of a catalogue case -> their paths, in time order."""
    os.makedirs(directory, exist_ok=True)
    return [write_tiff(os.path.join(directory, fn), pages, bo, big) for fn, pages, bo, big in case["files"]]


def refusal_catalogue():
    """[(name, [pages], byteorder, word the reason must hold)]: one file per item of `tiff.py`'s refusal list."""
    a = field("u2", 1)[0]
    f = field("f4", 1)[0]
    out = []
    for code, word in ((7, "JPEG"), (32773, "PackBits"), (50000, "ZSTD"), (34887, "LERC"), (50001, "WebP"), (34925, "LZMA"), (60000, "unknown")):
        out.append((f"compression {code}", [page(a, tags={259: (3, [code])})], "<", word))
    old = page(a, compression=5, rows_per_strip=H0)
    out.append(("old-style LZW", [old], "<", "old-style LZW"))                           # (its stream is patched below: `write_refusal`)
    out.append(("FillOrder 2", [page(a, tags={266: (3, [2])})], "<", "FillOrder"))
    out.append(("12 bits", [page(a, tags={258: (3, [12])})], "<", "bits per sample"))
    out.append(("1 bit", [page(a, tags={258: None})], "<", "bits per sample"))
    out.append(("float16", [page(a, tags={339: (3, [3])})], "<", "16 bits"))
    out.append(("predictor 2 on floats", [page(f, tags={317: (3, [2])})], "<", "predictor 2"))
    out.append(("predictor 3 on integers", [page(a, tags={317: (3, [3])})], "<", "predictor 3"))
    out.append(("three samples chunky", [page(a, tags={277: (3, [3]), 258: (3, [16, 16, 16])})], "<", "SamplesPerPixel"))
    out.append(("three samples planar", [page(a, tags={277: (3, [3]), 284: (3, [2]), 258: (3, [16, 16, 16])})], "<", "SamplesPerPixel"))
    out.append(("complex samples", [page(f, tags={339: (3, [6])})], "<", "complex"))
    out.append(("projected CRS", [page(a, geo=geo_tags(model=1))], "<", "projected"))
    out.append(("rotated transformation", [page(a, geo=geo_tags(transformation=True, rot=0.01))], "<", "rotated"))
    out.append(("no georeferencing", [page(a, geo=False)], "<", "georeferencing"))
    out.append(("pages differ in grid", [page(a), page(a, geo=geo_tags(lon0=-90.0))], "<", "differs"))
    out.append(("pages differ in type", [page(a), page(a.astype("i2"))], "<", "differs"))
    out.append(("pages differ in nodata", [page(a, nodata="0"), page(a, nodata="1")], "<", "differs"))
    out.append(("pages differ in size", [page(a), page(a[:, :60])], "<", "differs"))
    out.append(("offset leaves the file", [page(a, tags={273: (4, [1 << 30])})], "<", "leaves the file"))
    out.append(("byte count leaves the file", [page(a, tags={279: (4, [1 << 30])})], "<", "leaves the file"))
    return out


def write_refusal(item, directory):
    name, pages, bo, word = item
    os.makedirs(directory, exist_ok=True)
    path = write_tiff(os.path.join(directory, name.replace(" ", "_") + "_20200101.tif"), pages, bo)
    if name == "old-style LZW":
        # what TIFF 5.0 writers left: codes least significant bit first, so a stream begins with the Clear code as 00 01
        with open(path, "r+b") as fh:
            fh.seek(8)
            fh.write(b"\x00\x01")
    return path


# ---- the streams for the sanitizer program ----
def mutated_streams(count=2000, seed=5):
    rng = np.random.default_rng(seed)
    base = [(s, n) for _, s, n, exp in stream_catalogue() if len(s) > 0 and n <= 20000]
    out = []
    for i in range(count):
        s, n = base[int(rng.integers(len(base)))]
        b = bytearray(s)
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(len(b)))
            if rng.random() < 0.5:
                b[at] ^= 1 << int(rng.integers(8))
            else:
                b[at] = int(rng.integers(256))
        how = rng.random()
        if how < 0.15:
            b = b[:int(rng.integers(len(b) + 1))]
        elif how < 0.25:
            b += bytes(rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8))
        out.append((bytes(b), max(0, n + int(rng.integers(-3, 4)))))
    return out


def main(argv):
    with open(argv[1], "wb") as f:
        n = 0
        for _, s, size, exp in stream_catalogue():
            f.write(struct.pack("<iii", 0 if exp is not None else 1, len(s), size) + s + (exp if exp is not None else b""))
            n += 1
        for s, size in mutated_streams():
            f.write(struct.pack("<iii", 2, len(s), size) + s)
            n += 1
    print(f"{n} streams -> {argv[1]}")


if __name__ == "__main__":
    main(sys.argv)
