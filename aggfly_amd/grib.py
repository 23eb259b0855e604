"""Index and host decode of GRIB files (editions 1 and 2, regular latitude / longitude grids; simple packing, and in edition 2 complex
packing with and without spatial differencing, data representation templates 5.2 and 5.3, and CCSDS packing, template 5.42), written from the format's octet tables (WMO Manual on Codes, FM 92 GRIB; edition 1 as in the ECMWF / NCEP descriptions of its sections).  `GribFile`
walks the file message by message and reads the section HEADERS only: it tells where the packed bits and the bitmap of every field
lie and how they unpack; `io._GribSource.to_device` `pread`s those bytes into page-locked memory and kernels (`hip.grib_unpack`,
`hip.grib_unpack_complex`, `hip.grib_unpack_ccsds`) extract, scale and place them in the cube in HBM.  `GribFile.read` is the same decode in numpy: the ``device=None`` route.

    edition 1   0 indicator (8)  1 product definition  2 grid description  [3 bitmap]  4 binary data  5 '7777'
    edition 2   0 indicator (16) 1 identification [2 local use] 3 grid definition 4 product definition
                5 data representation 6 bitmap 7 data 8 '7777'

Simple packing: a field is a big-endian bit stream of ``nbits``-bit unsigned integers X (nbits 0..32), and the value is
``(X * 2**E + R) * 10**-D``, computed here — and in the kernel — as ``((X * s) + R) * d`` in float64 with ``s = 2.0 ** E`` and
``d = 10.0 ** -D`` and rounded to float32.  A bitmap, one bit per grid point in scan order, marks the points that have a value; the
others are NaN.

Complex packing (5.2 / 5.3; what NCEP writes, and `wgrib2 -set_grib_type c3`): the N values are cut into NG groups, and section 7 is one
bit stream, most significant bit first: [5.3: ``order`` first values ival1 [, ival2] and the smallest difference minsd, ``extra`` octets
each, sign-magnitude;] NG group references of ``nbits_ref`` bits; NG widths of ``nbits_width`` bits (``width = ref_width + stored``); NG
scaled lengths of ``nbits_len`` bits (``len = ref_len + len_inc * stored``, the last group's length is ``last_len`` whatever was stored)
- each table padded with zero bits to an octet boundary, a table of 0 bits absent and all 0 -; then group after group ``len[g]``
fields of ``width[g]`` bits, ``raw[n] = ref[g] + field``.  5.2: ``X = raw``.  Order 1: ``X[0] = ival1``, ``X[n] = X[n-1] + raw[n] +
minsd``.  Order 2: ``X[0] = ival1``, ``X[1] = ival2``, ``X[n] = raw[n] + minsd + 2 X[n-1] - X[n-2]`` (``raw[0]``, ``raw[1]`` are
placeholders).  As plain running sums: ``g[0] = 0``, ``g[1] = ival2 - ival1`` (order 2) and ``g[n] = raw[n] + minsd`` otherwise; ``X =
ival1 + cumsum(g)`` for order 1, ``ival1 + cumsum(cumsum(g))`` for order 2 - in int64, wrapping, here and in the kernels.  The value is
the same ``((X * s) + R) * d`` with X a signed int64, exact while ``|X| < 2**53``.  With NG = 0 every X is 0.

CCSDS packing (5.42; what ECMWF writes for grid-point fields since IFS cycle 48r1): section 5 is 25 octets - R, E, D, nbits as in 5.0,
octet 22 the flags, octet 23 the block size J, octets 24-25 the reference sample interval ``rsi`` - and section 7 is one CCSDS 121.0-B
adaptive-entropy-coded stream of ``n_values`` unsigned ``nbits``-bit samples X as libaec writes it (``aggfly_amd/csrc/aec_passes.h`` has
the blocks, the preprocessor and the passes that decode them; `codec.aec_decode` runs those on the host, `hip.grib_unpack_ccsds` in HBM).
Flags 2 and 4 say how samples lie in memory and are ignored, flag 8 (the preprocessor) is honoured either way, flags 1 (signed), 16
(restricted IDs), 32 (RSIs padded to bytes), 64 and 128 are refused; so are J outside 8 / 16 / 32 / 64 and rsi outside 1..4096.  With
nbits 0 the field is constant and section 7 is empty.  The value is the same ``((X * s) + R) * d``.

Everything else is refused with a ValueError that names it: other grids (Gaussian, reduced, rotated), other packings (edition 1's
second-order packing, complex packing with missing value management 1 / 2, a spatial differencing order outside 1..2, extra
descriptors of more than 4 octets, group widths above 32 bits, group lengths that do not sum to N, a section 7 too short for what
section 5 announces, JPEG 2000, PNG, CCSDS packing of signed samples or with restricted IDs or padded RSIs, spherical harmonics, IEEE floating point), -i / column-major / alternating-row scanning, predefined bitmaps, several fields
in one edition-2 message, ECMWF's large-message extension of edition 1.

No file written by ecCodes, g2clib or wgrib2 was at hand when this was written: the reader is held to hand-assembled messages and to
the independent writers of ``tests/grib_cases.py``, ``tests/grib_complex_cases.py`` and ``tests/grib_ccsds_cases.py``, not to real archive
files.  Parity with the output of those libraries is unverified - with one exception: the CCSDS streams are libaec's own (the library
ecCodes writes section 7 of a 5.42 message with), so the stream decode is held to the real encoder; a whole 5.42 message ecCodes wrote
remains unverified.
"""
from __future__ import annotations

import datetime as _dt
import math
import os
import struct

import numpy as np
import pandas as pd

# edition 1, table version 128 (ECMWF): parameter number -> short name
ED1_TABLE128 = {165: "u10", 166: "v10", 167: "t2m", 168: "d2m", 34: "sst", 134: "sp", 151: "msl", 201: "mx2t", 202: "mn2t", 228: "tp",
                130: "t", 139: "stl1", 39: "swvl1", 169: "ssrd"}
# edition 2: short name -> (discipline, category, number[, type of first fixed surface[, level]])
ED2_NAMES = {"t2m": (0, 0, 0, 103, 2), "d2m": (0, 0, 6, 103, 2), "u10": (0, 2, 2, 103, 10), "v10": (0, 2, 3, 103, 10),
             "sp": (0, 3, 0, 1), "msl": (0, 3, 1, 101), "t": (0, 0, 0)}
_ED1_NAMES = {v: k for k, v in ED1_TABLE128.items()}
_UNIT_SECONDS = {0: 60, 1: 3600, 2: 86400, 10: 10800, 11: 21600, 12: 43200}       # + second: 254 in edition 1, 13 in edition 2
_DRT_BYTES = {0: 20, 2: 47, 3: 49, 42: 25}                                       # the octets of section 5 under each template that is read
_CCSDS_REFUSED = ((1, "signed samples"), (16, "restricted block IDs"), (32, "RSIs padded to bytes"), (64, "flag 64"), (128, "flag 128"))
_SCAN_REFUSED = ((0x80, "-i (east to west)"), (0x20, "j-consecutive (column-major)"), (0x10, "alternating-row"))
_DRT_NAMES = {0: "simple packing", 2: "complex packing", 3: "complex packing with spatial differencing", 40: "JPEG 2000", 41: "PNG", 42: "CCSDS",
              50: "spherical harmonics", 51: "spherical harmonics, complex packing", 4: "IEEE floating point"}


def is_grib(path) -> bool:
    """Does ``path`` start with ``GRIB``?"""
    try:
        with open(path, "rb") as f:
            return f.read(4) == b"GRIB"
    except (OSError, TypeError):
        return False


def sign_magnitude(v: int, bits: int) -> int:
    """A sign-magnitude integer of ``bits`` bits: the top bit is the sign, the rest the magnitude."""
    top = 1 << (bits - 1)
    return -(v & (top - 1)) if v & top else v


def ibm_float(word: int) -> float:
    """An IBM hexadecimal float (sign, 7-bit exponent A, 24-bit mantissa B): ``±16^(A-64) * B / 2^24``, exact in float64."""
    b = word & 0xFFFFFF
    v = math.ldexp(float(b), 4 * (((word >> 24) & 0x7F) - 64) - 24)
    return -v if word >> 31 else v


def _unit_seconds(unit: int, edition: int) -> int:
    if unit in _UNIT_SECONDS:
        return _UNIT_SECONDS[unit]
    if unit == (254 if edition == 1 else 13):
        return 1
    raise ValueError(f"unit of time range {unit} is not read (minute, hour, day, 3 / 6 / 12 hours and second are)")


def _refuse_scan(scan: int):
    for bit, what in _SCAN_REFUSED:
        if scan & bit:
            raise ValueError(f"{what} scanning (scanning mode {scan:#04x}, bit {bit:#04x}) is not read")


class Message:
    """One field: what its headers say and where its packed bits (and its bitmap) lie in the file.  No data."""
    __slots__ = ("offset", "length", "edition", "param", "level_type", "level", "valid_time", "Ni", "Nj", "La1", "La2", "Lo1", "Lo2",
                 "scan", "nbits", "E", "D", "R", "data_offset", "data_length", "bitmap_offset", "bitmap_length", "n_values",
                 # complex packing (edition 2, templates 5.2 / 5.3): ``packing`` 0 / 2 / 3; ``nbits`` is then the bits of a group reference
                 "packing", "n_groups", "ref_width", "nbits_width", "ref_len", "len_inc", "last_len", "nbits_len", "order", "extra",
                 # CCSDS packing (edition 2, template 5.42): ``packing`` 42; ``nbits`` is the bits of a sample
                 "ccsds_flags", "block_size", "rsi")
    COMPLEX_FIELDS = ("n_groups", "ref_width", "nbits_width", "ref_len", "len_inc", "last_len", "nbits_len", "order", "extra")
    CCSDS_FIELDS = ("ccsds_flags", "block_size", "rsi")

    @property
    def grid(self):
        return (self.Ni, self.Nj, self.La1, self.La2, self.Lo1, self.Lo2)

    @property
    def s(self) -> float:
        return 2.0 ** self.E

    @property
    def d(self) -> float:
        return 10.0 ** -self.D

    @property
    def short_name(self):
        if self.edition == 1:
            return ED1_TABLE128.get(self.param[0]) if self.param[1] == 128 else None
        for name, key in ED2_NAMES.items():
            if _ed2_match(key, self):
                return name
        return None

    def __repr__(self):
        return (f"<grib.Message ed{self.edition} {self.param} level {self.level_type}:{self.level} {self.valid_time} "
                f"{self.Nj}x{self.Ni} nbits={self.nbits} at {self.offset}>")


def _ed2_match(key, m) -> bool:
    if tuple(key[:3]) != tuple(m.param):
        return False
    if len(key) > 3 and key[3] != m.level_type:
        return False
    return len(key) <= 4 or key[4] == m.level


class Field:
    """The messages of one variable in time order: what `GribFile.select` returns.  ``dims`` / ``shape`` / ``dtype`` / ``attrs`` are
    what `io` asks of a streamed source."""
    dims = ("time", "latitude", "longitude")
    dtype = np.dtype(np.float32)

    def __init__(self, gf, var, messages):
        self.file, self.path, self.var, self.messages = gf, gf.path, var, messages
        m = messages[0]
        self.shape = (len(messages), m.Nj, m.Ni)
        self.attrs = {"GRIB_edition": m.edition, "GRIB_param": ".".join(str(p) for p in m.param)}
        self._time = self._arrays = None

    @property
    def time(self) -> pd.DatetimeIndex:
        if self._time is None:
            self._time = pd.DatetimeIndex(np.array([m.valid_time for m in self.messages], dtype="datetime64[s]").astype("datetime64[ns]"))
        return self._time

    def arrays(self) -> dict:
        """The messages' numbers as arrays, one element per step (built once): ``nbits``, ``R``, ``s``, ``d``, ``data_offset``,
        ``data_length``, ``bitmap_offset`` (-1: none), ``packing`` (0 / 2 / 3 / 42), ``n_values``, the group parameters of complex
        packing (`Message.COMPLEX_FIELDS`; 0 for any other step) and the parameters of CCSDS packing (`Message.CCSDS_FIELDS`) — what the device route lays its staging plan out from."""
        if self._arrays is None:
            ms = self.messages
            self._arrays = {
                "packing": np.array([m.packing for m in ms], dtype=np.int64), "n_values": np.array([m.n_values for m in ms], dtype=np.int64),
                **{k: np.array([getattr(m, k) for m in ms], dtype=np.int64) for k in Message.COMPLEX_FIELDS + Message.CCSDS_FIELDS},
                "nbits": np.array([m.nbits for m in ms], dtype=np.int64), "R": np.array([m.R for m in ms], dtype=np.float64),
                "s": np.array([m.s for m in ms], dtype=np.float64), "d": np.array([m.d for m in ms], dtype=np.float64),
                "data_offset": np.array([m.data_offset for m in ms], dtype=np.int64), "data_length": np.array([m.data_length for m in ms], dtype=np.int64),
                "bitmap_offset": np.array([-1 if m.bitmap_offset is None else m.bitmap_offset for m in ms], dtype=np.int64)}
        return self._arrays

    def coords(self) -> dict:
        m = self.messages[0]
        lo2 = m.Lo2 + 360.0 if m.Lo2 < m.Lo1 else m.Lo2
        return {"time": self.time, "latitude": np.linspace(m.La1, m.La2, m.Nj), "longitude": np.linspace(m.Lo1, lo2, m.Ni)}


_INDEX_CACHE = {}                      # path -> (size, mtime_ns, GribFile): the last few files indexed (`open_index`)


def open_index(path) -> "GribFile":
    """`GribFile(path)`, kept for the next caller while the file's size and modification time stay what they were: a job opens the
    same file for its grid, its time coordinate and every window of its steps, and a year of hourly messages takes 40 ms to walk."""
    st = os.stat(path)
    hit = _INDEX_CACHE.get(path)
    if hit is not None and hit[0] == st.st_size and hit[1] == st.st_mtime_ns:
        return hit[2]
    gf = GribFile(path)
    while len(_INDEX_CACHE) >= 8:
        _INDEX_CACHE.pop(next(iter(_INDEX_CACHE)))
    _INDEX_CACHE[path] = (st.st_size, st.st_mtime_ns, gf)
    return gf


class GribFile:
    """The index of a GRIB file: ``messages``, one `Message` per field, in file order."""

    def __init__(self, path):
        self.path = path
        self.messages = []
        self._selected = {}
        fd = os.open(path, os.O_RDONLY)
        try:
            self.size = os.fstat(fd).st_size
            self._walk(fd)
        finally:
            os.close(fd)

    # ---- the walk ----
    def _walk(self, fd):
        pos, size = 0, self.size
        while pos + 8 <= size:
            head = os.pread(fd, 16, pos)
            if head[:4] != b"GRIB":
                pos = self._next_magic(fd, pos)
                if pos < 0:
                    break
                continue
            edition = head[7]
            if edition == 1:
                total = int.from_bytes(head[4:7], "big")
                if total & 0x800000:
                    raise ValueError(f"{self.path}: message at offset {pos}: the edition-1 length has bit 23 set "
                                     "(ECMWF's large-message extension), which is not read")
            elif edition == 2:
                if len(head) < 16:
                    raise ValueError(f"{self.path}: the message at offset {pos} is cut short")
                total = int.from_bytes(head[8:16], "big")
            else:
                raise ValueError(f"{self.path}: message at offset {pos}: GRIB edition {edition} is not read")
            if total < 12 or pos + total > size or os.pread(fd, 4, pos + total - 4) != b"7777":
                raise ValueError(f"{self.path}: the message at offset {pos} ({total} bytes) does not end with '7777': "
                                 "the file is cut short or damaged")
            try:
                self.messages.append(self._edition1(fd, pos, total, head) if edition == 1 else self._edition2(fd, pos, total, head))
            except ValueError as e:
                raise ValueError(f"{self.path}: message at offset {pos}: {e}") from None
            pos += total

    def _next_magic(self, fd, pos) -> int:
        """The offset of the next ``GRIB`` after ``pos`` (bytes between messages are skipped), or -1."""
        pos += 1
        while pos < self.size:
            buf = os.pread(fd, 1 << 16, pos)
            k = buf.find(b"GRIB")
            if k >= 0:
                return pos + k
            if len(buf) < 4:
                break
            pos += len(buf) - 3
        return -1

    @staticmethod
    def _edition1(fd, off, total, head) -> Message:
        m = Message()
        m.offset, m.length, m.edition = off, total, 1
        m.packing = 0
        for k in Message.COMPLEX_FIELDS + Message.CCSDS_FIELDS:
            setattr(m, k, 0)
        end = off + total - 4
        # the indicator, the PDS and the GDS in one read (8 + 28 + 32 bytes as a rule), then one read per later section header
        buf = os.pread(fd, 128, off)
        p = 8
        n1 = int.from_bytes(buf[p:p + 3], "big")
        if n1 < 28:
            raise ValueError(f"product definition section of {n1} bytes (at least 28)")
        pds = buf[p:p + 28]
        flags = pds[7]
        m.param = (pds[8], pds[3])                                      # (parameter, table version)
        m.level_type, m.level = pds[9], int.from_bytes(pds[10:12], "big")
        year = (pds[24] - 1) * 100 + pds[12]
        ref = _dt.datetime(year, pds[13], pds[14], pds[15], pds[16])
        unit, p1, p2, tri = pds[17], pds[18], pds[19], pds[20]
        if tri in (0, 1):
            step = p1
        elif tri == 10:
            step = (p1 << 8) | p2
        elif tri in (2, 3, 4, 5):
            step = p2
        else:
            raise ValueError(f"time range indicator {tri} is not read (0, 1, 2-5 and 10 are)")
        m.valid_time = ref + _dt.timedelta(seconds=step * _unit_seconds(unit, 1))
        m.D = sign_magnitude(int.from_bytes(pds[26:28], "big"), 16)
        p += n1
        if not flags & 0x80:
            raise ValueError("no grid description section: a predefined grid is not read")
        gds = buf[p:p + 32] if p + 32 <= len(buf) else os.pread(fd, 32, off + p)
        n2 = int.from_bytes(gds[0:3], "big")
        if gds[5] != 0:
            raise ValueError(f"data representation type {gds[5]} ({'Gaussian grid' if gds[5] == 4 else 'not a regular latitude/longitude grid'}) is not read")
        if n2 < 28:
            raise ValueError(f"grid description section of {n2} bytes")
        m.Ni, m.Nj = int.from_bytes(gds[6:8], "big"), int.from_bytes(gds[8:10], "big")
        m.La1 = sign_magnitude(int.from_bytes(gds[10:13], "big"), 24) / 1000.0
        m.Lo1 = sign_magnitude(int.from_bytes(gds[13:16], "big"), 24) / 1000.0
        m.La2 = sign_magnitude(int.from_bytes(gds[17:20], "big"), 24) / 1000.0
        m.Lo2 = sign_magnitude(int.from_bytes(gds[20:23], "big"), 24) / 1000.0
        m.scan = gds[27]
        _refuse_scan(m.scan)
        p += n2
        m.bitmap_offset = m.bitmap_length = None
        if flags & 0x40:
            bms = buf[p:p + 6] if p + 6 <= len(buf) else os.pread(fd, 6, off + p)
            n3 = int.from_bytes(bms[0:3], "big")
            predefined = int.from_bytes(bms[4:6], "big")
            if predefined != 0:
                raise ValueError(f"predefined bitmap {predefined} is not read (only a bitmap that follows in the message)")
            m.bitmap_offset, m.bitmap_length = off + p + 6, n3 - 6
            if n3 < 6 or m.bitmap_length * 8 < m.Ni * m.Nj:
                raise ValueError(f"bitmap of {m.bitmap_length} bytes for {m.Ni * m.Nj} grid points")
            p += n3
        bds = buf[p:p + 11] if p + 11 <= len(buf) else os.pread(fd, 11, off + p)
        if off + p + 11 > end or len(bds) < 11:
            raise ValueError("the binary data section lies beyond the end of the message")
        n4 = int.from_bytes(bds[0:3], "big")
        if bds[3] & 0xF0:
            f = bds[3]
            what = ("spherical harmonic coefficients" if f & 0x80 else "second-order (complex) packing" if f & 0x40
                    else "integer original values" if f & 0x20 else "additional flags in octet 14")
            raise ValueError(f"{what} (binary data section flags {f >> 4:#x}) not read: only grid-point data in simple packing")
        m.E = sign_magnitude(int.from_bytes(bds[4:6], "big"), 16)
        m.R = ibm_float(int.from_bytes(bds[6:10], "big"))
        m.nbits = bds[10]
        if m.nbits > 32:
            raise ValueError(f"{m.nbits} bits per value (at most 32)")
        m.data_offset, m.data_length = off + p + 11, n4 - 11
        if n4 < 11 or m.data_offset + m.data_length > end:
            raise ValueError(f"binary data section of {n4} bytes leaves the message")
        m.n_values = (m.data_length * 8 - (bds[3] & 0x0F)) // m.nbits if m.nbits else 0
        return m

    @staticmethod
    def _edition2(fd, off, total, head) -> Message:
        m = Message()
        m.offset, m.length, m.edition = off, total, 2
        m.packing = 0
        for k in Message.COMPLEX_FIELDS + Message.CCSDS_FIELDS:
            setattr(m, k, 0)
        discipline = head[6]
        end = off + total - 4
        pos = off + 16
        seen = set()
        m.bitmap_offset = m.bitmap_length = None
        ref = step_s = None
        while pos < end:
            sec = os.pread(fd, 80, pos)                               # one small read per section header
            if len(sec) < 5:
                raise ValueError("a section header is cut short")
            n, num = int.from_bytes(sec[0:4], "big"), sec[4]
            if n < 5 or pos + n > end:
                raise ValueError(f"section {num} of {n} bytes leaves the message")
            if num in seen and num >= 2:
                raise ValueError(f"section {num} is repeated: several fields in one message are not read")
            if num < 1 or num > 7:
                raise ValueError(f"unknown section number {num}")
            seen.add(num)
            if num == 1:
                ref = _dt.datetime(int.from_bytes(sec[12:14], "big"), sec[14], sec[15], sec[16], sec[17], sec[18])
            elif num == 3:
                if sec[10] != 0:
                    raise ValueError("a grid with an optional list of numbers of points (a reduced grid) is not read")
                tmpl = int.from_bytes(sec[12:14], "big")
                if tmpl != 0:
                    raise ValueError(f"grid definition template 3.{tmpl} ({'Gaussian grid' if tmpl == 40 else 'not a regular latitude/longitude grid'}) is not read")
                if n < 72:
                    raise ValueError(f"grid definition section of {n} bytes")
                m.Ni, m.Nj = int.from_bytes(sec[30:34], "big"), int.from_bytes(sec[34:38], "big")
                basic, sub = int.from_bytes(sec[38:42], "big"), int.from_bytes(sec[42:46], "big")
                if basic not in (0, 0xFFFFFFFF) or sub not in (0, 0xFFFFFFFF):
                    raise ValueError(f"basic angle {basic} with subdivisions {sub}: only angles in 1e-6 degrees are read")
                m.La1 = sign_magnitude(int.from_bytes(sec[46:50], "big"), 32) / 1e6
                m.Lo1 = sign_magnitude(int.from_bytes(sec[50:54], "big"), 32) / 1e6
                m.La2 = sign_magnitude(int.from_bytes(sec[55:59], "big"), 32) / 1e6
                m.Lo2 = sign_magnitude(int.from_bytes(sec[59:63], "big"), 32) / 1e6
                m.scan = sec[71]
                _refuse_scan(m.scan)
                if int.from_bytes(sec[6:10], "big") != m.Ni * m.Nj:
                    raise ValueError(f"{int.from_bytes(sec[6:10], 'big')} data points on a grid of {m.Nj} x {m.Ni}")
            elif num == 4:
                tmpl = int.from_bytes(sec[7:9], "big")
                if tmpl not in (0, 8):
                    raise ValueError(f"product definition template 4.{tmpl} is not read (4.0 and 4.8 are)")
                m.param = (discipline, sec[9], sec[10])
                m.level_type = sec[22]
                scale, value = sec[23], int.from_bytes(sec[24:28], "big")
                if scale == 0xFF or value == 0xFFFFFFFF:
                    m.level = 0
                else:
                    scale = sign_magnitude(scale, 8)
                    m.level = value if scale == 0 else value / 10.0 ** scale
                if tmpl == 0:
                    step_s = int.from_bytes(sec[18:22], "big") * _unit_seconds(sec[17], 2)
                else:
                    if n < 41:
                        raise ValueError(f"product definition section of {n} bytes for template 4.8")
                    m.valid_time = _dt.datetime(int.from_bytes(sec[34:36], "big"), sec[36], sec[37], sec[38], sec[39], sec[40])
            elif num == 5:
                tmpl = int.from_bytes(sec[9:11], "big")
                if tmpl not in _DRT_BYTES:
                    raise ValueError(f"data representation template 5.{tmpl} ({_DRT_NAMES.get(tmpl, 'unknown')}) is not read: only 5.0, "
                                     "simple packing, 5.2 / 5.3, complex packing, and 5.42, CCSDS packing")
                if n < _DRT_BYTES[tmpl]:
                    raise ValueError(f"data representation section of {n} bytes" + (f" for template 5.{tmpl} ({_DRT_NAMES[tmpl]}), which takes "
                                                                                    f"{_DRT_BYTES[tmpl]}" if tmpl else ""))
                m.packing = tmpl
                m.n_values = int.from_bytes(sec[5:9], "big")
                m.R = struct.unpack(">f", sec[11:15])[0]
                m.E = sign_magnitude(int.from_bytes(sec[15:17], "big"), 16)
                m.D = sign_magnitude(int.from_bytes(sec[17:19], "big"), 16)
                m.nbits = sec[19]
                if m.nbits > 32:
                    raise ValueError(f"{m.nbits} bits per value (at most 32)")
                if tmpl == 42:                                          # CCSDS packing: octets 22 (flags), 23 (J), 24 - 25 (rsi)
                    m.ccsds_flags, m.block_size, m.rsi = sec[21], sec[22], int.from_bytes(sec[23:25], "big")
                    for bit, what in _CCSDS_REFUSED:
                        if m.ccsds_flags & bit:
                            raise ValueError(f"template 5.42: CCSDS flags {m.ccsds_flags:#04x} with bit {bit} ({what}) are not read (2, 4 and 8 are)")
                    if m.block_size not in (8, 16, 32, 64):
                        raise ValueError(f"template 5.42: a block size of {m.block_size} samples is not read (8, 16, 32 and 64 are)")
                    if not 1 <= m.rsi <= 4096:
                        raise ValueError(f"template 5.42: a reference sample interval of {m.rsi} blocks is not read (1..4096 are)")
                elif tmpl:                                              # complex packing: octets 21 - 47 (5.2), - 49 (5.3)
                    if sec[22] != 0:
                        raise ValueError(f"template 5.{tmpl}: missing value management {sec[22]} (primary / secondary missing values "
                                         "inside the groups) is not read, only 0")
                    m.n_groups, m.ref_width, m.nbits_width = int.from_bytes(sec[31:35], "big"), sec[35], sec[36]
                    m.ref_len, m.len_inc, m.last_len, m.nbits_len = int.from_bytes(sec[37:41], "big"), sec[41], int.from_bytes(sec[42:46], "big"), sec[46]
                    if m.nbits_width > 32 or m.nbits_len > 32:
                        raise ValueError(f"template 5.{tmpl}: group widths of {m.nbits_width} bits and lengths of {m.nbits_len} bits (at most 32)")
                    if tmpl == 3:
                        m.order, m.extra = sec[47], sec[48]
                        if m.order not in (1, 2):
                            raise ValueError(f"template 5.3: spatial differencing of order {m.order} is not read (1 and 2 are)")
                        if m.extra > 4:
                            raise ValueError(f"template 5.3: extra descriptors of {m.extra} octets are not read (at most 4)")
            elif num == 6:
                ind = sec[5]
                if ind == 0:
                    m.bitmap_offset, m.bitmap_length = pos + 6, n - 6
                elif ind == 254:
                    raise ValueError("bitmap indicator 254 (the bitmap of an earlier field of the message) is not read")
                elif ind != 255:
                    raise ValueError(f"predefined bitmap (indicator {ind}) is not read (only a bitmap that follows in the message)")
            elif num == 7:
                m.data_offset, m.data_length = pos + 5, n - 5
            pos += n
        missing = [k for k in (1, 3, 4, 5, 6, 7) if k not in seen]
        if missing:
            raise ValueError(f"sections {missing} are missing")
        if step_s is not None:
            m.valid_time = ref + _dt.timedelta(seconds=step_s)
        if m.bitmap_length is not None and m.bitmap_length * 8 < m.Ni * m.Nj:
            raise ValueError(f"bitmap of {m.bitmap_length} bytes for {m.Ni * m.Nj} grid points")
        if m.packing and (m.n_values > m.Ni * m.Nj or (m.bitmap_offset is None and m.n_values != m.Ni * m.Nj)):
            raise ValueError(f"template 5.{m.packing}: {m.n_values} packed values on a grid of {m.Ni * m.Nj} points")
        return m

    # ---- choosing a variable ----
    def _matches(self, var, m) -> bool:
        var = str(var)
        parts = var.split(".")
        if all(p.isdigit() for p in parts):
            nums = tuple(int(p) for p in parts)
            if m.edition == 1:
                return len(nums) in (1, 2) and nums[0] == m.param[0] and (len(nums) == 1 or nums[1] == m.param[1])
            return len(nums) >= 3 and _ed2_match(nums, m)
        if m.edition == 1:
            return m.param[1] == 128 and _ED1_NAMES.get(var) == m.param[0]
        return var in ED2_NAMES and _ed2_match(ED2_NAMES[var], m)

    def select(self, var, filter_by_keys=None) -> Field:
        """The messages of ``var`` — a short name of the tables above, or ``"167"`` / ``"167.128"`` (edition 1: parameter[.table]) /
        ``"0.0.0"`` (edition 2: discipline.category.number) — in the order of their valid times.  ``filter_by_keys={"level": N}`` picks
        one level where the variable has several."""
        memo = (str(var), tuple(sorted((filter_by_keys or {}).items())))
        if memo in self._selected:
            return self._selected[memo]
        keys = dict(filter_by_keys or {})
        level = keys.pop("level", None)
        if keys:
            raise ValueError(f"filter_by_keys: {sorted(keys)} not understood (only 'level' is)")
        msgs = [m for m in self.messages if self._matches(var, m)]
        if not msgs:
            found = sorted({m.short_name or ".".join(str(p) for p in m.param) for m in self.messages})
            raise KeyError(f"{var!r} not in {self.path}: {found}")
        if level is not None:
            msgs = [m for m in msgs if m.level == level]
            if not msgs:
                raise ValueError(f"{self.path}: no message of {var!r} at level {level}")
        levels = sorted({(m.level_type, m.level) for m in msgs})
        if len(levels) > 1:
            raise ValueError(f"{self.path}: {var!r} has several levels (level type, level): {levels}; pick one with filter_by_keys={{'level': N}}")
        m0 = msgs[0]
        for m in msgs:
            if m.edition != m0.edition:
                raise ValueError(f"{self.path}: the messages of {var!r} mix GRIB editions 1 and 2")
            if m.grid != m0.grid or m.scan != m0.scan:
                raise ValueError(f"{self.path}: the messages of {var!r} do not share one grid and scanning mode "
                                 f"(offset {m0.offset}: {m0.grid}, {m0.scan:#04x}; offset {m.offset}: {m.grid}, {m.scan:#04x})")
        msgs.sort(key=lambda m: m.valid_time)                               # (stable)
        for a, b in zip(msgs, msgs[1:]):
            if a.valid_time == b.valid_time:
                raise ValueError(f"{self.path}: two messages of {var!r} share the valid time {a.valid_time} (offsets {a.offset} and {b.offset})")
        self._selected[memo] = Field(self, var, msgs)
        return self._selected[memo]

    # ---- host decode ----
    def read(self, var, filter_by_keys=None, steps=None) -> np.ndarray:
        """float32 (time, latitude, longitude) of ``var``, rows in stored order, NaN where a bitmap has 0.  ``steps=(k0, k1)``: those
        steps of the time-ordered field only."""
        field = var if isinstance(var, Field) else self.select(var, filter_by_keys)
        msgs = field.messages if steps is None else field.messages[int(steps[0]):int(steps[1])]
        out = np.empty((len(msgs), field.shape[1], field.shape[2]), dtype=np.float32)
        fd = os.open(self.path, os.O_RDONLY)
        try:
            for k, m in enumerate(msgs):
                out[k] = decode_message(m, os.pread(fd, m.data_length, m.data_offset),
                                        os.pread(fd, m.bitmap_length, m.bitmap_offset) if m.bitmap_offset is not None else None)
        finally:
            os.close(fd)
        return out


def unpack_bits(data: bytes, nbits: int, count: int) -> np.ndarray:
    """The first ``count`` ``nbits``-bit big-endian unsigned integers of ``data`` as uint64 (vectorised; nbits 0..32)."""
    if nbits == 0 or count == 0:
        return np.zeros(count, dtype=np.uint64)
    if (count * nbits + 7) // 8 > len(data):
        raise ValueError(f"{count} values of {nbits} bits need {(count * nbits + 7) // 8} bytes, the data section has {len(data)}")
    if nbits in (8, 16, 32):
        return np.frombuffer(data, dtype=f">u{nbits // 8}", count=count).astype(np.uint64)
    buf = np.zeros(len(data) + 8, dtype=np.uint8)
    buf[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    bit = np.arange(count, dtype=np.int64) * nbits
    byte, off = bit >> 3, (bit & 7).astype(np.uint64)
    win = np.zeros(count, dtype=np.uint64)                                   # the 40 bits from the value's first byte on
    for k in range(5):
        win |= buf[byte + k].astype(np.uint64) << np.uint64(8 * (4 - k))
    return (win >> (np.uint64(40 - nbits) - off)) & np.uint64((1 << nbits) - 1)


def _cut_bits(buf: np.ndarray, bit: np.ndarray, width) -> np.ndarray:
    """The big-endian unsigned integers of ``width`` bits (0..32; an array or one number) that begin at the bits ``bit`` of ``buf``, as
    uint64: the 40-bit window of `unpack_bits`, with a width of its own for every value.  ``buf`` has 8 bytes of slack at its end."""
    byte, off = bit >> 3, (bit & 7).astype(np.uint64)
    win = np.zeros(len(bit), dtype=np.uint64)
    for k in range(5):
        win |= buf[byte + k].astype(np.uint64) << np.uint64(8 * (4 - k))
    w = np.broadcast_to(np.asarray(width, dtype=np.uint64), win.shape)
    return (win >> (np.uint64(40) - w - off)) & ((np.uint64(1) << w) - np.uint64(1))


def unpack_complex(m, data: bytes) -> np.ndarray:
    """The ``m.n_values`` integers X (int64) of a complex-packed message (templates 5.2 / 5.3) from the body of its section 7: the
    group tables, the values cut out group by group, and the spatial differencing undone by one or two running sums (the module
    docstring has the layout).  int64 throughout, wrapping like the kernels."""
    N, NG, tag = int(m.n_values), int(m.n_groups), f"template 5.{m.packing}"
    if NG == 0:
        return np.zeros(N, dtype=np.int64)
    total = len(data) * 8
    buf = np.zeros(len(data) + 8, dtype=np.uint8)
    buf[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    pos = 0

    def need(bits, what):
        if pos + bits > total:
            raise ValueError(f"{tag}: section 7 holds {len(data)} bytes, too short for {what} ({(pos + bits + 7) // 8} bytes)")

    ival = [0, 0, 0]                                                          # ival1, ival2, minsd
    if m.packing == 3 and m.extra:
        need(8 * m.extra * (m.order + 1), "the extra descriptors")
        words = [sign_magnitude(int.from_bytes(data[k * m.extra:(k + 1) * m.extra], "big"), 8 * m.extra) for k in range(m.order + 1)]
        ival[:m.order], ival[2] = words[:m.order], words[m.order]
        pos = 8 * m.extra * (m.order + 1)
    tables = []
    for nb, what in ((m.nbits, "group references"), (m.nbits_width, "group widths"), (m.nbits_len, "group lengths")):
        need(nb * NG, f"{NG} {what} of {nb} bits")
        tables.append(_cut_bits(buf, pos + np.arange(NG, dtype=np.int64) * nb, nb).astype(np.int64))
        pos = (pos + nb * NG + 7) // 8 * 8
    refs, widths, lens = tables[0], m.ref_width + tables[1], m.ref_len + m.len_inc * tables[2]
    lens[-1] = m.last_len
    if int(widths.max()) > 32:
        raise ValueError(f"{tag}: a group of {int(widths.max())} bits per value (at most 32)")
    if int(lens.sum()) != N:
        raise ValueError(f"{tag}: the group lengths sum to {int(lens.sum())}, the section announces {N} values")
    w = np.repeat(widths, lens)
    bit = np.cumsum(w) - w + pos
    need(int(w.sum()), f"{N} values in {NG} groups")
    raw = np.repeat(refs, lens) + _cut_bits(buf, bit, w).astype(np.int64)
    if m.packing == 2:
        return raw
    g = raw + np.int64(ival[2])
    g[0] = 0
    if m.order == 2 and N > 1:
        g[1] = ival[1] - ival[0]
    for _ in range(m.order):
        g = np.cumsum(g, dtype=np.int64)
    return g + np.int64(ival[0])


def unpack_ccsds(m, data: bytes) -> np.ndarray:
    """The ``m.n_values`` integers X (int64, each below 2**32) of a CCSDS-packed message (template 5.42) from the body of its section 7:
    the passes of ``aec_passes.h`` on the host (`codec.aec_decode`).  A stream that is damaged or ends before its last sample raises."""
    from . import codec
    if m.nbits == 0:
        return np.zeros(int(m.n_values), dtype=np.int64)
    try:
        return codec.aec_decode(data, m.n_values, m.nbits, m.ccsds_flags, m.block_size, m.rsi).astype(np.int64)
    except codec.CodecError as e:
        raise ValueError(f"template 5.42: section 7 of {len(data)} bytes does not hold {m.n_values} samples of {m.nbits} bits "
                         f"(block size {m.block_size}, rsi {m.rsi}, flags {m.ccsds_flags:#04x}): {e}") from None


def decode_message(m, data: bytes, bitmap: bytes | None) -> np.ndarray:
    """float32 (Nj, Ni) of one message from its packed bits and its bitmap: ``((X * s) + R) * d`` in float64, rounded once.  X is an
    unsigned integer of at most 32 bits under simple and CCSDS packing and a signed int64 under complex packing; the conversion to float64 is
    exact while ``|X| < 2**53``."""
    n = m.Ni * m.Nj
    if m.packing:
        have = None
        if bitmap is not None:
            if len(bitmap) * 8 < n:
                raise ValueError(f"bitmap of {len(bitmap)} bytes for {n} grid points")
            have = np.unpackbits(np.frombuffer(bitmap, dtype=np.uint8), count=n).astype(bool)
        if m.n_values != (n if have is None else int(have.sum())):
            raise ValueError(f"template 5.{m.packing}: {m.n_values} packed values for {n if have is None else int(have.sum())} present grid points")
        X = unpack_ccsds(m, data) if m.packing == 42 else unpack_complex(m, data)
        v = (((X.astype(np.float64) * m.s) + m.R) * m.d).astype(np.float32)
        if have is None:
            return v.reshape(m.Nj, m.Ni)
        out = np.full(n, np.nan, dtype=np.float32)
        out[have] = v
        return out.reshape(m.Nj, m.Ni)
    if bitmap is None:
        x = unpack_bits(data, m.nbits, n)
        return (((x.astype(np.float64) * m.s) + m.R) * m.d).astype(np.float32).reshape(m.Nj, m.Ni)
    if len(bitmap) * 8 < n:
        raise ValueError(f"bitmap of {len(bitmap)} bytes for {n} grid points")
    have = np.unpackbits(np.frombuffer(bitmap, dtype=np.uint8), count=n).astype(bool)
    x = unpack_bits(data, m.nbits, int(have.sum()))
    out = np.full(n, np.nan, dtype=np.float32)
    out[have] = (((x.astype(np.float64) * m.s) + m.R) * m.d).astype(np.float32)
    return out.reshape(m.Nj, m.Ni)
