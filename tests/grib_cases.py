"""A small catalogue of GRIB files (editions 1 and 2, regular latitude / longitude grids, simple packing) for tests/test_grib.py and
tests/test_gpu_grib.py, with its own writer: deliberately naive and independent of aggfly_amd/grib.py.  The fields are packed through
Python big integers, sign-magnitude numbers are put together bit by bit, and the IBM float of edition 1 is found by a search over
the exponent.  Every case keeps the integers X, the bitmaps and the header numbers it wrote; the expected array is
``float32(((X * s) + R) * d)`` from those, NaN where the bitmap has 0.

    edition 1   'GRIB' len(3) 1 | PDS (28) | GDS (32) | [BMS: len(3) unused predefined(2) bits] | BDS: len(3) flags|unused E(2) R(4) nbits bits | '7777'
    edition 2   'GRIB' 0 0 discipline 2 len(8) | 1 (21) | 3 (72) | 4 (34 or 58) | 5 (21) | 6 (6 + bits) | 7 (5 + bits) | '7777'
"""
import datetime as dt
import os

import numpy as np

BASE = dt.datetime(2024, 7, 15, 0, 0)
NJ, NI, STEPS = 5, 9, 7


# ---------------------------------------------------------------------------------------
# numbers
# ---------------------------------------------------------------------------------------
def u(v: int, nbytes: int) -> bytes:
    assert 0 <= v < (1 << (8 * nbytes)), (v, nbytes)
    return int(v).to_bytes(nbytes, "big")


def sm(v: int, nbytes: int) -> bytes:
    """Sign-magnitude: the top bit is the sign, the rest the magnitude."""
    mag = abs(int(v))
    assert mag < (1 << (8 * nbytes - 1))
    return u(mag | ((1 << (8 * nbytes - 1)) if v < 0 else 0), nbytes)


def ibm(x: float) -> bytes:
    """The IBM hexadecimal float of ``x``, by a search over the exponent A for a 24-bit mantissa B with ±16^(A-64)·B/2^24 == x;
    the largest mantissa (the normalised form) wins.  ``x`` must be representable."""
    if x == 0:
        return b"\x00\x00\x00\x00"
    best = None
    for a in range(128):
        b = abs(x) * 2.0 ** 24 / 16.0 ** (a - 64)
        if b == int(b) and 0 < b < (1 << 24):
            best = (a, int(b))                                   # (B shrinks as A grows: keep the first hit)
            break
    assert best is not None, f"{x} is no IBM float"
    a, b = best
    return u(((0x80 | a) if x < 0 else a) << 24 | b, 4)


def pack_bits(values, nbits: int) -> tuple:
    """(bytes, bit count) of ``values`` as ``nbits``-bit big-endian integers, through one Python big integer; zero bits pad the last byte."""
    big, n = 0, 0
    for v in values:
        assert 0 <= int(v) < (1 << nbits) or (nbits == 0 and int(v) == 0)
        big = (big << nbits) | int(v)
        n += nbits
    pad = -n % 8
    return (big << pad).to_bytes((n + pad) // 8, "big"), n


# ---------------------------------------------------------------------------------------
# one field and its messages
# ---------------------------------------------------------------------------------------
class Step:
    """One field as written: ``X`` — the packed integers of the PRESENT points, in scan order —, ``bitmap`` (a list of 0 / 1 per grid
    point, or None), the packing numbers and the valid time."""

    def __init__(self, X, nbits, E=0, D=0, R=0.0, bitmap=None, valid=BASE, **header):
        self.X, self.nbits, self.E, self.D, self.R, self.bitmap, self.valid, self.header = list(X), nbits, E, D, float(R), bitmap, valid, header

    def expected(self, nj, ni) -> np.ndarray:
        s, d = 2.0 ** self.E, 10.0 ** -self.D
        vals = [np.float32(((float(x) * s) + self.R) * d) for x in self.X]
        if self.bitmap is None:
            out = vals
        else:
            it = iter(vals)
            out = [next(it) if b else np.float32(np.nan) for b in self.bitmap]
        return np.array(out, dtype=np.float32).reshape(nj, ni)


def message1(step, grid, param=167, table=128, level_type=1, level=0, ref=None, unit=1, p1=0, p2=0, tri=0, gds_type=0,
             bds_flags=0, predefined_bitmap=0, gds=True):
    """An edition-1 message of ``step`` on ``grid`` = (Ni, Nj, La1, Lo1, La2, Lo2, scan), angles in degrees."""
    ni, nj, la1, lo1, la2, lo2, scan = grid
    ref = step.valid if ref is None else ref
    flags = (0x80 if gds else 0) | (0x40 if step.bitmap is not None or predefined_bitmap else 0)
    pds = (u(28, 3) + u(table, 1) + u(98, 1) + u(145, 1) + u(255, 1) + u(flags, 1) + u(param, 1) + u(level_type, 1) + u(level, 2)
           + u((ref.year - 1) % 100 + 1, 1) + u(ref.month, 1) + u(ref.day, 1) + u(ref.hour, 1) + u(ref.minute, 1)
           + u(unit, 1) + u(p1, 1) + u(p2, 1) + u(tri, 1) + u(0, 2) + u(0, 1) + u((ref.year - 1) // 100 + 1, 1) + u(0, 1) + sm(step.D, 2))
    md = lambda deg: int(round(deg * 1000))
    di = abs(md(lo2 + (360 if lo2 < lo1 else 0)) - md(lo1)) // max(ni - 1, 1)
    dj = abs(md(la2) - md(la1)) // max(nj - 1, 1)
    g = (u(32, 3) + u(0, 1) + u(255, 1) + u(gds_type, 1) + u(ni, 2) + u(nj, 2) + sm(md(la1), 3) + sm(md(lo1), 3) + u(0x80, 1)
         + sm(md(la2), 3) + sm(md(lo2), 3) + u(di, 2) + u(dj, 2) + u(scan, 1) + u(0, 4)) if gds else b""
    bms = b""
    if predefined_bitmap:
        bms = u(6, 3) + u(0, 1) + u(predefined_bitmap, 2)
    elif step.bitmap is not None:
        bits, n = pack_bits(step.bitmap, 1)
        bits += b"\x00" * ((6 + len(bits)) % 2)                         # sections have an even length
        bms = u(6 + len(bits), 3) + u(len(bits) * 8 - n, 1) + u(0, 2) + bits
    data, n = pack_bits(step.X, step.nbits)
    data += b"\x00" * ((11 + len(data)) % 2)
    bds = u(11 + len(data), 3) + u((bds_flags << 4) | (len(data) * 8 - n), 1) + sm(step.E, 2) + ibm(step.R) + u(step.nbits, 1) + data
    body = pds + g + bms + bds + b"7777"
    return b"GRIB" + u(8 + len(body), 3) + u(1, 1) + body


def sections2(step, grid, param=(0, 0, 0), surface=(103, 0, 2), ref=None, unit=1, forecast=0, template=0, end=None,
              grid_template=0, drt=0, bitmap_indicator=None):
    """Sections 3 - 7 of an edition-2 message (a list of bytes, one per section)."""
    ni, nj, la1, lo1, la2, lo2, scan = grid
    ud = lambda deg: int(round(deg * 1e6))
    di = abs(ud(lo2 + (360 if lo2 < lo1 else 0)) - ud(lo1)) // max(ni - 1, 1)
    dj = abs(ud(la2) - ud(la1)) // max(nj - 1, 1)
    s3 = (u(72, 4) + u(3, 1) + u(0, 1) + u(ni * nj, 4) + u(0, 1) + u(0, 1) + u(grid_template, 2) + u(6, 1)
          + (u(255, 1) + u(0xFFFFFFFF, 4)) * 3 + u(ni, 4) + u(nj, 4) + u(0, 4) + u(0xFFFFFFFF, 4) + sm(ud(la1), 4) + sm(ud(lo1), 4) + u(0x30, 1)
          + sm(ud(la2), 4) + sm(ud(lo2), 4) + u(di, 4) + u(dj, 4) + u(scan, 1))
    body4 = (u(0, 2) + u(template, 2) + u(param[1], 1) + u(param[2], 1) + u(0, 1) + u(0, 1) + u(145, 1) + u(0, 2) + u(0, 1) + u(unit, 1)
             + u(forecast, 4) + u(surface[0], 1) + u(surface[1], 1) + u(surface[2], 4) + u(255, 1) + u(255, 1) + u(0xFFFFFFFF, 4))
    if template == 8:
        body4 += (u(end.year, 2) + u(end.month, 1) + u(end.day, 1) + u(end.hour, 1) + u(end.minute, 1) + u(end.second, 1) + u(1, 1) + u(0, 4)
                  + u(0, 1) + u(2, 1) + u(1, 1) + u(1, 4) + u(255, 1) + u(0, 4))
    s4 = u(5 + len(body4), 4) + u(4, 1) + body4
    s5 = (u(21, 4) + u(5, 1) + u(len(step.X), 4) + u(drt, 2) + np.array(step.R, dtype=">f4").tobytes() + sm(step.E, 2) + sm(step.D, 2)
          + u(step.nbits, 1) + u(0, 1))
    if bitmap_indicator is not None:
        s6 = u(6, 4) + u(6, 1) + u(bitmap_indicator, 1)
    elif step.bitmap is None:
        s6 = u(6, 4) + u(6, 1) + u(255, 1)
    else:
        bits, _ = pack_bits(step.bitmap, 1)
        s6 = u(6 + len(bits), 4) + u(6, 1) + u(0, 1) + bits
    data, _ = pack_bits(step.X, step.nbits)
    s7 = u(5 + len(data), 4) + u(7, 1) + data
    return [s3, s4, s5, s6, s7]


def message2(step, grid, ref=None, fields=None, **kw):
    """An edition-2 message: ``ref`` is the reference time (default: the step's valid time, forecast 0).  ``fields``: further
    (step, keywords) whose sections 4 - 7 are repeated in the same message."""
    ref = step.valid if ref is None else ref
    discipline = kw.get("param", (0, 0, 0))[0]
    s1 = (u(21, 4) + u(1, 1) + u(98, 2) + u(0, 2) + u(4, 1) + u(0, 1) + u(1, 1) + u(ref.year, 2) + u(ref.month, 1) + u(ref.day, 1)
          + u(ref.hour, 1) + u(ref.minute, 1) + u(ref.second, 1) + u(0, 1) + u(1, 1))
    body = s1 + b"".join(sections2(step, grid, **kw))
    for st2, kw2 in fields or []:
        body += b"".join(sections2(st2, grid, **kw2)[1:])
    body += b"7777"
    return b"GRIB" + u(0, 2) + u(discipline, 1) + u(2, 1) + u(16 + len(body), 8) + body


# ---------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------
GRID = (NI, NJ, 50.0, -10.5, 49.0, -8.5, 0x00)                         # north to south, 0.25 degrees


class Case:
    """A file as a list of pieces (messages and whatever lies between them) and what reading ``var`` from it must give: ``steps``
    in the order of their valid times."""

    def __init__(self, name, var, pieces, steps, grid=GRID, edition=1, **read_kw):
        self.name, self.var, self.pieces, self.steps, self.grid, self.edition, self.read_kw = name, var, pieces, steps, grid, edition, read_kw

    def write(self, directory) -> str:
        path = os.path.join(str(directory), self.name + (".grib" if self.edition == 1 else ".grib2"))
        with open(path, "wb") as f:
            f.write(b"".join(self.pieces))
        return path

    @property
    def expected(self) -> np.ndarray:
        ni, nj = self.grid[0], self.grid[1]
        return np.stack([s.expected(nj, ni) for s in self.steps]) if self.steps else np.empty((0, nj, ni), np.float32)

    @property
    def times(self):
        return [s.valid for s in self.steps]

    @property
    def latitude(self):
        return np.linspace(self.grid[2], self.grid[4], self.grid[1])

    @property
    def longitude(self):
        lo1, lo2 = self.grid[3], self.grid[5]
        return np.linspace(lo1, lo2 + 360.0 if lo2 < lo1 else lo2, self.grid[0])


def field(rng, nbits, k, n=NJ * NI, bitmap=None, E=-2, D=0, R=-118.625, **kw):
    """Step ``k`` (valid BASE + k hours) of random ``nbits``-bit integers that include 0 and the largest one."""
    m = n if bitmap is None else int(sum(bitmap))
    X = [int(x) for x in rng.integers(0, 1 << nbits, size=m, dtype=np.uint64)] if nbits else [0] * m
    if m and nbits:
        X[0], X[-1] = 0, (1 << nbits) - 1
    return Step(X, nbits, E, D, R, bitmap, BASE + dt.timedelta(hours=k), **kw)


def some_bitmap(rng, n=NJ * NI, keep=0.66):
    b = [int(v) for v in (rng.random(n) < keep)]
    b[0], b[1] = 1, 0
    return b


def _msgs(edition, steps, grid=GRID, **kw):
    return [(message1 if edition == 1 else message2)(s, grid, **kw) for s in steps]


def build_cases():
    rng = np.random.default_rng(20240715)
    cases = []
    for ed in (1, 2):
        R = -118.625 if ed == 1 else float(np.float32(273.15))
        for nbits in (0, 1, 7, 8, 12, 16, 24, 31, 32):
            steps = [field(rng, nbits, k, E=-2 if nbits < 24 else -12, R=R) for k in range(STEPS)]
            cases.append(Case(f"e{ed}_n{nbits}", "t2m", _msgs(ed, steps), steps, edition=ed))
        n = NJ * NI
        for tag, bm in (("some", None), ("all", [0] * n), ("none", [1] * n)):
            steps = [field(rng, 12 if ed == 1 else 16, k, bitmap=bm if bm is not None else some_bitmap(rng), R=R) for k in range(STEPS)]
            cases.append(Case(f"e{ed}_bitmap_{tag}_missing", "t2m", _msgs(ed, steps), steps, edition=ed))
        # nbits, E, R, D and the presence of a bitmap change from step to step, as in real files
        Rs = [100.0, -118.625, 1.0, 0.0, 273.125, -0.5, 4096.0]
        steps = [field(rng, (16, 12, 9, 0, 24, 16, 5)[k], k, bitmap=some_bitmap(rng) if k % 3 == 1 else None, E=(-3, 0, 2, 0, -10, -4, 1)[k],
                       D=(0, 1, -1, 0, 2, 0, 0)[k], R=Rs[k]) for k in range(STEPS)]
        cases.append(Case(f"e{ed}_varying", "t2m", _msgs(ed, steps), steps, edition=ed))
        # south to north (scanning mode 0x40: La1 < La2), and a longitude axis across the date line of the 0..360 convention
        g = (NI, NJ, -10.0, 356.0, -9.0, 4.0, 0x40)
        steps = [field(rng, 16, k, R=R) for k in range(STEPS)]
        cases.append(Case(f"e{ed}_south_to_north_lon_wraps", "t2m", _msgs(ed, steps, g), steps, grid=g, edition=ed))
        # messages out of time order, a second parameter interleaved, bytes that are no message in between
        a = [field(rng, 16, k, R=R) for k in range(STEPS)]
        b = [field(rng, 12, k, R=R) for k in range(STEPS)]
        kw_b = dict(param=168) if ed == 1 else dict(param=(0, 0, 6))
        order = [3, 0, 6, 1, 5, 2, 4]
        pieces = []
        for j, k in enumerate(order):
            pieces += _msgs(ed, [a[k]]) + ([b"\x00\x00GRI\x00garbage" * 3] if j % 2 else []) + _msgs(ed, [b[k]], **kw_b)
        cases.append(Case(f"e{ed}_shuffled_t2m", "t2m", pieces, a, edition=ed))
        cases.append(Case(f"e{ed}_shuffled_d2m", "d2m", pieces, b, edition=ed))
    # edition 1: time range indicators 0, 1 (step P1), 10 (P1 || P2) and 4 (P2), in hours, days and minutes
    ref = BASE
    spec = [(0, 1, 5, 0, 5 * 3600), (1, 1, 7, 99, 7 * 3600), (10, 1, 1, 44, 300 * 3600), (4, 1, 3, 9, 9 * 3600), (0, 2, 2, 0, 2 * 86400),
            (0, 0, 30, 0, 30 * 60), (0, 254, 45, 0, 45), (0, 10, 1, 0, 10800), (3, 12, 0, 1, 43200)]
    steps, pieces = [], []
    for tri, unit, p1, p2, secs in spec:
        st = field(rng, 16, 0)
        st.valid = ref + dt.timedelta(seconds=secs)
        steps.append(st)
        pieces.append(message1(st, GRID, ref=ref, unit=unit, p1=p1, p2=p2, tri=tri))
    cases.append(Case("e1_time_ranges", "t2m", pieces, sorted(steps, key=lambda s: s.valid), edition=1))
    # edition 2: product templates 4.0 (reference + forecast time) and 4.8 (the end of the interval)
    steps, pieces = [], []
    for k in range(STEPS):
        st = field(rng, 16, 0, R=float(np.float32(273.15)))
        if k % 2:
            st.valid = ref + dt.timedelta(hours=6 * k + 1)
            pieces.append(message2(st, GRID, ref=ref, template=8, forecast=6 * k - 5, end=st.valid))
        else:
            st.valid = ref + dt.timedelta(hours=3 * k)
            pieces.append(message2(st, GRID, ref=ref, template=0, forecast=k, unit=10))
        steps.append(st)
    cases.append(Case("e2_templates_0_and_8", "t2m", pieces, sorted(steps, key=lambda s: s.valid), edition=2))
    return cases


def refusals():
    """[(name, file bytes, edition, var, read keywords, a word the reason must hold)]: everything `grib.py` refuses."""
    rng = np.random.default_rng(7)
    st = lambda k=0, **kw: field(rng, 12, k, **kw)
    out = [
        ("e1_gaussian", message1(st(), GRID, gds_type=4), 1, "t2m", {}, "Gaussian"),
        ("e2_gaussian", message2(st(), GRID, grid_template=40), 2, "t2m", {}, "Gaussian"),
        ("e1_second_order", message1(st(), GRID, bds_flags=0x4), 1, "t2m", {}, "second-order"),
        ("e1_spherical", message1(st(), GRID, bds_flags=0x8), 1, "t2m", {}, "spherical"),
        ("e2_jpeg2000", message2(st(), GRID, drt=40), 2, "t2m", {}, "5.40"),
        ("e2_png", message2(st(), GRID, drt=41), 2, "t2m", {}, "5.41"),
        ("e2_ccsds", message2(st(), GRID, drt=42), 2, "t2m", {}, "5.42"),
        ("e2_complex", message2(st(), GRID, drt=3), 2, "t2m", {}, "5.3"),
        ("e1_minus_i", message1(st(), GRID[:6] + (0x80,)), 1, "t2m", {}, "-i"),
        ("e2_minus_i", message2(st(), GRID[:6] + (0x80,)), 2, "t2m", {}, "-i"),
        ("e1_column_major", message1(st(), GRID[:6] + (0x20,)), 1, "t2m", {}, "j-consecutive"),
        ("e2_alternating", message2(st(), GRID[:6] + (0x10,)), 2, "t2m", {}, "alternating"),
        ("e1_predefined_bitmap", message1(st(), GRID, predefined_bitmap=5), 1, "t2m", {}, "predefined bitmap"),
        ("e2_predefined_bitmap", message2(st(), GRID, bitmap_indicator=1), 2, "t2m", {}, "predefined bitmap"),
        ("e2_bitmap_254", message2(st(), GRID, bitmap_indicator=254), 2, "t2m", {}, "254"),
        ("e1_no_gds", message1(st(), GRID, gds=False), 1, "t2m", {}, "grid description"),
        ("e2_several_fields", message2(st(), GRID, fields=[(st(), {})]), 2, "t2m", {}, "several fields"),
        ("e1_two_levels", message1(st(0), GRID, param=130, level_type=100, level=850) + message1(st(0), GRID, param=130, level_type=100, level=500),
         1, "t", {}, "levels"),
        ("e1_duplicate_times", message1(st(0), GRID) + message1(st(1), GRID) + message1(st(1), GRID), 1, "t2m", {}, "valid time"),
        ("e1_truncated", message1(st(0), GRID) + message1(st(1), GRID)[:-9], 1, "t2m", {}, "7777"),
        ("e2_truncated", message2(st(0), GRID) + message2(st(1), GRID)[:-1], 2, "t2m", {}, "7777"),
        ("e1_two_grids", message1(st(0), GRID) + message1(st(1), GRID[:2] + (40.0,) + GRID[3:]), 1, "t2m", {}, "grid"),
        ("e1_time_range_7", message1(st(), GRID, tri=7), 1, "t2m", {}, "time range indicator 7"),
        ("e1_unit_month", message1(st(), GRID, unit=3), 1, "t2m", {}, "unit of time range 3"),
        ("e2_template_4_1", message2(st(), GRID, template=1), 2, "t2m", {}, "4.1"),
    ]
    big = bytearray(message1(st(), GRID))
    big[4] |= 0x80                                                        # ECMWF's large-message extension: bit 23 of the length
    out.append(("e1_large_message", bytes(big), 1, "t2m", {}, "bit 23"))
    return out
