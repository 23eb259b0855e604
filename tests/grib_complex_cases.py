"""A catalogue of edition-2 GRIB files in complex packing (data representation templates 5.2 and 5.3) for tests/test_grib_complex.py and
tests/test_gpu_grib_complex.py, with its own writer: its own bit packer and group builder, independent of aggfly_amd/grib.py.  A
field is given as the integers X it must decode to (signed Python integers, the present points in scan order) and the lengths of its
groups; the writer differences X, subtracts the smallest difference, gives every group its reference and width, and packs the
tables and the values through one Python big integer each.  The expected array is ``float32(((X * s) + R) * d)`` from X alone, NaN
where the bitmap has 0: nothing here decodes.  Sections 0 - 4 and 6 come from tests/grib_cases.py (`message2`); sections 5 and 7 are
replaced by the ones written here.

    section 5   len(4) 5 N(4) template(2) R(4) E(2) D(2) nbits_ref type split mvm sub1(4) sub2(4) NG(4) ref_width nbits_width
                ref_len(4) len_inc last_len(4) nbits_len [order extra]                                   47 bytes (5.2) / 49 (5.3)
    section 7   len(4) 7 [ival1 [ival2] minsd] refs | widths | lengths | values          (each table padded to an octet boundary)
"""
import datetime as dt
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_cases as C  # noqa: E402

u, sm, pack_bits = C.u, C.sm, C.pack_bits
BASE, GRID, NI, NJ = C.BASE, C.GRID, C.NI, C.NJ
NP = NI * NJ


def pack_fields(values, widths) -> tuple:
    """(bytes, bit count) of ``values[i]`` as a ``widths[i]``-bit big-endian integer each, back to back; zero bits pad the last byte."""
    big, n = 0, 0
    for v, w in zip(values, widths):
        assert 0 <= int(v) < (1 << w) or (w == 0 and int(v) == 0), (v, w)
        big = (big << w) | int(v)
        n += w
    pad = -n % 8
    return (big << pad).to_bytes((n + pad) // 8, "big"), n


def pack_fields_np(values, widths) -> tuple:
    """`pack_fields` for fields of half a million values, where one big integer is too slow: every bit is set in an array of bits by
    its position (the field's first bit + width - 1 - j for bit j of the value), and numpy packs them most significant bit first."""
    v, w = np.asarray(values, dtype=np.uint64), np.asarray(widths, dtype=np.int64)
    assert ((v >> w.astype(np.uint64).clip(0, 63)) == 0).all() and (w <= 32).all()
    first = np.cumsum(w) - w
    n = int(w.sum())
    bits = np.zeros(n + (-n % 8), dtype=np.uint8)
    for j in range(int(w.max()) if len(w) else 0):
        has = w > j
        bits[(first + w - 1 - j)[has]] = ((v[has] >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits).tobytes(), n


class CStep:
    """One field in complex packing as written.  ``X``: the integers of the present points; ``lens``: the group lengths (their sum is
    len(X); an empty list writes NG = 0, and X must then be all 0).  ``template`` 2 / 3, ``order`` 1 / 2 and ``extra`` (octets of
    ival1 / ival2 / minsd; with 0 they are absent and X must begin with 0 [, 0] and have no negative difference).  Knobs, all
    optional: ``min_width`` (bits every group gets at least, one number or one per group), ``zero_refs`` (all references 0, so
    ``nbits_ref`` may be 0), ``nbits_ref`` / ``nbits_width`` / ``nbits_len`` / ``ref_width`` (wider tables, a lower base), ``ref_len``
    and ``len_inc`` (every length but the last must be ref_len + len_inc * k), ``last_stored`` (what the length table holds for the last
    group: anything, the true length is in section 5), ``placeholders`` (raw[0], raw[1] under 5.3: ignored by a reader), ``minsd`` (a
    smaller minimum than the true one), ``sec5`` (octet overrides {octet number: byte}) and ``cut7`` (bytes cut off section 7)."""

    def __init__(self, X, lens, template=3, order=2, extra=2, E=0, D=0, R=0.0, bitmap=None, valid=BASE, min_width=0, zero_refs=False,
                 nbits_ref=None, nbits_width=None, nbits_len=None, ref_width=None, ref_len=None, len_inc=1, last_stored=None,
                 placeholders=(0, 0), minsd=None, sec5=None, cut7=0, last_len=None, n_values=None):
        self.X, self.lens, self.template, self.order, self.extra = [int(x) for x in X], [int(v) for v in lens], template, order if template == 3 else 0, extra
        self.E, self.D, self.R, self.bitmap, self.valid = E, D, float(R), bitmap, valid
        self.knobs = dict(min_width=min_width, zero_refs=zero_refs, nbits_ref=nbits_ref, nbits_width=nbits_width, nbits_len=nbits_len,
                          ref_width=ref_width, ref_len=ref_len, len_inc=len_inc, last_stored=last_stored, placeholders=placeholders,
                          minsd=minsd, sec5=sec5 or {}, cut7=cut7, last_len=last_len, n_values=n_values)
        self.nbits = 0                                                    # (what tests/grib_cases.py asks of a step)
        self._build()

    # ---- the closed formula ----
    def expected(self, nj, ni) -> np.ndarray:
        s, d = 2.0 ** self.E, 10.0 ** -self.D
        if len(self.X) > 10000:                                           # (the same formula on an array; |X| < 2^53 there)
            assert max(abs(x) for x in self.X) < (1 << 53)
            vals = (((np.array(self.X, dtype=np.int64).astype(np.float64) * s) + self.R) * d).astype(np.float32)
        else:
            vals = np.array([np.float32(((float(x) * s) + self.R) * d) for x in self.X], dtype=np.float32)
        if self.bitmap is not None:
            out = np.full(len(self.bitmap), np.nan, dtype=np.float32)
            out[np.array(self.bitmap, dtype=bool)] = vals
            vals = out
        return vals.reshape(nj, ni)

    # ---- the writer ----
    def _build(self):
        X, k, N = self.X, self.knobs, len(self.X)
        order = self.order
        self.ival, self.minsd = [0, 0], 0
        if not self.lens:                                                 # NG = 0: a constant field of X = 0, no tables and no values
            assert not any(X)
            raw = []
        elif order == 0:
            raw = list(X)
        else:
            if order == 1:
                diff = [X[n] - X[n - 1] for n in range(1, N)]
            else:
                diff = [X[n] - 2 * X[n - 1] + X[n - 2] for n in range(2, N)]
            self.ival = [X[0] if N else 0, X[1] if order == 2 and N > 1 else 0]
            self.minsd = (min(diff) if diff else 0) if k["minsd"] is None else k["minsd"]
            if self.extra == 0:
                assert self.ival == [0, 0] and (not diff or min(diff) >= 0), "extra = 0: ival1 = ival2 = minsd = 0"
                self.minsd = 0
            assert not diff or self.minsd <= min(diff)
            raw = (list(k["placeholders"][:order]) + [v - self.minsd for v in diff])[:N]
        assert all(v >= 0 for v in raw)
        self.raw = raw
        # groups: reference = the smallest member (or 0), width = the bits of the largest remainder (or more)
        assert sum(self.lens) == N or not self.lens
        NG = len(self.lens)
        mw = k["min_width"] if isinstance(k["min_width"], (list, tuple)) else [k["min_width"]] * NG
        refs, widths, fields, p = [], [], [], 0
        for g, ln in enumerate(self.lens):
            members = raw[p:p + ln]
            p += ln
            ref = 0 if k["zero_refs"] or not members else min(members)
            refs.append(ref)
            widths.append(max(mw[g], max([(v - ref).bit_length() for v in members], default=0)))
            fields += [(v - ref, widths[-1]) for v in members]
        assert all(w <= 32 for w in widths) or k["sec5"] or k["min_width"], widths
        self.refs, self.widths = refs, widths
        need_ref = max([r.bit_length() for r in refs], default=0)
        self.nbits_ref = need_ref if k["nbits_ref"] is None else k["nbits_ref"]
        self.ref_width = (min(widths) if widths else 0) if k["ref_width"] is None else k["ref_width"]
        need_w = max([(w - self.ref_width).bit_length() for w in widths], default=0)
        self.nbits_width = need_w if k["nbits_width"] is None else k["nbits_width"]
        self.len_inc = k["len_inc"]
        body_lens = self.lens[:-1]
        self.ref_len = (min(body_lens) if body_lens else (self.lens[-1] if self.lens else 0)) if k["ref_len"] is None else k["ref_len"]
        stored = []
        for ln in body_lens:
            q, r = divmod(ln - self.ref_len, self.len_inc) if self.len_inc else (0, ln - self.ref_len)
            assert r == 0 and q >= 0, (ln, self.ref_len, self.len_inc)
            stored.append(q)
        if self.lens:
            q, r = divmod(self.lens[-1] - self.ref_len, self.len_inc) if self.len_inc else (0, 1)
            stored.append((q if r == 0 and q >= 0 else 0) if k["last_stored"] is None else k["last_stored"])
        need_l = max([v.bit_length() for v in stored], default=0)
        self.nbits_len = need_l if k["nbits_len"] is None else k["nbits_len"]
        self.last_len = (self.lens[-1] if self.lens else 0) if k["last_len"] is None else k["last_len"]
        assert self.nbits_ref >= need_ref and self.nbits_width >= need_w and self.nbits_len >= need_l
        body = b""
        if self.template == 3 and self.extra:
            body += b"".join(sm(v, self.extra) for v in self.ival[:order] + [self.minsd])
        table = pack_bits if NG <= 10000 else (lambda vals, nb: pack_fields_np(vals, [nb] * len(vals)))
        body += table(refs, self.nbits_ref)[0] + table([w - self.ref_width for w in widths], self.nbits_width)[0]
        body += table(stored, self.nbits_len)[0]
        values, self.value_bits = (pack_fields_np if len(fields) > 10000 else pack_fields)([f for f, _ in fields], [w for _, w in fields])
        self.body = body + values
        self.table_bytes = len(body)

    def section5(self) -> bytes:
        N = len(self.X) if self.knobs["n_values"] is None else self.knobs["n_values"]
        s5 = (u(49 if self.template == 3 else 47, 4) + u(5, 1) + u(N, 4) + u(self.template, 2) + np.array(self.R, dtype=">f4").tobytes()
              + sm(self.E, 2) + sm(self.D, 2) + u(self.nbits_ref, 1) + u(0, 1) + u(1, 1) + u(0, 1) + u(0, 4) + u(0, 4) + u(len(self.lens), 4)
              + u(self.ref_width, 1) + u(self.nbits_width, 1) + u(self.ref_len, 4) + u(self.len_inc, 1) + u(self.last_len, 4) + u(self.nbits_len, 1))
        if self.template == 3:
            s5 += u(self.order, 1) + u(self.extra, 1)
        s5 = bytearray(s5)
        for octet, byte in self.knobs["sec5"].items():
            s5[octet - 1] = byte
        return bytes(s5)

    def section7(self) -> bytes:
        body = self.body[:len(self.body) - self.knobs["cut7"]]
        return u(5 + len(body), 4) + u(7, 1) + body


def message(step, grid=GRID, **kw) -> bytes:
    """An edition-2 message of the complex-packed ``step``: `grib_cases.message2` of a stand-in with sections 5 and 7 replaced."""
    stand_in = C.Step([0] * len(step.X), 0, step.E, step.D, step.R, step.bitmap, step.valid)
    raw = C.message2(stand_in, grid, **kw)
    pos, out = 16, []
    while raw[pos:pos + 4] != b"7777":
        n, num = int.from_bytes(raw[pos:pos + 4], "big"), raw[pos + 4]
        out.append(step.section5() if num == 5 else step.section7() if num == 7 else raw[pos:pos + n])
        pos += n
    assert pos + 4 == len(raw)
    body = b"".join(out) + b"7777"
    return raw[:8] + u(16 + len(body), 8) + body


# ---------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------
def smooth(rng, n, lo=-400, hi=400, step=9):
    """A random walk of ``n`` integers inside [lo, hi]: small first and second differences, as a smooth field has."""
    x, out = int(rng.integers(lo, hi)), []
    for _ in range(n):
        x = min(hi, max(lo, x + int(rng.integers(-step, step + 1))))
        out.append(x)
    return out


def cut(rng, n, mean=6):
    """Random group lengths that sum to ``n``."""
    lens, total = [], 0
    while total < n:
        lens.append(min(n - total, int(rng.integers(1, 2 * mean))))
        total += lens[-1]
    return lens


def hours(k):
    return BASE + dt.timedelta(hours=k)


def build_cases():
    rng = np.random.default_rng(20240802)
    cases = []

    def add(name, steps, pieces=None):
        cases.append(C.Case(name, "t2m", pieces if pieces is not None else [message(s) if isinstance(s, CStep) else C.message2(s, GRID) for s in steps],
                            sorted(steps, key=lambda s: s.valid), edition=2))

    # the three forms, E / D / R differing from message to message
    EDR = [(-3, 0, 100.0), (0, 1, -118.625), (2, -1, 1.0), (-10, 2, 273.125)]
    for tag, tmpl, order in (("c2", 2, 0), ("c3_order1", 3, 1), ("c3_order2", 3, 2)):
        steps = []
        for k, (E, D, R) in enumerate(EDR):
            X = smooth(rng, NP, 0 if tmpl == 2 else -400)
            steps.append(CStep(X, cut(rng, NP), tmpl, order, extra=2, E=E, D=D, R=R, valid=hours(k)))
        add(tag, steps)
    # the octets of the extra descriptors: 0 (ival1 = ival2 = minsd = 0: X begins with 0 and its differences are not negative), 1, 2, 4
    for order in (1, 2):
        steps = []
        for k, extra in enumerate((0, 1, 2, 4)):
            if extra == 0:
                inc = [int(v) for v in rng.integers(0, 5, size=NP)]
                inc[0] = 0
                if order == 2:
                    inc[1] = 0
                X = np.cumsum(inc).tolist() if order == 1 else np.cumsum(np.cumsum(inc)).tolist()
            else:
                top = {1: 100, 2: 30000, 4: 2_000_000_000}[extra]
                X = smooth(rng, NP, -top, top, step=min(top // 4, 50000))
                if X[0] >= 0:                                                # a negative ival1 (and minsd below zero: the walk goes both ways)
                    X = [-v - 1 for v in X]
            steps.append(CStep(X, cut(rng, NP), 3, order, extra=extra, E=-1, R=2.5, valid=hours(k)))
        assert any(s.minsd < 0 for s in steps) and any(s.ival[0] < 0 for s in steps)
        add(f"c3_order{order}_extra_0_1_2_4", steps)
    # widths 0, 1, 31 and 32 in one message: constant groups, a group of 0 / 1, and groups that hold 2^31 - 1 and 2^32 - 1
    lens = [5, 1, 7, 4, 9, 3, 6, 10]
    assert sum(lens) == NP
    X = [7] * 5 + [9] + [int(v) for v in rng.integers(0, 2, size=7)] + [3] * 4 + [int(v) for v in rng.integers(0, 1 << 31, size=9, dtype=np.int64)]
    X += [11] * 3 + [int(v) for v in rng.integers(0, 1 << 32, size=6, dtype=np.int64)] + [100 + int(v) for v in rng.integers(0, 1000, size=10)]
    X[7], X[8], X[17], X[18], X[29], X[30] = 0, 1, 0, (1 << 31) - 1, 0, (1 << 32) - 1
    st = CStep(X, lens, 2, E=-4, R=0.5, valid=hours(0))
    assert {0, 1, 31, 32} <= set(st.widths)
    add("c2_widths_0_1_31_32", [st])
    # the same under order 2 with wide raw values: a second difference of 32 bits
    X = smooth(rng, NP, -1000, 1000)
    X = X[:20] + [v + (1 << 31) - 50 for v in X[20:]]                    # a step: second differences of +A and -A, 2 A just below 2^32
    st = CStep(X, cut(rng, NP), 3, 2, extra=4, valid=hours(0))
    assert max(st.widths) == 32
    add("c3_order2_width_32", [st])
    # absent tables: every reference 0 (nbits_ref 0), every width the same (nbits_width 0), every length the same (nbits_len 0)
    steps = [CStep(smooth(rng, NP), cut(rng, NP), 3, 1, extra=2, zero_refs=True, minsd=-9, valid=hours(0)),
             CStep(smooth(rng, NP), cut(rng, NP), 3, 2, extra=2, min_width=7, valid=hours(1)),
             CStep(smooth(rng, NP), [6] * 7 + [3], 3, 2, extra=2, valid=hours(2)),
             CStep([5] * NP, [NP], 2, valid=hours(3))]                                                  # all three absent: a constant group
    assert steps[0].nbits_ref == 0 and steps[1].nbits_width == 0 and steps[2].nbits_len == 0
    assert (steps[3].nbits_ref, steps[3].nbits_width, steps[3].nbits_len, steps[3].widths) == (3, 0, 0, [0])
    add("c3_absent_tables", steps)
    # lengths in steps of 3 from 2 on, a wrong stored length for the last group, wider tables than needed, a lower width base
    lens = [2, 5, 8, 2, 11, 5, 8, 4]
    steps = [CStep(smooth(rng, NP), lens, 3, 2, extra=2, ref_len=2, len_inc=3, last_stored=3, valid=hours(0)),
             CStep(smooth(rng, NP), lens, 3, 1, extra=2, ref_len=2, len_inc=3, last_stored=1, nbits_ref=13, nbits_width=5, nbits_len=9, ref_width=0, valid=hours(1)),
             CStep(smooth(rng, NP, 0), lens, 2, ref_len=2, len_inc=3, last_stored=2, min_width=3, ref_width=1, valid=hours(2))]
    assert steps[0].len_inc == 3 and steps[0].ref_len == 2 and steps[0].nbits_len == 2
    add("c3_len_inc_3_wrong_last_length", steps)
    # NG = 1, NG = N (groups of length 1), NG = 0 (5.2, 5.3 without and with extra descriptors: every X is 0 whatever they hold)
    steps = [CStep(smooth(rng, NP), [NP], 3, 2, extra=2, valid=hours(0)), CStep(smooth(rng, NP), [1] * NP, 3, 2, extra=2, valid=hours(1)),
             CStep(smooth(rng, NP, 0), [1] * NP, 2, valid=hours(2)), CStep([0] * NP, [], 2, R=3.25, valid=hours(3)),
             CStep([0] * NP, [], 3, 2, extra=0, R=-1.5, valid=hours(4)), CStep([0] * NP, [], 3, 1, extra=2, R=7.0, valid=hours(5))]
    add("c3_ng_1_n_0", steps)
    # nonzero placeholders in raw[0] and raw[1]
    steps = [CStep(smooth(rng, NP), cut(rng, NP), 3, 2, extra=2, placeholders=(77, 5), valid=hours(0)),
             CStep(smooth(rng, NP), cut(rng, NP), 3, 1, extra=2, placeholders=(1234,), valid=hours(1))]
    assert steps[0].raw[:2] == [77, 5] and steps[1].raw[0] == 1234
    add("c3_placeholders", steps)
    # a bitmap: the packed values are the present points
    steps = []
    for k, (tmpl, order) in enumerate(((2, 0), (3, 1), (3, 2), (3, 2))):
        bm = C.some_bitmap(rng) if k < 3 else [0] * NP                  # (the last one has no present point: N = 0, NG = 0)
        n = sum(bm)
        steps.append(CStep(smooth(rng, n, 0 if tmpl == 2 else -400), cut(rng, n), tmpl, order, extra=2, E=-2, R=10.0, bitmap=bm, valid=hours(k)))
    add("c3_bitmap", steps)
    # a file that mixes simple packing (5.0: a writer's fallback for a constant field, and a 12-bit one) with 5.3 and 5.2
    steps = [CStep(smooth(rng, NP), cut(rng, NP), 3, 2, extra=2, R=1.0, valid=hours(0)), C.field(rng, 0, 1, R=280.5), C.field(rng, 12, 2),
             CStep(smooth(rng, NP, 0), cut(rng, NP), 2, valid=hours(3)), CStep(smooth(rng, NP, -100, 100), cut(rng, NP), 3, 1, extra=1, minsd=-20, valid=hours(4)),
             CStep(smooth(rng, NP), cut(rng, NP), 3, 2, extra=2, valid=hours(5)), C.field(rng, 16, 6, bitmap=C.some_bitmap(rng))]
    add("c3_mixed_with_simple", steps)
    # messages out of time order, a second parameter (simple packing) in between
    a = [CStep(smooth(rng, NP), cut(rng, NP), 3, 2, extra=2, E=-1, valid=hours(k)) for k in range(5)]
    pieces = []
    for k in (3, 0, 4, 1, 2):
        pieces += [message(a[k]), C.message2(C.field(rng, 12, k), GRID, param=(0, 0, 6))]
    add("c3_shuffled", a, pieces)
    return cases


def refusals():
    """[(name, file bytes, a word the reason must hold, raised on read rather than on indexing)]: what `grib.py` refuses of 5.2 / 5.3."""
    rng = np.random.default_rng(9)
    mk = lambda **kw: CStep(smooth(rng, NP), kw.pop("lens", None) or cut(rng, NP), 3, kw.pop("order", 2), extra=kw.pop("extra", 2), **kw)
    wide = CStep(smooth(rng, NP), cut(rng, NP), 3, 2, extra=2, min_width=33)
    out = [
        ("missing_value_management_1", message(mk(sec5={23: 1})), "missing value management 1", False),
        ("missing_value_management_2", message(mk(sec5={23: 2})), "missing value management 2", False),
        ("order_0", message(mk(sec5={48: 0})), "order 0", False),
        ("order_3", message(mk(sec5={48: 3})), "order 3", False),
        ("extra_5", message(mk(sec5={49: 5})), "5 octets", False),
        ("width_33", message(wide), "33 bits", True),
        ("lengths_do_not_sum", message(mk(lens=[9] * 5, last_len=8)), "sum to 44", True),
        ("section_7_too_short", message(mk(cut7=2)), "too short", True),
        ("tables_too_short", message(mk(cut7=10 ** 6)), "too short", True),
        ("n_values_not_the_grid", message(mk(n_values=NP - 1)), "packed values", False),
        ("short_section_5_2", C.message2(C.field(rng, 12, 0), GRID, drt=2), "5.2", False),
        ("short_section_5_3", C.message2(C.field(rng, 12, 0), GRID, drt=3), "5.3", False),
        ("ieee", C.message2(C.field(rng, 12, 0), GRID, drt=4), "5.4", False),
        ("jpeg2000", C.message2(C.field(rng, 12, 0), GRID, drt=40), "5.40", False),
        ("png", C.message2(C.field(rng, 12, 0), GRID, drt=41), "5.41", False),
        ("ccsds", C.message2(C.field(rng, 12, 0), GRID, drt=42), "5.42", False),
        ("spherical", C.message2(C.field(rng, 12, 0), GRID, drt=50), "5.50", False),
        ("spherical_complex", C.message2(C.field(rng, 12, 0), GRID, drt=51), "5.51", False),
        ("edition_1_second_order", C.message1(C.field(rng, 12, 0), GRID, bds_flags=0x4), "second-order", False),
    ]
    return out
