"""A catalogue of edition-2 GRIB files in CCSDS packing (data representation template 5.42) for tests/test_grib_ccsds.py and
tests/test_gpu_grib_ccsds.py, with a stream writer of its own: an encoder of CCSDS 121.0-B adaptive entropy coding written from the
encoder's side of the standard (the forward predictor and mapper, the code options), independent of aggfly_amd/csrc/aec_passes.h and of
aggfly_amd/grib.py: nothing here decodes.  The option of every block can be forced (`encode(..., choose=...)`), so tests can write what
an encoder would not choose; left alone, the writer takes the shortest option like any encoder.  `load_libaec` finds libaec through
ctypes (or reports it absent): the tests that hold the decoder to the real encoder use it, and `python tests/grib_ccsds_cases.py`
(no argument; with a file name it writes the streams of tests/aec_streams_check.c) wrote tests/golden/grib_ccsds_streams.json with it - every stream of that file, forced ones included, was decoded by libaec before it was
written.  Sections 0 - 4 and 6 come from tests/grib_cases.py (`message2`); sections 5 and 7 are replaced by the ones written here.

    section 5   len(4) 5 N(4) 42(2) R(4) E(2) D(2) nbits type flags J rsi(2)                                             25 bytes
    section 7   len(4) 7 stream
    block       ID(id_len) [0: one bit: 0 zero blocks / 1 second extension] [reference(n), first block of an RSI] payload
"""
import ctypes
import ctypes.util
import datetime as dt
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grib_cases as C  # noqa: E402

u, sm = C.u, C.sm
BASE, GRID, NI, NJ = C.BASE, C.GRID, C.NI, C.NJ
NP = NI * NJ
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grib_ccsds_streams.json")
PREPROCESS = 8


def id_len(n: int) -> int:
    return 3 if n <= 8 else 4 if n <= 16 else 5


# ---------------------------------------------------------------------------------------
# the stream writer
# ---------------------------------------------------------------------------------------
def fs(v: int) -> str:
    return "0" * v + "1"


def bits(v: int, w: int) -> str:
    assert 0 <= v < (1 << w) or (w == 0 and v == 0), (v, w)
    return format(v, f"0{w}b") if w else ""


def map_deltas(x, n):
    """The mapped prediction errors of the samples ``x`` after their first (CCSDS 121.0-B 4.2: unit-delay predictor, then the mapper):
    with D = x[i] - x[i-1] and theta = min(x[i-1], xmax - x[i-1]): 2 D for 0 <= D <= theta, 2 |D| - 1 for -theta <= D < 0, else theta + |D|."""
    xmax, out = (1 << n) - 1, []
    for prev, cur in zip(x, x[1:]):
        D, theta = cur - prev, min(prev, xmax - prev)
        out.append(2 * D if 0 <= D <= theta else 2 * -D - 1 if -theta <= D < 0 else theta + abs(D))
    return out


def se_codes(deltas):
    """The second-extension codes of an even number of deltas, or None when one exceeds libaec's bound of 90."""
    out = []
    for a, b in zip(deltas[0::2], deltas[1::2]):
        m = (a + b) * (a + b + 1) // 2 + b
        if m > 90:
            return None
        out.append(m)
    return out


def shortest(deltas, first, n, J):
    """What an encoder takes for a block that is not all zero: the shortest of uncompressed, every k-split and second extension."""
    best, size = ("unc",), J * n
    for k in range((1 << id_len(n)) - 2):
        sz = sum((d >> k) + 1 + k for d in deltas)
        if sz < size:
            best, size = ("k", k), sz
    codes = se_codes(([0] if first else []) + deltas)
    if codes is not None and 1 + sum(m + 1 for m in codes) < size:
        best = ("se",)
    return best


def encode(X, n, J, rsi, pp=True, choose=None) -> bytes:
    """The AEC stream of the samples ``X`` (``n`` bits each).  ``choose(ri, b, deltas, first)`` may return the option of block ``b`` of RSI
    ``ri`` — ("unc",), ("k", k), ("se",), ("zero", z) for a run of z zero blocks written with its own count, ("ros",) for the
    "remainder of segment" code — or None for the shortest one.  A zero run may pass the last sample, never the RSI's last block."""
    X = [int(v) for v in X]
    assert X and all(0 <= v < (1 << n) for v in X)
    idl, per = id_len(n), rsi * J
    out = []
    for ri, s0 in enumerate(range(0, len(X), per)):
        x = X[s0:s0 + per]
        x += [x[-1]] * (-len(x) % J)                                          # the last block is padded with its last sample
        d = ([None] + map_deltas(x, n)) if pp else list(x)                    # (None: the reference stands there)
        nb = len(x) // J
        blocks = [[v for v in d[b * J:(b + 1) * J] if v is not None] for b in range(nb)]
        b = 0
        while b < nb:
            first = pp and b == 0
            ref = bits(x[0], n) if first else ""
            seg_end = min(rsi - b, 64 - b % 64)                               # blocks to the end of the segment
            opt = choose(ri, b, blocks[b], first) if choose else None
            if opt is None:
                if any(blocks[b]):
                    opt = shortest(blocks[b], first, n, J)
                else:
                    z = 1
                    while z < seg_end and b + z < nb and not any(blocks[b + z]):
                        z += 1
                    opt = ("ros",) if z == seg_end and z >= 5 else ("zero", z)
            if opt[0] in ("zero", "ros"):
                z = seg_end if opt[0] == "ros" else opt[1]
                assert 1 <= z <= rsi - b and not any(any(blk) for blk in blocks[b:b + z]), (ri, b, opt)
                v = 4 if opt[0] == "ros" else z - 1 if z <= 4 else z
                out += [bits(0, idl), "0", ref, fs(v)]
                b += z
                continue
            if opt[0] == "unc":
                out += [bits((1 << idl) - 1, idl), ref] + [bits(v, n) for v in blocks[b]]      # (the reference is the block's first field)
            elif opt[0] == "k":
                k = opt[1]
                assert 0 <= k <= (1 << idl) - 3
                out += [bits(k + 1, idl), ref] + [fs(v >> k) for v in blocks[b]] + [bits(v & ((1 << k) - 1), k) for v in blocks[b]]
            elif opt[0] == "se":
                codes = se_codes(([0] if first else []) + blocks[b])
                assert codes is not None, (ri, b, "second extension needs codes <= 90")
                out += [bits(0, idl), "1", ref] + [fs(m) for m in codes]
            else:
                raise KeyError(opt)
            b += 1
    s = "".join(out)
    s += "0" * (-len(s) % 8)
    return int(s, 2).to_bytes(len(s) // 8, "big")


# ---------------------------------------------------------------------------------------
# libaec through ctypes
# ---------------------------------------------------------------------------------------
class _AecStream(ctypes.Structure):
    _fields_ = [("next_in", ctypes.c_void_p), ("avail_in", ctypes.c_size_t), ("total_in", ctypes.c_size_t), ("next_out", ctypes.c_void_p),
                ("avail_out", ctypes.c_size_t), ("total_out", ctypes.c_size_t), ("bits_per_sample", ctypes.c_uint), ("block_size", ctypes.c_uint),
                ("rsi", ctypes.c_uint), ("flags", ctypes.c_uint), ("state", ctypes.c_void_p)]


_LIBAEC = []


def load_libaec():
    """libaec as a ctypes library, or None when this machine has none."""
    if not _LIBAEC:
        lib = None
        # $AGGFLY_LIBAEC, the loader's own search, then the lib directories of this interpreter and of a conda installation
        names = [os.environ.get("AGGFLY_LIBAEC"), ctypes.util.find_library("aec"), "libaec.so.0", "libaec.so"]
        prefixes = [sys.prefix, sys.base_prefix, os.environ.get("CONDA_PREFIX"), "/opt/conda", os.path.expanduser("~/miniconda3"), "/usr/local"]
        names += [os.path.join(p, "lib", "libaec.so.0") for p in prefixes if p]
        for name in names:
            try:
                lib = ctypes.CDLL(name) if name else None
            except OSError:
                lib = None
            if lib is not None and hasattr(lib, "aec_buffer_decode"):
                break
            lib = None
        _LIBAEC.append(lib)
    return _LIBAEC[0]


def _sample_dtype(n):
    return np.uint8 if n <= 8 else np.uint16 if n <= 16 else np.uint32


def libaec_encode(X, n, J, rsi, flags=PREPROCESS) -> bytes:
    lib = load_libaec()
    a = np.ascontiguousarray(np.asarray(X).astype(_sample_dtype(n)))
    out = np.zeros(a.nbytes * 2 + 4096, dtype=np.uint8)
    s = _AecStream()
    s.next_in, s.avail_in, s.next_out, s.avail_out = a.ctypes.data, a.nbytes, out.ctypes.data, out.nbytes
    s.bits_per_sample, s.block_size, s.rsi, s.flags = n, J, rsi, flags
    rc = lib.aec_buffer_encode(ctypes.byref(s))
    assert rc == 0, rc
    return out[:s.total_out].tobytes()


def libaec_decode(data: bytes, count, n, J, rsi, flags=PREPROCESS):
    """The ``count`` samples libaec reads from ``data`` (uint64), or None where it reports an error or stops short."""
    lib = load_libaec()
    src = np.frombuffer(bytes(data), dtype=np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    out = np.zeros(count, dtype=_sample_dtype(n))
    s = _AecStream()
    s.next_in, s.avail_in, s.next_out, s.avail_out = src.ctypes.data, len(data), out.ctypes.data, out.nbytes
    s.bits_per_sample, s.block_size, s.rsi, s.flags = n, J, rsi, flags
    rc = lib.aec_buffer_decode(ctypes.byref(s))
    if rc != 0 or s.total_out != out.nbytes:
        return None
    return out.astype(np.uint64)


# ---------------------------------------------------------------------------------------
# one field and its message
# ---------------------------------------------------------------------------------------
class AStep:
    """One field in CCSDS packing as written.  ``X``: the integers of the present points; ``nbits``, ``J`` = block size, ``rsi``, ``flags``
    (octet 22 of section 5; bit 8 says whether the stream is written with the preprocessor).  ``stream``: the body of section 7 (default:
    `encode` with ``choose``; pass libaec's bytes to write those).  Knobs: ``sec5`` (octet overrides {octet number: byte}), ``cut7`` (bytes
    cut off section 7), ``n_values`` (what section 5 announces instead of len(X))."""

    def __init__(self, X, nbits, J=32, rsi=128, flags=PREPROCESS | 4 | 2, E=0, D=0, R=0.0, bitmap=None, valid=BASE, choose=None, stream=None,
                 sec5=None, cut7=0, n_values=None):
        self.X, self.nbits, self.J, self.rsi, self.flags = [int(x) for x in X], nbits, J, rsi, flags
        self.E, self.D, self.R, self.bitmap, self.valid = E, D, float(R), bitmap, valid
        self.sec5, self.cut7, self.n_values = sec5 or {}, cut7, len(self.X) if n_values is None else n_values
        if stream is None:
            stream = encode(self.X, nbits, J, rsi, bool(flags & PREPROCESS), choose) if nbits and self.X else b""
        self.body = bytes(stream)

    def expected(self, nj, ni) -> np.ndarray:
        s, d = 2.0 ** self.E, 10.0 ** -self.D
        vals = (((np.array(self.X, dtype=np.uint64).astype(np.float64) * s) + self.R) * d).astype(np.float32)
        if self.bitmap is not None:
            out = np.full(len(self.bitmap), np.nan, dtype=np.float32)
            out[np.array(self.bitmap, dtype=bool)] = vals
            vals = out
        return vals.reshape(nj, ni)

    def section5(self) -> bytes:
        s5 = bytearray(u(25, 4) + u(5, 1) + u(self.n_values, 4) + u(42, 2) + np.array(self.R, dtype=">f4").tobytes() + sm(self.E, 2) + sm(self.D, 2)
                       + u(self.nbits, 1) + u(0, 1) + u(self.flags, 1) + u(self.J, 1) + u(self.rsi, 2))
        for octet, byte in self.sec5.items():
            s5[octet - 1] = byte
        return bytes(s5)

    def section7(self) -> bytes:
        body = self.body[:len(self.body) - self.cut7]
        return u(5 + len(body), 4) + u(7, 1) + body


def message(step, grid=GRID, **kw) -> bytes:
    """An edition-2 message of the CCSDS-packed ``step``: `grib_cases.message2` of a stand-in with sections 5 and 7 replaced."""
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


def hours(k):
    return BASE + dt.timedelta(hours=k)


def smooth(rng, count, n, step=9, start=None):
    """A random walk of ``count`` ``n``-bit integers: small differences, as a smooth field has."""
    hi = (1 << n) - 1
    x = int(rng.integers(0, hi + 1)) if start is None else start
    w = np.cumsum(rng.integers(-step, step + 1, size=count)) + x
    return np.clip(w, 0, hi).astype(np.uint64).tolist()


def near_constant(rng, count, n, p=0.02):
    """A field that is one value but for a few points one above it: long runs of zero blocks."""
    base = int(rng.integers(0, (1 << n) - 1))
    return (base + (rng.random(count) < p)).astype(np.uint64).tolist()


# ---------------------------------------------------------------------------------------
# the golden streams
# ---------------------------------------------------------------------------------------
KNOWN = dict(n=8, J=8, rsi=2, pp=True, X=[int(v) for v in "100 101 103 103 102 250 0 7 7 7 7 7 7 7 7 7 7 7 7 7 7 7 7 7 7 7 9 8".split()],
             hex="ec804080003f5fe0e10079c2f8")


def golden_inputs():
    """[(name, writer, n, J, rsi, pp, X, choose)]: what tests/golden/grib_ccsds_streams.json holds; ``writer`` "libaec" or "forced"."""
    rng = np.random.default_rng(542)
    out = [("known_answer", "libaec", 8, 8, 2, True, KNOWN["X"], None)]
    for n in (1, 8, 12, 16, 24, 32):
        hi = (1 << n) - 1
        J = 8 if n <= 12 else 16
        out.append((f"smooth_n{n}", "libaec", n, J, 4, True, smooth(rng, 3 * J * 4 + 5, n, step=1 if n == 1 else 9), None))
        out.append((f"noisy_n{n}", "libaec", n, 8, 2, True, [int(v) for v in rng.integers(0, hi + 1, size=41, dtype=np.uint64)], None))
        # both branches of the inverse mapping near 0 and near xmax: jumps between the ends and small steps at them
        ends = [0, 1, 0, hi, hi - 1 if n > 1 else hi, hi, 0, hi, 1 if n > 1 else 0, 0, hi, hi, 0, 0, min(2, hi), hi, max(hi - 2, 0), hi, 0]
        out.append((f"ends_n{n}", "libaec", n, 8, 2, True, ends, None))
        for k in sorted({0, (1 << id_len(n)) - 3}):                          # k = 0 and the largest k of this id_len, also as a first block
            kk = min(k, n)
            X = [int(v) for v in (rng.integers(0, 1 << min(kk + 1, n), size=24, dtype=np.uint64))]
            if n > 1:
                X = [min(hi, (hi // 2) + v) for v in X]
            out.append((f"forced_k{k}_n{n}", "forced", n, 8, 3, True, X, ("k", k)))
    out.append(("x_above_2_31", "libaec", 32, 8, 2, True, [0x80000000 + int(v) for v in rng.integers(0, 1 << 30, size=19)] + [0xFFFFFFFF, 0x80000000], None))
    # every option as the first block of an RSI and elsewhere (rsi = 2: every other block is a first one)
    for opt in (("unc",), ("k", 0), ("k", 2), ("se",)):
        out.append((f"forced_{'_'.join(str(v) for v in opt)}_every_block", "forced", 8, 8, 2, True, [9, 9, 10, 9, 9, 8, 9, 9] * 4, opt))
    out.append(("forced_zero_first_and_later", "forced", 8, 8, 2, True, [7] * 32, ("zero", 1)))
    for J in (8, 16, 32, 64):
        out.append((f"lengths_J{J}_1", "libaec", 12, J, 2, True, smooth(rng, 1, 12), None))
        out.append((f"lengths_J{J}_minus_1", "libaec", 12, J, 2, True, smooth(rng, J - 1, 12), None))
        out.append((f"lengths_J{J}_plus_1", "libaec", 12, J, 2, True, smooth(rng, J + 1, 12), None))
        out.append((f"lengths_J{J}_rsi_plus_1", "libaec", 12, J, 2, True, smooth(rng, 2 * J + 1, 12), None))
    # zero runs of 1, 4, 6 and more; the segment-end code at b % 64 != 0 (rsi = 80: the second segment holds 16 blocks); a run past n_values
    def runs(lens, J=8):
        X = []
        for i, z in enumerate(lens):
            X += [40] * (z * J) + [41 + i % 3, 40, 39, 40, 40, 42, 40, 40]
        return X
    out.append(("zero_runs_1_4_6_9", "libaec", 8, 8, 80, True, [40, 41, 40, 40, 40, 40, 39, 40] + runs([1, 4, 6, 9]), None))
    out.append(("zero_run_to_segment_end", "libaec", 8, 8, 80, True, runs([3]) + [40] * (8 * 70), None))
    out.append(("zero_run_ros_mid_segment", "libaec", 8, 8, 20, True, runs([3, 2]) + [40] * (8 * 13) + runs([1]) + [40] * (8 * 5), None))
    out.append(("forced_ros_past_n_values", "forced", 8, 8, 16, True, runs([2]) + [40] * 11, lambda ri, b, d, first: ("ros",) if b == 3 else None))
    out.append(("forced_zero_count_past_n_values", "forced", 8, 8, 16, True, [40, 41, 40, 40, 40, 40, 39, 40] + [40] * 9,
                lambda ri, b, d, first: ("zero", 7) if b == 1 else None))
    out.append(("second_extension_72", "libaec", 12, 8, 16, True, [int(v) for v in (2000 + (rng.random(8 * 40) < 0.3))], None))
    out.append(("no_preprocessor", "libaec", 12, 8, 4, False, [int(v) for v in rng.integers(0, 60, size=77)], None))
    out.append(("no_preprocessor_zero_and_se", "forced", 8, 8, 4, False, [0] * 24 + [1, 0, 2, 1, 0, 0, 1, 3] + [0] * 17, None))
    # FS runs longer than 2,048 bits: k = 0 forced on jumps of 2,500 in 12 bits (deltas 2,600 and 3,995).  Noisy blocks follow: libaec's
    # fast path reads a run seven bytes at a time and gives up on one that ends within the stream's last six bytes
    out.append(("forced_long_fs", "forced", 12, 8, 2, True, [100] * 9 + [2600, 2600, 100, 100, 101, 100, 100]
                + [int(v) for v in rng.integers(0, 4096, size=45)], lambda ri, b, d, first: ("k", 0) if ri == 0 and any(d) else None))
    return out


def _choose_of(spec):
    if spec is None or callable(spec):
        return spec
    return lambda ri, b, deltas, first: spec


def write_golden(path=GOLDEN):
    """Write the fixture: needs libaec (every stream, forced ones included, is decoded by it first)."""
    assert load_libaec() is not None, "libaec is needed to write the fixture"
    rows = []
    for name, writer, n, J, rsi, pp, X, choose in golden_inputs():
        flags = PREPROCESS if pp else 0
        data = libaec_encode(X, n, J, rsi, flags) if writer == "libaec" else encode(X, n, J, rsi, pp, _choose_of(choose))
        back = libaec_decode(data, len(X), n, J, rsi, flags)
        assert back is not None and back.tolist() == [int(v) for v in X], name
        rows.append({"name": name, "writer": writer, "nbits": n, "block_size": J, "rsi": rsi, "preprocess": pp, "samples": [int(v) for v in X],
                     "hex": data.hex()})
    assert rows[0]["hex"] == KNOWN["hex"]
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    return rows


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------
# the catalogue of files
# ---------------------------------------------------------------------------------------
def build_cases():
    rng = np.random.default_rng(20241021)
    cases = []

    def add(name, steps, pieces=None, grid=GRID):
        cases.append(C.Case(name, "t2m", pieces if pieces is not None else [message(s, grid) for s in steps], steps, grid=grid, edition=2))

    R = float(np.float32(273.15))
    for n in (1, 8, 12, 16, 24, 32):
        add(f"a_n{n}", [AStep(smooth(rng, NP, n), n, J=8, rsi=2, E=-2 if n < 24 else -12, R=R, valid=hours(k)) for k in range(C.STEPS)])
    add("a_defaults", [AStep(smooth(rng, NP, 16), 16, E=-3, R=R, valid=hours(k)) for k in range(C.STEPS)])
    add("a_no_preprocessor", [AStep(smooth(rng, NP, 10, step=2, start=20), 10, J=16, rsi=1, flags=0, R=1.5, valid=hours(k)) for k in range(C.STEPS)])
    steps = []
    for k in range(C.STEPS):
        bm = C.some_bitmap(rng)
        steps.append(AStep(smooth(rng, sum(bm), 12), 12, J=8, rsi=3, E=-1, R=-118.625, bitmap=bm, valid=hours(k)))
    add("a_bitmap", steps)
    add("a_constant_and_nbits0", [AStep([77] * NP, 8, J=8, rsi=4, R=2.0, valid=hours(0)), AStep([0] * NP, 0, R=280.5, valid=hours(1)),
                                  AStep(near_constant(rng, NP, 16, 0.1), 16, J=8, rsi=128, E=-4, valid=hours(2)),
                                  AStep([0] * 20, 0, R=-3.25, bitmap=[1] * 20 + [0] * (NP - 20), valid=hours(3))])
    # the parameters change from step to step, and every block option is forced somewhere
    opts = [("unc",), ("k", 0), ("k", 3), ("se",), None, ("k", 5), None]
    Js, rsis, ns = (8, 16, 32, 64, 8, 16, 8), (1, 2, 128, 4096, 3, 1, 7), (8, 12, 16, 9, 24, 32, 5)
    steps = [AStep(smooth(rng, NP, ns[k], step=1), ns[k], J=Js[k], rsi=rsis[k], flags=PREPROCESS | (4 if k % 2 else 0), E=(-3, 0, 2, 0, -10, -4, 1)[k],
                   D=(0, 1, -1, 0, 2, 0, 0)[k], R=(100.0, -118.625, 1.0, 0.0, 273.125, -0.5, 4096.0)[k], valid=hours(k), choose=_choose_of(opts[k]))
             for k in range(C.STEPS)]
    add("a_varying_forced_options", steps)
    # out of time order, with simple- and complex-packed messages of another parameter between them
    a = [AStep(smooth(rng, NP, 16), 16, J=8, rsi=2, E=-2, R=R, valid=hours(k)) for k in range(C.STEPS)]
    pieces = []
    for j, k in enumerate([3, 0, 6, 1, 5, 2, 4]):
        pieces += [message(a[k])] + ([b"\x00\x00GRI\x00garbage"] if j % 2 else []) + [C.message2(C.field(rng, 12, k), GRID, param=(0, 0, 6))]
    add("a_shuffled", a, pieces)
    return cases


def refusals():
    """[(name, file bytes, a word the reason must hold, does it fail at the index (True) or at the read (False))]."""
    rng = np.random.default_rng(43)
    X = smooth(rng, NP, 12)
    out = []
    for bit, word in ((1, "signed"), (16, "restricted"), (32, "padded"), (64, "flag 64"), (128, "flag 128")):
        out.append((f"flag_{bit}", message(AStep(X, 12, J=8, rsi=2, flags=PREPROCESS | bit)), word, True))
    for J in (0, 4, 12, 128):
        out.append((f"block_size_{J}", message(AStep(X, 12, J=8, rsi=2, sec5={23: J})), "block size", True))
    for rsi in (0, 4097, 65535):
        out.append((f"rsi_{rsi}", message(AStep(X, 12, J=8, rsi=2, sec5={24: rsi >> 8, 25: rsi & 255})), "reference sample interval", True))
    out.append(("nbits_33", message(AStep(X, 12, J=8, rsi=2, sec5={20: 33})), "33 bits", True))
    out.append(("short_section_5", C.message2(C.field(rng, 12, 0), GRID, drt=42), "5.42", True))
    out.append(("more_values_than_points", message(AStep(X + [5], 12, J=8, rsi=2)), "packed values", True))
    out.append(("truncated_section_7", message(AStep(X, 12, J=8, rsi=2, cut7=3)), "section 7", False))
    out.append(("empty_section_7", message(AStep(X, 12, J=8, rsi=2, stream=b"")), "section 7", False))
    bm = C.some_bitmap(rng)
    out.append(("bitmap_disagrees", message(AStep(X[:sum(bm) - 1], 12, J=8, rsi=2, bitmap=bm)), "present grid points", False))
    return out


def write_check_file(path) -> int:
    """The streams of tests/aec_streams_check.c (its header has the format): the golden streams and the catalogue's as valid ones, then
    some 6,000 mutated ones - bits flipped, bytes replaced, streams truncated and extended."""
    import struct
    valid = [(bytes.fromhex(r["hex"]), r["samples"], r["nbits"], PREPROCESS if r["preprocess"] else 0, r["block_size"], r["rsi"]) for r in golden()]
    valid += [(s.body, s.X, s.nbits, s.flags, s.J, s.rsi) for c in build_cases() for s in c.steps if isinstance(s, AStep) and s.nbits]
    rng = np.random.default_rng(121)
    recs = [(0,) + v for v in valid]
    for data, X, n, flags, J, rsi in valid[::2]:
        for trial in range(90):
            b = bytearray(data)
            how = trial % 5
            if how == 0:
                for _ in range(int(rng.integers(1, 4))):
                    bit = int(rng.integers(0, len(b) * 8))
                    b[bit >> 3] ^= 0x80 >> (bit & 7)
            elif how == 1:
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
            elif how == 2:
                b = b[:int(rng.integers(0, len(b)))]
            elif how == 3:
                at = int(rng.integers(0, len(b)))
                b[at:at + int(rng.integers(1, 9))] = bytes(int(rng.integers(1, 9)) * [int(rng.choice([0, 255]))])
            else:
                b += bytes(rng.integers(0, 256, size=int(rng.integers(1, 5)), dtype=np.uint8))
            recs.append((2, bytes(b), X, n, flags, J, rsi))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)))
        for kind, data, X, n, flags, J, rsi in recs:
            f.write(struct.pack("<7I", kind, len(data), len(X), n, flags, J, rsi) + data)
            if kind == 0:
                f.write(np.asarray(X, dtype="<u4").tobytes())
    return len(recs)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        print("grib_ccsds_cases: wrote", write_check_file(sys.argv[1]), "streams to", sys.argv[1])
    else:
        print(len(write_golden()), "streams ->", GOLDEN)
