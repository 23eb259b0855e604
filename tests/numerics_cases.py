"""A catalogue of the arithmetic the numerics contract rests on — integer powers by the double-double chain (`powi_dd_vec`,
afhip_numerics.h; its written-out copy in the lean group end, afhip_kernels.h "leaf: x^n"), the Markstein quotient behind every mean (`div_by`)
and the element-wise transforms of `k_transform` (afhip_panel_kernels.h) — with the one reference all of it is held to: `fractions.Fraction`.
Host only, deterministic; shared by tests/test_numerics_host.py and tests/test_gpu_numerics.py.

Exact references.  `rn64` / `rn32` round a Fraction to the nearest double / float (ties to even, overflow to +-inf, a negative value that rounds
to zero to -0); `exact_power(x, e)` is `rn64(Fraction(x) ** e)` with np.power's specials; a mean is `rn64(Fraction(s) / n)`.  Hinge and product are
single IEEE operations, exact by definition: their expected values are the numpy expressions themselves.

Classes of a power case, decided from the exact value alone (never from the code under test):
    exact      e >= 0 and 2^-1022 <= |exact| < overflow, or a special (NaN, +-inf, +-0): bit equality, the sign of a zero included
    step       e >= 0 and 0 < |exact| < 2^-1022: |got - exact| <= 2^-1074 and the right sign (the chain's error terms cannot be held below 2^-1074)
    ulp        e <  0 and a normal result: |got - exact| <= 1 ulp of exact (two roundings of 2^-53 each: the power, then its reciprocal)
    ulp-step   e <  0 and a subnormal result: one subnormal step, as above
Classes of a mean case: `exact` where |s / n| >= 2^-1022 (and for s = 0), `step` below.

Emulations.  `emulate_powi` (the fused kernels' chain), `emulate_powi_scaled` (k_transform's) and `emulate_div_by` restate the device texts step by step with an exact `fma`
(`rn64(F(a) * F(b) + F(c))`, computed on integers), so the host test can prove the table's classes fair before a GPU sees them.
"""
from __future__ import annotations

import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

INF, NAN = math.inf, math.nan
STEP64 = 2.0 ** -1074
MIN_NORMAL64 = 2.0 ** -1022
MAX64 = float(np.finfo(np.float64).max)
EXPONENTS = tuple(range(-64, 65))                 # every exponent the host lowers to the chain (|e| <= 64; afhip_api.hip, afhip_planner.cpp)
MEAN_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 23, 24, 25, 28, 29, 30, 31, 48)


# ---------------------------------------------------------------------------------------
# exact rounding
# ---------------------------------------------------------------------------------------
def _rn_scaled(neg: bool, n: int, d: int, k: int, prec: int, qmin: int, emax: int) -> float:
    """The nearest value of the format (prec bits, smallest quantum 2^qmin, largest binade 2^emax) to (-1)^neg * (n / d) * 2^k, n >= 0, d > 0."""
    if n == 0:
        return -0.0 if neg else 0.0
    ex = n.bit_length() - d.bit_length() + k                      # 2^(ex - 1) < value < 2^(ex + 1)
    lhs, rhs = (n << max(0, k - ex)), (d << max(0, ex - k))       # value >= 2^ex  <=>  n 2^k >= d 2^ex
    e = ex if lhs >= rhs else ex - 1
    q = max(e - (prec - 1), qmin)
    s = k - q                                                     # mantissa = n 2^s / d, rounded half to even
    num, den = (n << s, d) if s >= 0 else (n, d << -s)
    m, r = divmod(num, den)
    if 2 * r > den or (2 * r == den and (m & 1)):
        m += 1
    if m.bit_length() + q - 1 > emax:
        return -INF if neg else INF
    v = math.ldexp(float(m), q)
    return -v if neg else v


def rn64(fr) -> float:
    """The correctly rounded double of a Fraction (or int): ties to even, overflow to +-inf, a negative value that rounds to zero to -0."""
    fr = Fraction(fr)
    return _rn_scaled(fr < 0, abs(fr.numerator), fr.denominator, 0, 53, -1074, 1023)


def rn32(fr) -> np.float32:
    """The correctly rounded float32 of a Fraction — rounded once, not through a double."""
    fr = Fraction(fr)
    return np.float32(_rn_scaled(fr < 0, abs(fr.numerator), fr.denominator, 0, 24, -149, 127))


def _parts(x: float):
    """finite x -> (negative, m, k) with |x| = m 2^k, m an integer below 2^53"""
    f, ex = math.frexp(abs(x))
    return math.copysign(1.0, x) < 0, int(math.ldexp(f, 53)), ex - 53


def fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once: rn64(F(a) * F(b) + F(c)) on integers; specials and exact zeros by IEEE's rules."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        if math.isfinite(a) and math.isfinite(b):
            return c                                               # a finite product never changes an infinite or NaN addend
        return a * b + c                                           # the product is +-inf or NaN exactly: one float add is the IEEE answer
    if a == 0.0 or b == 0.0:
        return a * b + c                                           # the product is an exact +-0
    na, ma, ka = _parts(a)
    nb, mb, kb = _parts(b)
    p, kp = ma * mb, ka + kb
    if na != nb:
        p = -p
    if c != 0.0:
        nc, mc, kc = _parts(c)
        k = min(kp, kc)
        p = (p << (kp - k)) + ((-mc if nc else mc) << (kc - k))
        kp = k
        if p == 0:
            return 0.0                                             # x + (-x) = +0 under round-to-nearest
    return _rn_scaled(p < 0, abs(p), 1, kp, 53, -1074, 1023)


def ulp64(v: float) -> float:
    """The spacing of doubles at |v| (the step 2^-1074 in the subnormal range)."""
    v = abs(float(v))
    if v < MIN_NORMAL64:
        return STEP64
    return math.ldexp(1.0, math.frexp(v)[1] - 53)


def bits64(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def bits32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def same_bits(got, want) -> np.ndarray:
    """Element-wise: the same double bit for bit, every NaN equal to every NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return (bits64(got) == bits64(want)) | (np.isnan(got) & np.isnan(want))


# ---------------------------------------------------------------------------------------
# exact powers
# ---------------------------------------------------------------------------------------
def exact_power(x, e: int) -> float:
    """rn64(Fraction(x) ** e) for every integer e; the specials as np.power has them: x^0 = 1 for every x (NaN and +-inf included), NaN -> NaN,
    +-inf and +-0 take their sign from the parity of e."""
    x, e = float(x), int(e)
    if e == 0:
        return 1.0
    if x != x:
        return NAN
    odd_neg = (e & 1) == 1 and math.copysign(1.0, x) < 0
    if math.isinf(x) or x == 0.0:
        big = math.isinf(x) == (e > 0)
        v = INF if big else 0.0
        return -v if odd_neg else v
    neg, m, k = _parts(x)
    n = abs(e)
    if e > 0:
        return _rn_scaled(odd_neg, m ** n, 1, k * n, 53, -1074, 1023)
    return _rn_scaled(odd_neg, 1, m ** n, -k * n, 53, -1074, 1023)


def power_fraction(x: float, e: int) -> Fraction:
    """Fraction(x) ** e of a finite non-zero x (what `exact_power` rounds)."""
    return Fraction(float(x)) ** int(e)


def power_class(exact: float, e: int) -> str:
    if exact != exact or math.isinf(exact) or exact == 0.0:
        return "exact"
    if e >= 0:
        return "exact" if abs(exact) >= MIN_NORMAL64 else "step"
    return "ulp" if abs(exact) >= MIN_NORMAL64 else "ulp-step"


def power_tolerance(exact: float, cls: str) -> float:
    """The largest |got - exact| the class allows (0: bit equality)."""
    return {"exact": 0.0, "step": STEP64, "ulp": ulp64(exact), "ulp-step": STEP64}[cls]


# ---------------------------------------------------------------------------------------
# the power table
# ---------------------------------------------------------------------------------------
PowerCase = namedtuple("PowerCase", "name x exact cls")

#: what the three roots of an exponent are there for: 2^(1024 / |e|) is where x^|e| overflows, 2^(-1022 / |e|) where it leaves the normal range,
#: 2^(-1074 / |e|) where it is the smallest subnormal, 2^(-1075 / |e|) where it underflows to zero (half a step: the tie goes to the even 0)
ROOTS = (("overflow-root", 1024), ("normal-root", -1022), ("underflow-root", -1074), ("zero-root", -1075))
ROOTS32 = (("f32-overflow-root", 128), ("f32-normal-root", -126), ("f32-underflow-root", -149))
#: finding 1: negative exponents whose positive power lies in (2^1022, 2^1074] — the reciprocal is a non-zero subnormal, or the smallest ones' tie to zero
OVERFLOWN_POWER_LOG2 = (1022.5, 1023.0, 1023.9, 1024.5, 1030.0, 1040.0, 1060.0, 1073.0, 1073.9)
#: finding 2: negative x whose |x|^|e| lies below 2^-1074 (the chain ends in -0 + +0)
UNDERFLOWN_POWER_LOG2 = (-1075.5, -1100.0, -1500.0, -3000.0)
NAMED_OVERFLOWN = ((2.0 ** 20, -52), (1e10, -31), (1e20, -16))


def _pow2(t: float) -> float:
    """2^t as a double (libm's exp2 on the fraction, ldexp on the whole part: within an ulp or two of the root, which is all a neighbourhood needs)."""
    w = math.floor(t)
    try:
        return math.ldexp(2.0 ** (t - w), int(w))
    except OverflowError:
        return INF


def root_below(t: int, n: int, dtype=np.float64):
    """The largest value of dtype whose n-th power is at most 2^t, found on integers: "the root itself" of a boundary 2^t (libm's guess is some
    ulps off, which is more than the neighbourhood's width once multiplied by n)."""
    bound = Fraction(2) ** t
    x = dtype(_pow2(t / n))
    up, down = dtype(np.inf), dtype(-np.inf)
    while Fraction(float(x)) ** n > bound:
        x = np.nextafter(x, down)
    while Fraction(float(np.nextafter(x, up))) ** n <= bound:
        x = np.nextafter(x, up)
    return x


def _neighbours(x, dtype, k=3):
    x = dtype(x)
    out, lo, hi = [(0, x)], x, x
    for i in range(1, k + 1):
        lo, hi = np.nextafter(lo, dtype(-np.inf)), np.nextafter(hi, dtype(np.inf))
        out += [(-i, lo), (i, hi)]
    return sorted(out, key=lambda t: t[0])


def power_inputs(e: int, dtype=np.float64):
    """[(name, x)]: the inputs of exponent e — a few hundred, every one named for what it aims at; float32 values when dtype is np.float32."""
    f32 = dtype == np.float32
    n = abs(e)
    rng = np.random.default_rng(1000 + e + (500 if f32 else 0))
    pos = []
    # random mantissas across the binades (float32: the binades it has), and the ones every exponent keeps in range
    for b in (range(-140, 121, 10) if f32 else range(-300, 301, 15)):
        pos.append((f"random/2^{b}", math.ldexp(1.0 + rng.random(), b)))
    for i in range(24):
        pos.append((f"random/unit-{i}", 0.5 + 1.5 * rng.random()))
    pos += [("one", 1.0), ("one+2^-52", 1.0 + 2.0 ** -52), ("one-2^-52", 1.0 - 2.0 ** -52), ("one-2^-53", 1.0 - 2.0 ** -53)]
    for k in ((-149, -126, -100, -64, -20, -1, 1, 2, 10, 16, 20, 64, 100, 127) if f32 else (-1074, -1022, -537, -100, -20, -1, 1, 2, 10, 16, 20, 100, 511, 512, 1023)):
        pos.append((f"pow2/2^{k}", math.ldexp(1.0, k)))
    if n >= 2:
        for name, t in ROOTS + (ROOTS32 if f32 else ()):
            if f32 and not -140 < t / n < 127:
                continue                                 # the double's boundary has no root among the float32 values
            for i, v in _neighbours(root_below(int(t), n, dtype), dtype):
                pos.append((f"{name}/{i:+d}", float(v)))
    pos += ([("subnormal/min", 2.0 ** -149), ("subnormal/mid", 1.5 * 2.0 ** -140), ("subnormal/max", 2.0 ** -126 - 2.0 ** -149), ("normal/min", 2.0 ** -126)] if f32 else
            [("subnormal/min", STEP64), ("subnormal/mid", 1.5 * 2.0 ** -1060), ("subnormal/max", MIN_NORMAL64 - STEP64), ("normal/min", MIN_NORMAL64)])
    pos.append(("max", float(np.finfo(dtype).max)))
    if e < 0:
        for t in OVERFLOWN_POWER_LOG2:
            if math.isfinite(_pow2(t / n)):
                pos.append((f"overflown-power/2^{t}", _pow2(t / n)))
        for x, ee in NAMED_OVERFLOWN:
            if ee == e:
                pos.append((f"overflown-power/named-{x:g}", x))
    if e != 0:
        for t in UNDERFLOWN_POWER_LOG2:
            if dtype(_pow2(t / n)) > 0:
                pos.append((f"underflown-power/2^{t}", _pow2(t / n)))
        if 200 * n * math.log2(10) > 1074:
            pos.append(("underflown-power/named-1e-200", 1e-200))
    pos += [("zero", 0.0), ("inf", INF)]
    out, seen = [], set()
    for name, x in pos:
        with np.errstate(over="ignore"):
            x = float(dtype(x))                          # a float32 table holds float32 values
        if (x == 0.0 or math.isinf(x)) and name not in ("zero", "inf"):
            continue                                     # (out of the float32 range)
        for sign, v in (("+", x), ("-", -x)):
            key = (math.copysign(1.0, v), abs(v))
            if key in seen:
                continue
            seen.add(key)
            out.append((f"{sign}{name}", v))
    out.append(("nan", NAN))
    return out


_TABLES = {}


def power_table(e: int, dtype=np.float64):
    """[PowerCase]: `power_inputs` with the exact power and its class (computed once per exponent and dtype)."""
    key = (int(e), np.dtype(dtype).name)
    if key not in _TABLES:
        cases = []
        for name, x in power_inputs(e, dtype):
            ex = exact_power(x, e)
            cases.append(PowerCase(name, x, ex, power_class(ex, e)))
        _TABLES[key] = cases
    return _TABLES[key]


def table_arrays(cases):
    """-> (x, exact, tolerance) float64 arrays of a case list"""
    x = np.array([c.x for c in cases], dtype=np.float64)
    ex = np.array([c.exact for c in cases], dtype=np.float64)
    tol = np.array([power_tolerance(c.exact, c.cls) for c in cases], dtype=np.float64)
    return x, ex, tol


def power_overflows(x: float, e: int) -> bool:
    """A finite x whose POSITIVE power |x|^|e| rounds to infinity (for e < 0: the cases of finding 1)."""
    return math.isfinite(x) and x != 0.0 and math.isinf(exact_power(abs(x), abs(e)))


def check_values(got, exact, tol, exact_sign=True):
    """Element-wise verdict of a result against the classes.  Where tol == 0: the same bits (any NaN for a NaN; with exact_sign=False a zero of
    either sign for a zero — a value that went through `0.0 + v` has lost a zero's sign).  Elsewhere also |got - exact| <= tol with a finite got
    that is zero or of the exact value's sign."""
    got, exact, tol = (np.asarray(a, dtype=np.float64) for a in (got, exact, tol))
    with np.errstate(invalid="ignore"):
        same = same_bits(got, exact)
        if not exact_sign:
            same = same | ((got == 0.0) & (exact == 0.0))
        near = np.isfinite(got) & (np.abs(got - exact) <= tol) & (np.signbit(got) == np.signbit(exact))
        if not exact_sign:
            near = near | (np.isfinite(got) & (np.abs(got - exact) <= tol) & (got == 0.0))
    return np.where(tol == 0.0, same, same | near)


# ---------------------------------------------------------------------------------------
# emulations of the device texts
# ---------------------------------------------------------------------------------------
def _clamp_finite(x: float) -> float:
    """clamp_finite (afhip_numerics.h): v_max(x, -2^1023) then v_min(., 2^1023); a NaN operand returns the other one."""
    if x != x:
        return -(2.0 ** 1023)
    return min(max(x, -(2.0 ** 1023)), 2.0 ** 1023)


def _chain(x: float, n: int):
    """powi_dd_vec's product chain for n >= 2 -> (hi, lo), unrenormalised (n = 2: the first step alone)"""
    hi = x * x
    lo = fma(x, x, -hi)
    for _ in range(n - 2):
        p = hi * x
        err = fma(hi, x, -p)
        lo = fma(lo, x, err)
        hi = p
    return hi, lo


def _div(a: float, b: float) -> float:
    """IEEE a / b on doubles (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _ldexp(v: float, k: int) -> float:
    """v_ldexp_f64: v 2^k rounded once, to nearest even (math.ldexp raises on overflow)."""
    if v != v or math.isinf(v) or v == 0.0:
        return v
    neg, m, kk = _parts(v)
    return _rn_scaled(neg, m, 1, kk + k, 53, -1074, 1023)


def emulate_powi(x: float, e: int, zero_sign: bool = False, sign_of_hi: bool = True) -> float:
    """`powi_dd_vec<N, true, ZERO_SIGN>` (afhip_numerics.h) on one element, statement by statement: the chain on x itself — the fused kernels'
    general group end (zero_sign=False); the lean group end's written-out chain (afhip_kernels.h, "leaf: x^n") is the same text for e >= 1.
    sign_of_hi=False: the text as it was before this catalogue — the zero's sign taken from hi by a select under ZERO_SIGN (k_transform) and not
    at all in the fused kernels (finding 2)."""
    x, e = float(x), int(e)
    if e == 0:
        return 1.0
    n = abs(e)
    if n == 2:
        x = x * x
    elif n > 2:
        hi, lo = _chain(x, n)
        x = hi + _clamp_finite(lo)
        if sign_of_hi:
            if math.copysign(1.0, hi) < 0:           # or_sign: hi's sign bit OR-ed in (hi + lo has hi's sign where it is not zero; the zero of
                x = -abs(x)                          # the product chain carries the power's)
        elif zero_sign and x == 0.0:
            x = hi
    if e < 0:
        x = _div(1.0, x)
    return x


def emulate_powi_scaled(x: float, e: int) -> float:
    """`powi_scaled_vec` (afhip_numerics.h), k_transform's power: for |e| >= 3 and e = -2 the chain on frexp's mantissa, the reciprocal, one ldexp."""
    x, e = float(x), int(e)
    n = abs(e)
    if n < 2 or e == 2:
        return emulate_powi(x, e, True)
    if x != x or math.isinf(x) or x == 0.0:
        f, k = x, 0                                  # v_frexp_mant_f64 returns these as they are, v_frexp_exp_i32_f64 returns 0
    else:
        f, k = math.frexp(x)
    v = emulate_powi(f, n, True)
    if e < 0:
        v = _div(1.0, v)
    return _ldexp(v, k * e)


# ---------------------------------------------------------------------------------------
# what the fused kernels promise: the chain runs on x itself there
# ---------------------------------------------------------------------------------------
LOST_TERMS = 2.0 ** -969           # 2^(-1022 + 53): below it the chain's error terms are subnormal or lost


def _near(got: float, want: float, tol: float) -> bool:
    if tol == 0.0 or want != want or math.isinf(want):
        return bool(same_bits(got, want)) or (got == 0.0 and want == 0.0)
    return math.isfinite(got) and abs(got - want) <= tol and (got == 0.0 or math.copysign(1.0, got) == math.copysign(1.0, want))


def fused_power_rule(x: float, e: int) -> str:
    """Which sentence of the fused kernels' contract a case falls under — decided from exact values alone:
    "class"       the four classes as they stand
    "one-ulp"     e > 0, 2^-1022 <= |exact| < 2^-969: within one ulp instead of correctly rounded; and a power that rounds to zero may be one step
    "brink"       the positive power |x|^|e| is finite and within |e| ulps of the largest double: the chain's high word, which carries up to
                  half an ulp of error per step until the error term is added, may have overflowed already — the class's value, or +-inf
                  (+-0 under a negative exponent) with the exact result's sign
    "zero"        e < 0 and the positive power overflows: +-0 with the exact result's sign (finding 1)
    "reciprocal"  e < 0 and 0 < |x|^|e| < 2^-969: the correctly rounded reciprocal of a positive power that is itself within one ulp (one step
                  below 2^-1022) of the exact one"""
    exact = exact_power(x, e)
    n = abs(e)
    if n < 2 or exact != exact or not math.isfinite(x) or x == 0.0:
        return "class"
    pos = exact_power(abs(x), n)
    if math.isinf(pos):
        return "zero" if e < 0 else "class"
    if n >= 3 and pos >= MAX64 - n * ulp64(MAX64):
        return "brink"
    if e > 0:
        return "one-ulp" if (MIN_NORMAL64 <= pos < LOST_TERMS or pos == 0.0) else "class"
    return "reciprocal" if 0.0 < pos < LOST_TERMS else "class"


def fused_power_ok(x: float, e: int, got: float) -> bool:
    """got against the fused kernels' contract for `0.0 + x^e` (the outer sum of one group: a zero has lost its sign)."""
    exact = exact_power(x, e)
    rule = fused_power_rule(x, e)
    negative = math.copysign(1.0, exact) < 0
    by_class = _near(got, 0.0 + exact, power_tolerance(exact, power_class(exact, e)))
    if rule == "class":
        return by_class
    if rule == "one-ulp":
        return _near(got, exact, ulp64(exact))
    if rule == "brink":
        return by_class or (got == 0.0 if e < 0 else got == (-INF if negative else INF))
    if rule == "zero":
        return got == 0.0
    pos = exact_power(abs(x), abs(e))
    return any(bool(same_bits(got, 0.0 + _div(-1.0 if negative else 1.0, p))) for p in (pos, math.nextafter(pos, 0.0), math.nextafter(pos, INF)))


def emulate_div_by(a: float, n: int) -> float:
    """`div_by(a, n, RN(1 / n))` (afhip_numerics.h) on a finite a: q0 = a y, r = fma(-q0, b, a), q = fma(r, y, q0); v_div_fixup leaves a finite
    quotient of finite operands as it is."""
    a, b = float(a), float(n)
    y = rn64(Fraction(1, n))
    q0 = a * y
    r = fma(-q0, b, a)
    return fma(r, y, q0)


# ---------------------------------------------------------------------------------------
# the mean table
# ---------------------------------------------------------------------------------------
MeanCase = namedtuple("MeanCase", "name n s rows exact cls")


def _split(s: float, n: int, rng):
    """n rows that add up to s exactly in any order: multiples of 2^-1074 of one sign (every partial sum is such a multiple below |s|: exact)."""
    units = int(Fraction(abs(s)) / Fraction(STEP64))
    cuts = sorted(int(c) for c in rng.integers(0, units + 1, size=n - 1))
    parts = np.diff([0] + cuts + [units])
    rows = [math.copysign(float(p) * STEP64, s) for p in parts]
    assert sum(Fraction(r) for r in rows) == Fraction(s) and all(abs(Fraction(r)) / Fraction(STEP64) == int(p) for r, p in zip(rows, parts))
    return rows


def mean_class(s: float, n: int) -> str:
    """From the quotient itself, before any rounding: `exact` where |s / n| >= 2^-1022 (and for s = 0), `step` below."""
    return "exact" if (s == 0.0 or abs(Fraction(s)) / n >= Fraction(MIN_NORMAL64)) else "step"


def mean_cases(n: int):
    """[MeanCase] of group length n: sums in the four bands of both signs, as one row s and n - 1 rows of +0 and (where s is a short multiple of
    2^-1074) split over the rows; for even n the constructed ties s = (2k + 1) (n / 2) 2^-1074, whose quotient lies half way between two subnormals."""
    rng = np.random.default_rng(7000 + n)
    sums = []
    for band, lo, hi, count in (("subnormal-quotient", -1074, -1022, 24), ("low-normal", -1022, -960, 10), ("ordinary", -40, 40, 10), ("huge", 900, 1023, 8)):
        for i in range(count):
            b = int(rng.integers(lo, hi))
            m = 1.0 + rng.random() if b > -1074 else 1.0
            sums.append((f"{band}/{i}", math.ldexp(m, b)))
    sums += [("subnormal-quotient/min", STEP64), ("subnormal-quotient/issue-2856", 2856 * STEP64), ("low-normal/min", MIN_NORMAL64), ("huge/max", MAX64),
             ("ordinary/one", 1.0), ("ordinary/n", float(n)), ("zero", 0.0)]
    if n % 2 == 0:
        for k in (0, 1, 2, 3, 29, 100, 2 ** 20, 2 ** 40 + 1, 2 ** 51 - 1):
            s = (2 * k + 1) * (n // 2) * STEP64
            if (2 * k + 1) * (n // 2) < 2 ** 53:
                sums.append((f"tie/k={k}", s))
    out = []
    for name, s in sums:
        for sign, v in (("+", s), ("-", -s)):
            if name == "zero" and sign == "-":
                continue
            exact = rn64(Fraction(v) / n) if v != 0.0 else 0.0
            cls = mean_class(v, n)
            rows = [v] + [0.0] * (n - 1)
            out.append(MeanCase(f"{sign}{name}/one-row", n, v, rows, exact, cls))
            if n > 1 and 0.0 < abs(v) < MIN_NORMAL64:                 # (below 2^52 steps: every part is a double)
                out.append(MeanCase(f"{sign}{name}/split", n, v, _split(v, n, rng), exact, cls))
    return out


def is_tie(case) -> bool:
    """The exact quotient lies half way between two neighbouring doubles."""
    if case.s == 0.0:
        return False
    q = Fraction(case.s) / case.n
    unit = Fraction(ulp64(case.exact)) if abs(case.exact) >= MIN_NORMAL64 else Fraction(STEP64)
    return (2 * q / unit).denominator == 1 and (q / unit).denominator == 2


# ---------------------------------------------------------------------------------------
# hinge and interact tables
# ---------------------------------------------------------------------------------------
KNOTS = (20.0, 20.1, 0.0)          # 20.1 is no float32: the float32 -> float32 hinge compares against (float)20.1


def hinge_inputs(knot: float, dtype=np.float64):
    """x values of a hinge at `knot`: the knot, its neighbours (in both precisions), zeros, infinities, NaN, subnormals, +-max (x - k overflows)."""
    fi = np.finfo(dtype)
    k = dtype(knot)
    vals = [k, np.nextafter(k, dtype(np.inf)), np.nextafter(k, dtype(-np.inf)), -k, dtype(np.float32(knot)), dtype(np.nextafter(np.float32(knot), np.float32(np.inf))),
            dtype(np.nextafter(np.float32(knot), np.float32(-np.inf))), 0.0, -0.0, np.inf, -np.inf, np.nan, fi.smallest_subnormal, -fi.smallest_subnormal,
            fi.tiny, -fi.tiny, fi.tiny - fi.smallest_subnormal, fi.max, -fi.max, 1.0, -1.0, 25.5, 19.999, 1e30, -1e30]
    return np.array(vals, dtype=dtype)


def hinge_expected(x: np.ndarray, knot: float, out_dtype):
    """numpy's `(x > k) * (x - k)` in the dtype its rules give (a Python-float knot is weak: float32 x stays float32), stored as out_dtype.
    Note False * -inf = NaN and False * negative = -0.0."""
    with np.errstate(all="ignore"):
        if x.dtype == np.float32 and np.dtype(out_dtype) == np.float32:
            k = np.float32(knot)
            return ((x > k).astype(np.float32) * (x - k)).astype(np.float32)
        xd = x.astype(np.float64)
        return ((xd > knot).astype(np.float64) * (xd - knot)).astype(out_dtype)


def inter_inputs(dtype=np.float64):
    """(x, other): factor pairs with 0 * inf, inf * -1, products that overflow, underflow to subnormals and to +-0, signed zeros, NaN."""
    fi = np.finfo(dtype)
    mx, tiny, sub = fi.max, fi.tiny, fi.smallest_subnormal
    pairs = [(0.0, np.inf), (-0.0, np.inf), (np.inf, 0.0), (np.inf, -1.0), (-np.inf, -1.0), (np.inf, -np.inf), (np.nan, 1.0), (1.0, np.nan), (np.nan, 0.0),
             (mx, 2.0), (mx, -2.0), (-mx, mx), (mx, 1.0), (mx, 1.0 + fi.eps), (mx, 1.0 - fi.epsneg),
             (tiny, 0.5), (tiny, -0.5), (tiny, 0.75), (tiny, tiny), (-tiny, tiny), (sub, 0.5), (sub, -0.5), (sub, 0.75), (sub, 1.5), (sub, sub), (-sub, sub), (sub, mx),
             (0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (-0.0, 5.0), (0.0, -5.0), (1.0, 1.0), (-1.0, 1.0), (3.0, 1.0 / 3.0), (1.0 + fi.eps, 1.0 + fi.eps), (1e10, 1e-10),
             (np.sqrt(mx), np.sqrt(mx)), (np.sqrt(tiny), np.sqrt(tiny)), (tiny * 4, 0.25 + fi.eps)]
    return np.array([p[0] for p in pairs], dtype=dtype), np.array([p[1] for p in pairs], dtype=dtype)


def inter_expected(x: np.ndarray, other: np.ndarray, out_dtype):
    """numpy's `x * other` in the dtype its rules give, stored as out_dtype.  (float32 x float32 stored as float32: the float64 product of two
    float32 values is exact, so rounding it once is the float32 product.)"""
    with np.errstate(all="ignore"):
        if x.dtype == np.float32 and other.dtype == np.float32 and np.dtype(out_dtype) == np.float32:
            return (x * other).astype(np.float32)
        return (x.astype(np.float64) * other.astype(np.float64)).astype(out_dtype)
