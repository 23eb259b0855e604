"""The catalogue of tests/numerics_cases.py, checked without a GPU: the exact roundings against Python's own and hand-worked cases, `exact_power`
against np.power, every table against what its names say (a census per exponent), and the emulated device texts — `powi_dd_vec`'s chain, `div_by` —
against exact rational arithmetic on every case, so that the zero tolerance the GPU tests apply is one the arithmetic can meet.

Emulation, not a device: tests/test_gpu_numerics.py runs the same tables through the kernels.  Miss counts of the emulations (this file asserts them):
    powi_scaled_vec (k_transform)        0 of 32,513 float64 cases and 0 of the float32 table's, by the four classes
    powi_dd_vec (the fused kernels)      0 of the 21,853 cases its contract holds to the four classes; of the others, by the four classes:
                                         250 of 4,370 powers below 2^-969, 8 of 212 on the brink of overflow, 1,044 of 3,884 negative powers behind an
                                         overflowed positive one (finding 1), 30 of 2,194 behind one below 2^-969 — each within its own sentence
    ... before its sign came from hi     879 infinities of the wrong sign (finding 2)
    div_by                               0 of 996 `exact` cases; 100 of 1,918 `step` cases, every one of them among the 386 exact ties (finding 3)
"""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import numerics_cases as nc

INF = math.inf


# ---- 1. the roundings ----
def test_rn64_and_rn32_against_python_and_hand_worked_cases():
    rng = np.random.default_rng(11)
    for _ in range(4000):
        m, b = float(rng.random() * 2 - 1), int(rng.integers(-1080, 1000))
        fr = F(math.ldexp(m, b)) * F(int(rng.integers(1, 10 ** 6)), int(rng.integers(1, 10 ** 6)))
        assert nc.rn64(fr) == fr.numerator / fr.denominator                    # int / int is correctly rounded in Python
        if -140 < b < 120:
            assert nc.rn32(fr) == np.float32(fr.numerator / fr.denominator) or _double_rounds(fr)
    # hand-worked: ties to even at 2^53, in the subnormal range and at the two ends
    assert nc.rn64(F(2 ** 53 + 1)) == 2.0 ** 53 and nc.rn64(F(2 ** 53 + 3)) == 2.0 ** 53 + 4
    assert nc.rn64(F(1, 3)) == 1.0 / 3.0 and nc.rn64(F(-2, 3)) == -2.0 / 3.0
    step = F(1, 2 ** 1074)
    assert nc.rn64(step / 2) == 0.0 and nc.rn64(step * 3 / 2) == 2 * nc.STEP64 and nc.rn64(step * 5 / 2) == 2 * nc.STEP64
    assert nc.rn64(F(119, 2) * step) == 60 * nc.STEP64 and nc.rn64(F(121, 2) * step) == 60 * nc.STEP64          # the issue's 59.5 steps
    assert math.copysign(1.0, nc.rn64(-step / 2)) == -1.0 and nc.rn64(-step / 2) == 0.0                         # a negative value that rounds to zero: -0
    assert math.copysign(1.0, nc.rn64(F(0))) == 1.0
    top = F(2 ** 1024) - F(2 ** 970)                                                                            # half way between the largest double and 2^1024
    assert nc.rn64(top) == INF and nc.rn64(-top) == -INF and nc.rn64(top - 1) == nc.MAX64
    assert nc.rn32(F(2 ** 24 + 1)) == np.float32(2 ** 24) and nc.rn32(F(2 ** 24 + 3)) == np.float32(2 ** 24 + 4)
    assert nc.rn32(F(2 ** 128) - F(2 ** 103)) == np.float32(INF) and nc.rn32(F(2 ** 128) - F(2 ** 103) - 1) == np.finfo(np.float32).max
    assert nc.rn32(F(1, 2 ** 150)) == 0 and nc.rn32(F(3, 2 ** 150)) == np.float32(2.0 ** -148) and np.signbit(nc.rn32(F(-1, 2 ** 150)))
    # rounded once, not through a double: 1 + 2^-24 + 2^-60 lies above the float32 tie, its double on it
    assert nc.rn32(1 + F(1, 2 ** 24) + F(1, 2 ** 60)) == np.float32(1 + 2.0 ** -23) and np.float32(float(1 + F(1, 2 ** 24) + F(1, 2 ** 60))) == np.float32(1.0)


def _double_rounds(fr):
    """The double of fr sits exactly on a float32 tie (then rounding through it may differ from rounding once)."""
    d = F(fr.numerator / fr.denominator)
    return d != fr and nc.rn32(d) != nc.rn32(fr)


def test_exact_fma_against_fractions():
    rng = np.random.default_rng(12)
    for _ in range(3000):
        a, b, c = (math.ldexp(float(rng.random() * 2 - 1), int(rng.integers(-540, 510))) for _ in range(3))
        if rng.random() < 0.3:
            c = -(a * b)                                       # cancellation: the result is the product's rounding error
        assert nc.fma(a, b, c) == nc.rn64(F(a) * F(b) + F(c)), (a, b, c)
    assert nc.fma(INF, 2.0, -INF) != nc.fma(INF, 2.0, -INF) and nc.fma(INF, 2.0, 1.0) == INF and nc.fma(1e308, 10.0, -INF) == -INF
    assert math.copysign(1.0, nc.fma(-0.0, 5.0, 0.0)) == 1.0 and math.copysign(1.0, nc.fma(-0.0, 5.0, -0.0)) == -1.0 and nc.fma(2.0, 3.0, -6.0) == 0.0
    assert nc.fma(1e308, 10.0, -1e308) == INF and nc.fma(nc.STEP64, 0.5, 0.0) == 0.0 and nc.fma(nc.STEP64, 0.5, nc.STEP64) == 2 * nc.STEP64


def test_exact_power_against_np_power():
    """Within 1 ulp of libm's on ordinary values (np.power is not exact: that is why it is no reference here), bit-equal on the specials."""
    rng = np.random.default_rng(13)
    x = np.concatenate([rng.normal(18, 9, 300), rng.uniform(-2, 2, 300), np.ldexp(1.0 + rng.random(100), rng.integers(-10, 10, 100))])
    for e in (-64, -33, -5, -3, -2, -1, 1, 2, 3, 4, 5, 8, 17, 33, 64):
        with np.errstate(all="ignore"):
            want = np.power(x, e)
        got = np.array([nc.exact_power(v, e) for v in x])
        ok = np.isfinite(want) & (np.abs(want) > 1e-290)
        assert ok.sum() > 500
        assert np.all(np.abs(got[ok] - want[ok]) <= np.array([nc.ulp64(v) for v in got[ok]])), e
        assert np.all(got[ok] == np.array([nc.rn64(nc.power_fraction(v, e)) for v in x[ok]]))          # the definition: rn64(Fraction(x) ** e)
    specials = np.array([0.0, -0.0, INF, -INF, np.nan, 1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 2.0 ** 20, -(2.0 ** -30)])
    for e in nc.EXPONENTS:
        with np.errstate(all="ignore"):
            want = np.power(specials, e)
        got = np.array([nc.exact_power(v, e) for v in specials])
        assert np.all(nc.same_bits(got, want)), (e, got, want)                                          # powers of two are exact in any libm
    # the issue's three: a zero where a non-zero subnormal belongs
    assert nc.exact_power(2.0 ** 20, -52) == 2.0 ** -1040 and nc.exact_power(1e10, -31) > 0 and nc.exact_power(1e20, -16) > 0


# ---- 2. the tables ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_power_table_census(dtype):
    """Every exponent's table holds what its names say: overflow-root, normal-root and underflow-root neighbourhoods that straddle their
    boundary, `step` cases, signed zeros and infinities of both signs, the band of finding 1 and the inputs of finding 2."""
    total, classes = 0, {}
    for e in nc.EXPONENTS:
        cases = nc.power_table(e, dtype)
        names = [c.name for c in cases]
        assert len(set(names)) == len(names) and 120 <= len(cases) <= 350, (e, len(cases))
        if dtype == np.float32:
            assert all(float(np.float32(c.x)) == c.x or c.x != c.x for c in cases)
        total += len(cases)
        for c in cases:
            classes[c.cls] = classes.get(c.cls, 0) + 1
            assert c.cls == nc.power_class(c.exact, e) and (nc.same_bits(c.exact, nc.exact_power(c.x, e)))
        by = lambda prefix: [c for c in cases if c.name[1:].startswith(prefix)]
        assert {"+one", "-one", "+zero", "-zero", "+inf", "-inf", "nan", "+subnormal/mid", "-subnormal/max"} <= set(names)
        tiny = float(np.finfo(dtype).smallest_subnormal)
        assert {tiny, -tiny} <= {c.x for c in cases}                      # (named pow2/2^-1074: a value stands once, under its first name)
        if e == 0:
            assert all(c.exact == 1.0 for c in cases)
            continue
        n = abs(e)
        if n >= 2:
            over, norm, under, zero = by("overflow-root"), by("normal-root"), by("underflow-root"), by("zero-root")
            if dtype == np.float64:
                assert min(len(over), len(norm), len(under), len(zero)) >= 12                # (a root that is a power of two stands under pow2/)
            else:                                                               # the float32 values have the double's roots only for larger |e| ...
                assert min(len(by("f32-overflow-root")), len(by("f32-normal-root")), len(by("f32-underflow-root"))) >= 12       # ... and always their own
                assert (len(over) >= 12) == (1024 / n < 127) and (len(norm) >= 12) == (1022 / n < 140) and (len(under) >= 12) == (len(zero) >= 12) == (1075 / n < 140), e
            straddles = lambda group, bound: any(nc.exact_power(abs(c.x), n) > bound for c in group) and any(nc.exact_power(abs(c.x), n) <= bound for c in group)
            assert (not over or straddles(over, nc.MAX64)) and (not norm or straddles(norm, nc.MIN_NORMAL64 - nc.STEP64)) and (not zero or straddles(zero, 0.0)), e
            assert all(abs(nc.exact_power(c.x, n)) == nc.STEP64 for c in under), e
        if dtype == np.float64 or n >= 8:                                  # (float32 inputs reach the double's subnormal powers from |e| = 8 on)
            assert any(c.cls == ("step" if e > 0 else "ulp-step") for c in cases), e
        # sign cases: infinities and zeros of both signs among the results of odd exponents, of one sign among those of even ones
        signs = {(math.isinf(c.exact), math.copysign(1.0, c.exact)) for c in cases if c.exact == 0.0 or math.isinf(c.exact)}
        assert signs == ({(True, 1.0), (True, -1.0), (False, 1.0), (False, -1.0)} if n % 2 else {(True, 1.0), (False, 1.0)}), (e, signs)
        if e < -1 and (dtype == np.float64 or n >= 9):           # (x^1 cannot overflow; float32 inputs reach 2^1024 from |e| = 9 on)
            f1 = [c for c in by("overflown-power") if nc.power_overflows(c.x, e) and c.exact != 0.0]
            assert len(f1) >= 6 and all(c.cls == "ulp-step" for c in f1), e                       # finding 1: non-zero subnormals behind an overflowed power
        f2 = [c for c in cases if c.name.startswith("-underflown-power") or c.name == "-zero"]
        assert len(f2) >= (2 if n >= 2 and dtype == np.float64 else 1) and all((math.isinf(c.exact) if e < 0 else c.exact == 0.0) and (math.copysign(1.0, c.exact) < 0) == (n % 2 == 1) for c in f2), e
    assert total == sum(classes.values()) and min(classes.values()) > 500, classes
    if dtype == np.float64:
        assert any(c.x == 2.0 ** 20 for c in nc.power_table(-52)) and any(c.x == 1e10 for c in nc.power_table(-31)) and any(c.x == 1e20 for c in nc.power_table(-16))
        assert any(c.x == -1e-200 and c.exact == -INF for c in nc.power_table(-3)) and total == 32513, total


# ---- 3. the emulated chains against the exact power ----
#: `exact` cases on which the emulated k_transform chain is not the correctly rounded power, held to 1 ulp instead ((dtype, e, name)).  At most
#: one in 10,000 of the table may stand here; none does.
NOT_CORRECTLY_ROUNDED = ()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_emulated_transform_chain_meets_every_class(dtype):
    """`emulate_powi_scaled` — the device text of k_transform's power, powi_scaled_vec — equals `exact_power` bit for bit on every `exact` case
    and stays inside the bound of every other class."""
    total, listed = 0, 0
    tag = np.dtype(dtype).name
    for e in nc.EXPONENTS:
        cases = nc.power_table(e, dtype)
        _, _, tol = nc.table_arrays(cases)
        for c, t in zip(cases, tol):
            if (tag, e, c.name) in NOT_CORRECTLY_ROUNDED:
                assert c.cls == "exact"
                t, listed = nc.ulp64(c.exact), listed + 1
            got = nc.emulate_powi_scaled(c.x, e)
            assert nc.check_values([got], [c.exact], [t])[0], (e, c, got)
        total += len(cases)
    assert listed == len([t for t in NOT_CORRECTLY_ROUNDED if t[0] == tag]) and listed * 10_000 <= total


#: how many float64 cases fall under each sentence of the fused kernels' contract (`fused_power_rule`), and how many of those the emulated chain
#: really misses by the four classes — so each sentence is there for cases the table holds
FUSED_CENSUS = {"class": (21853, 0), "one-ulp": (4370, 250), "brink": (212, 8), "zero": (3884, 1044), "reciprocal": (2194, 30)}


def test_emulated_fused_chain_meets_its_contract():
    """`emulate_powi(.., zero_sign=False)` — powi_dd_vec as the fused kernels instantiate it, the chain on x itself — meets the four classes
    wherever `fused_power_rule` says "class" (the sign of a zero aside: the outer sum loses it), and the documented value or bound under the
    three other sentences.  Without the sign select under e < 0 (the text as it was) it returns the infinity of the wrong sign: finding 2."""
    census = {k: [0, 0] for k in FUSED_CENSUS}
    wrong_sign_before = 0
    for e in nc.EXPONENTS:
        cases = nc.power_table(e)
        _, _, tol = nc.table_arrays(cases)
        for c, t in zip(cases, tol):
            got = 0.0 + nc.emulate_powi(c.x, e, False)
            rule = nc.fused_power_rule(c.x, e)
            assert nc.fused_power_ok(c.x, e, got), (e, c, got, rule)
            by_class = bool(nc.check_values([got], [0.0 + c.exact], [t], exact_sign=False)[0])
            census[rule][0] += 1
            census[rule][1] += not by_class
            assert by_class or rule != "class"
            before = 0.0 + nc.emulate_powi(c.x, e, False, sign_of_hi=False)
            if not nc.same_bits(before, got):
                assert e < 0 and e % 2 == 1 and (c.x < 0 or (c.x == 0.0 and math.copysign(1.0, c.x) < 0)), (e, c)
                assert math.isinf(got) and got == -before and nc.same_bits(got, c.exact), (e, c, got, before)
                wrong_sign_before += 1
    assert {k: tuple(v) for k, v in census.items()} == FUSED_CENSUS, census
    assert all(missed > 0 for rule, (n, missed) in FUSED_CENSUS.items() if rule != "class") and wrong_sign_before == FINDING_2_CASES, wrong_sign_before
    # the issue's examples
    assert nc.emulate_powi(2.0 ** 20, -52, False) == 0.0 and nc.fused_power_rule(2.0 ** 20, -52) == "zero" and nc.emulate_powi_scaled(2.0 ** 20, -52) == 2.0 ** -1040
    assert nc.emulate_powi(1e10, -31, False) == 0.0 and nc.emulate_powi(1e20, -16, False) == 0.0
    assert nc.emulate_powi(-0.0, -3, False, sign_of_hi=False) == INF and nc.emulate_powi(-0.0, -3, False) == -INF
    assert nc.emulate_powi(-1e-200, -3, False, sign_of_hi=False) == INF and nc.emulate_powi(-1e-200, -3, False) == -INF


FINDING_2_CASES = 879          # infinities that had the wrong sign in the fused form before the sign bit was taken from hi


# ---- 4. means ----
def test_mean_table_and_emulated_div_by():
    """Each case's rows add up to s exactly in any order; the expected mean is rn64(Fraction(s) / n); `emulate_div_by` equals it on every `exact`
    case and stays within one subnormal step on the others — where it does miss, ties among them (finding 3)."""
    n_cases = {"exact": 0, "step": 0}
    missed, ties, tie_missed = 0, 0, 0
    rng = np.random.default_rng(14)
    for n in nc.MEAN_LENGTHS:
        cases = nc.mean_cases(n)
        assert len({c.name for c in cases}) == len(cases)
        bands = {c.name[1:].split("/")[0] for c in cases}
        assert {"subnormal-quotient", "low-normal", "ordinary", "huge", "zero"} <= bands and (("tie" in bands) == (n % 2 == 0))
        assert any("/split" in c.name for c in cases) or n == 1
        for c in cases:
            assert len(c.rows) == n and c.exact == (nc.rn64(F(c.s) / n) if c.s else 0.0) and c.cls == nc.mean_class(c.s, n)
            for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):               # any order adds up to s without a rounding
                acc = 0.0
                for i in order:
                    assert F(acc) + F(c.rows[i]) == F(acc + c.rows[i])
                    acc += c.rows[i]
                assert acc == c.s
            got = nc.emulate_div_by(c.s, n)
            n_cases[c.cls] += 1
            tie = nc.is_tie(c)
            ties += tie
            if c.cls == "exact":
                assert nc.same_bits(got, c.exact), (c, got)
            else:
                assert abs(got - c.exact) <= nc.STEP64 and (got == 0.0 or (got < 0) == (c.exact < 0)), (c, got)
                if got != c.exact:
                    missed, tie_missed = missed + 1, tie_missed + tie
            if c.name.startswith(("+tie", "-tie")):
                assert tie and c.cls == "step", c
    assert nc.emulate_div_by(2856 * nc.STEP64, 48) == 59 * nc.STEP64 and nc.rn64(F(2856 * nc.STEP64) / 48) == 60 * nc.STEP64       # the issue's example
    assert missed > 0 and tie_missed > 0, (missed, tie_missed)                                  # the table provably contains the hard cases
    assert (n_cases, missed, ties, tie_missed) == (MEAN_CENSUS["classes"], MEAN_CENSUS["step_missed"], MEAN_CENSUS["ties"], MEAN_CENSUS["ties_missed"]), \
        (n_cases, missed, ties, tie_missed)


MEAN_CENSUS = {"classes": {"exact": 996, "step": 1918}, "step_missed": 100, "ties": 386, "ties_missed": 100}


# ---- 5. hinge and interact ----
def test_hinge_and_interact_tables():
    for dt in (np.float64, np.float32):
        for knot in nc.KNOTS:
            x = nc.hinge_inputs(knot, dt)
            want = nc.hinge_expected(x, knot, dt)
            assert want.dtype == dt and np.isnan(x).any() and np.isinf(x).any() and (x == dt(knot)).any()
            with np.errstate(all="ignore"):
                assert np.all(nc.same_bits(want, (x > knot) * (x - dt(knot))))                    # the numpy expression itself, in numpy's dtype
            assert np.isnan(want[x == -np.inf]).all()                                            # False * -inf
            z = want[(x < dt(knot)) & np.isfinite(x)]
            assert len(z) and np.all(z == 0.0) and np.signbit(z).all()                           # False * negative = -0.0
            assert np.isfinite(want[np.abs(x) == np.finfo(dt).max]).all()                    # (with knots >= 0 and far below the spacing at max, +-max - k is +-max: no overflow)
        assert float(np.float32(20.1)) != 20.1
        x, o = nc.inter_inputs(dt)
        for odt in (dt, np.float64):
            want = nc.inter_expected(x, o.astype(odt), np.result_type(dt, odt))
            with np.errstate(all="ignore"):
                assert want.dtype == np.result_type(dt, odt) and np.all(nc.same_bits(want, np.multiply(x, o.astype(odt))))
            assert np.isnan(want[:2]).all() and want[3] == -np.inf and np.isinf(want).sum() >= 3
            assert ((want == 0.0) & np.signbit(want)).any() and ((want == 0.0) & ~np.signbit(want)).any()
            fi = np.finfo(want.dtype)
            assert ((want != 0.0) & (np.abs(want) < fi.tiny)).any() or want.dtype != dt          # products that underflow to subnormals
