"""The catalogue of tests/numerics_cases.py on the GPU: every exponent the host lowers to the double-double chain (-64 .. 64) against exact rational
arithmetic — through `hip.transform` (k_transform: powi_scaled_vec) and through `FusedPlan.run_temporal` under `exact_order` in every group-end text
that holds a copy of the chain (the general form, `_pair`, `_pair_lean`, the lean three-row form) —, the lowering boundary to device `pow`, the launch
geometry of k_transform, hinge and interact on special values bit for bit, and `div_by` behind inner means (and the outer mean's division) against
the exact quotient.  Tolerances by class (numerics_cases: exact / step / ulp / ulp-step); tests/test_numerics_host.py proves them fair on the emulated
device texts.  The fused kernels run the chain on x itself, and their contract says in four sentences where that differs from the classes
(`numerics_cases.fused_power_rule`): each is asserted as documented.

Packed and float32 cubes run a general-form plan of their own on the values a packed cube reaches (`test_fused_power_table_packed_and_float32`): every float32
is a stored 1 under an unpack rule whose multiplier it is, so the cases of findings 1 and 2, powers of two and the float32 roots are all within reach.

With AGGFLY_NUMERICS_COUNTS=<file> in the environment the tests leave their per-class counts in that JSON file (results that are inside their
bound but not the correctly rounded value): the figures of profiles/numerics_exact.txt.
"""
import json
import math
import os

import numpy as np
import pytest

import numerics_cases as nc

pytestmark = pytest.mark.gpu
WG, TRANSFORM_PER_THREAD = 256, 4             # afhip_plan_types.h, afhip_panel_kernels.h
CELLS = 70                                    # one wave and six tail lanes (two cells per lane: 35 lanes)


def _record(key, value):
    path = os.environ.get("AGGFLY_NUMERICS_COUNTS")
    if path:
        data = {}
        if os.path.exists(path):
            with open(path) as f:
                data = json.load(f)
        data[key] = value
        text = json.dumps(data, indent=1, sort_keys=True, default=lambda o: o.item())          # (numpy scalars)
        with open(path, "w") as f:
            f.write(text)


def _name(plan):
    return plan.describe().split()[0].replace("variant=", "")


def _spacing32(v):
    v = np.abs(np.asarray(v, dtype=np.float32))
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(v), (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64), 0.0)


# ---- 1. k_transform: every exponent ----
INEXACT_ON_DEVICE = {("float64", "float64"): {"step": 160, "ulp": 1414, "ulp-step": 184}, ("float32", "float64"): {"step": 96, "ulp": 2062, "ulp-step": 148},
                     ("float32", "float32"): {}}


@pytest.mark.parametrize("x_dtype,out_dtype", [(np.float64, np.float64), (np.float32, np.float32), (np.float32, np.float64)], ids=["f64", "f32", "f32-f64"])
def test_transform_pow_every_exponent(torch_cuda, x_dtype, out_dtype):
    """`hip.transform(x, "pow", e)` for e = -64 .. 64, one launch per exponent on that exponent's table, against `exact_power` by class.  A float32
    result is np.float32(the exact double): bit-equal wherever the double's class is `exact` (and where the double is below the float32 range: a
    signed zero), else within one float32 step — two doubles an ulp apart round to the same or to neighbouring floats."""
    from aggfly_amd import hip
    torch = torch_cuda
    tdt = torch.float64 if out_dtype == np.float64 else torch.float32
    bad, inexact, total = [], {}, 0
    for e in nc.EXPONENTS:
        cases = nc.power_table(e, x_dtype)
        x, exact, tol = nc.table_arrays(cases)
        got = hip.transform(torch.from_numpy(x.astype(x_dtype)).cuda(), "pow", float(e), out_dtype=tdt).cpu().numpy()
        assert got.dtype == out_dtype and got.shape == x.shape
        if out_dtype == np.float64:
            ok = nc.check_values(got, exact, tol)
            strict = nc.same_bits(got, exact)
        else:
            with np.errstate(over="ignore"):
                want = exact.astype(np.float32)
            tol32 = np.where((tol == 0.0) | (np.abs(exact) < 2.0 ** -150), 0.0, _spacing32(want))
            ok = nc.check_values(got.astype(np.float64), want.astype(np.float64), tol32)
            strict = nc.same_bits(got.astype(np.float64), want.astype(np.float64))
        total += len(cases)
        for c, o, s, g in zip(cases, ok, strict, got):
            if not o:
                bad.append((e, c.name, c.x, float(g), c.exact, c.cls))
            elif not s:
                inexact[c.cls] = inexact.get(c.cls, 0) + 1
    _record(f"transform_pow/{np.dtype(x_dtype).name}->{np.dtype(out_dtype).name}", {"cases": total, "outside_bound": len(bad), "inside_bound_not_correctly_rounded": inexact})
    assert not bad, (len(bad), bad[:12])
    # the device's counts of results inside their bound that are not the correctly rounded value (profiles/numerics_exact.txt, section 4): asserted, so
    # that neither the file nor the arithmetic drifts unseen
    assert inexact == INEXACT_ON_DEVICE[np.dtype(x_dtype).name, np.dtype(out_dtype).name], inexact


# ---- 2. the lowering boundary ----
def _exact_half_power(x, twice_e):
    """rn64(x ** (twice_e / 2)) for x > 0 by an integer square root (80 guard bits: far more than the bar needs)."""
    fr = nc.power_fraction(x, twice_e)
    s = 2 * (80 + max(0, fr.denominator.bit_length() - fr.numerator.bit_length()))
    return nc.rn64(nc.Fraction(math.isqrt(fr.numerator * fr.denominator << s), fr.denominator << (s // 2)))


def test_pow_lowering_boundary(torch_cuda):
    """|e| = 64 still takes the chain (test_transform_pow_every_exponent holds it to the classes); 65, -65 and 64.5 take device `pow`, held to the bar the
    project uses for it: 1e-12 relative on ordinary x, and bit-equal on the specials and on powers of two."""
    from aggfly_amd import hip
    torch = torch_cuda
    rng = np.random.default_rng(21)
    ordinary = np.concatenate([0.5 + 1.5 * rng.random(300), -(0.5 + 1.5 * rng.random(100)), rng.normal(18, 9, 100)])
    pow2 = np.array([2.0 ** k for k in (-14, -8, -2, 0, 2, 4, 10, 14)] + [-(2.0 ** k) for k in (-8, -2, 0, 2, 10)])
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0])
    x = np.concatenate([ordinary, pow2, special])
    d = torch.from_numpy(x).cuda()
    for e in (65, -65, 64.5):
        got = hip.transform(d, "pow", float(e)).cpu().numpy()
        with np.errstate(all="ignore"):
            libm = np.power(x, e)
        if e == 64.5:
            want = np.array([_exact_half_power(v, 129) if v > 0 and np.isfinite(v) else w for v, w in zip(x, libm)])      # (negative x: NaN, as libm's)
        else:
            want = np.array([nc.exact_power(v, e) for v in x])
        o, p = len(ordinary), len(ordinary) + len(pow2)
        assert np.array_equal(np.isnan(got), np.isnan(want)), e
        fin = ~np.isnan(want[:o])
        assert np.all(np.abs(got[:o][fin] - want[:o][fin]) <= 1e-12 * np.abs(want[:o][fin])), (e, np.max(np.abs(got[:o][fin] / want[:o][fin] - 1)))
        assert np.all(nc.same_bits(got[o:], want[o:])), (e, x[o:], got[o:], want[o:])
        assert np.all(nc.same_bits(want[p:], libm[p:]))                                   # the specials are C99's, whoever computes them
    for e in (64, -64):                                                                    # ... and on the chain's side of the boundary: exact, not 1e-12
        got = hip.transform(torch.from_numpy(ordinary).cuda(), "pow", float(e)).cpu().numpy()
        want = np.array([nc.exact_power(v, e) for v in ordinary])
        tol = np.array([nc.power_tolerance(w, nc.power_class(w, e)) for w in want])
        assert np.all(nc.check_values(got, want, tol)), e


# ---- 3. launch geometry of k_transform ----
BLOCK = WG * TRANSFORM_PER_THREAD
LENGTHS = (0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK - 1, 3 * BLOCK, 3 * BLOCK + 1)
_GEOMETRY = {}


def _geometry_reference(kind):
    """x, other and the expected values of the longest case, computed once (shorter lengths are prefixes)."""
    if kind not in _GEOMETRY:
        rng = np.random.default_rng(22)
        n = max(LENGTHS)
        x, other = rng.normal(18, 9, n), rng.normal(0, 3, n)
        want = {"pow": lambda: np.array([nc.exact_power(v, 3) for v in x]), "hinge": lambda: nc.hinge_expected(x, 20.1, np.float64),
                "inter": lambda: nc.inter_expected(x, other, np.float64)}[kind]()
        _GEOMETRY[kind] = (x, other, want)
    return _GEOMETRY[kind]


@pytest.mark.parametrize("kind", ["pow", "hinge", "inter"])
def test_transform_launch_geometry(torch_cuda, kind):
    """Lengths 0, 1 and around one and three blocks of WG * TRANSFORM_PER_THREAD elements; the input a slice that starts one element into its
    allocation, the output a slice of a larger buffer filled with a sentinel, the whole buffer compared: nothing is written beyond n or before 0."""
    from aggfly_amd import hip
    torch = torch_cuda
    lib = hip.load()
    x, other, want = _geometry_reference(kind)
    code = {"pow": hip.TF_POW, "hinge": hip.TF_HINGE, "inter": hip.TF_INTER}[kind]
    arg = {"pow": 3.0, "hinge": 20.1, "inter": 0.0}[kind]
    sentinel, pad = -12345.678, 64
    for n in LENGTHS:
        xbase = torch.from_numpy(np.concatenate([[777.0], x[:n]])).cuda()          # (addresses by hand: an empty slice has no pointer)
        obase = torch.from_numpy(np.concatenate([[777.0], other[:n]])).cuda()
        buf = torch.full((pad + n + pad,), sentinel, dtype=torch.float64, device="cuda")
        xptr, out = xbase.data_ptr() + 8, buf.data_ptr() + 8 * pad
        assert xptr % 16 == 8
        optr, ocode = (obase.data_ptr() + 8, hip.F64) if kind == "inter" else (None, 0)
        hip._check(lib.afhip_transform(xptr, hip.F64, n, code, arg, optr, ocode, out, hip.F64, hip._stream_ptr(xbase)))
        got = buf.cpu().numpy()
        expect = np.concatenate([np.full(pad, sentinel), want[:n], np.full(pad, sentinel)])
        assert np.all(nc.same_bits(got, expect)), (kind, n, np.flatnonzero(~nc.same_bits(got, expect))[:8])


# ---- 4. hinge and interact on special values ----
def test_hinge_and_interact_bit_for_bit(torch_cuda):
    """Every dtype combination numpy's rules produce — hinge float64 -> float64 and float32 -> float32 (a Python-float knot is weak), the product of
    float32 | float64 with float32 | float64 — on the special tables, bit for bit, signs of zeros and NaN placement included."""
    from aggfly_amd import hip
    torch = torch_cuda
    for dt in (np.float64, np.float32):
        for knot in nc.KNOTS:
            x = nc.hinge_inputs(knot, dt)
            want = nc.hinge_expected(x, knot, dt)
            got = hip.transform(torch.from_numpy(x).cuda(), "hinge", knot).cpu().numpy()
            assert got.dtype == want.dtype == dt
            assert np.all(nc.same_bits(got, want)), (dt.__name__, knot, x[~nc.same_bits(got, want)], got[~nc.same_bits(got, want)], want[~nc.same_bits(got, want)])
        x = nc.inter_inputs(dt)[0]
        for odt in (np.float64, np.float32):
            other = nc.inter_inputs(odt)[1]                          # the same pairs, each factor at its own precision's extremes
            res = np.result_type(dt, odt)
            want = nc.inter_expected(x, other, res)
            tdt = torch.float64 if res == np.float64 else torch.float32
            got = hip.transform(torch.from_numpy(x).cuda(), "inter", other=torch.from_numpy(other).cuda(), out_dtype=tdt).cpu().numpy()
            assert got.dtype == want.dtype == res
            miss = ~nc.same_bits(got, want)
            assert not miss.any(), (dt.__name__, np.dtype(odt).name, x[miss], other[miss], got[miss], want[miss])


# ---- 5. the power table through the fused kernels ----
PATTERNS = {"general": (1, 2, 3, 4, 24), "pair": (2,), "tri": (3,)}


def _group_cube(values, pattern):
    """values -> (cube [T, 1, CELLS], ib, G): one value per (group, cell), every group constant over its rows, group lengths cycling through
    `pattern`; the tail is padded with 1.0."""
    G = -(-len(values) // CELLS)
    G = -(-G // len(pattern)) * len(pattern)
    grid = np.ones(G * CELLS)
    grid[:len(values)] = values
    grid = grid.reshape(G, CELLS)
    lens = np.tile(pattern, G // len(pattern))
    cube = np.repeat(grid, lens, axis=0)
    return cube.reshape(cube.shape[0], 1, CELLS), np.concatenate([[0], np.cumsum(lens)]), G


def _fused_power_plans():
    """(form, exponents of one plan): the general form on every exponent, sixteen columns a plan; `_pair` on the negative ones and zero, `_pair_lean`
    on 1 .. 64 (the written-out chain, every leaf: x, x^2, x^3, x^4 and the loop), six a plan; the lean three-row form on the leaves and the loop at
    5, 33 and 64."""
    plans = []
    for i in range(0, len(nc.EXPONENTS), 16):
        plans.append(("general", nc.EXPONENTS[i:i + 16]))
    neg = [e for e in nc.EXPONENTS if e <= 0]
    pos = [e for e in nc.EXPONENTS if e >= 1]
    for i in range(0, len(neg), 6):
        plans.append(("pair", tuple(neg[i:i + 6])))
    for i in range(0, len(pos), 6):
        plans.append(("pair_lean", tuple(pos[i:i + 6])))
    plans.append(("tri_lean", (1, 2, 3, 4, 5, 33)))
    plans.append(("tri_lean", (64, 1)))
    return plans


def test_fused_power_table(torch_cuda):
    """The float64 power table laid out as [G groups x 70 cells] with constant groups: inner max returns x itself, the column's transform is x^e and
    the outer sum of one group gives cells[k, p, c] = 0.0 + x^e — expected exactly (a -0 becomes +0), by the fused kernels' contract.  One plan per
    group-end text and batch of exponents, its name asserted from describe()."""
    from aggfly_amd import hip
    torch = torch_cuda
    bad, names, rules = [], {}, {}
    for form, exps in _fused_power_plans():
        offsets, values = {}, []
        for e in exps:
            cases = nc.power_table(e)
            offsets[e] = (len(values), cases)
            values += [c.x for c in cases]
        cube, ib, G = _group_cube(np.array(values), PATTERNS[{"pair_lean": "pair", "tri_lean": "tri"}.get(form, form)])
        cols = [dict(inner="max", transform="pow", transform_arg=float(e), outer="sum") for e in exps]
        plan = hip.FusedPlan(cube.shape[0], CELLS, hip.F64, ib, np.arange(G + 1), cols, exact_order=True)
        got = plan.run_temporal(torch.from_numpy(cube).cuda()).cpu().numpy().reshape(len(exps), G * CELLS)
        name = _name(plan)
        names.setdefault(form, set()).add(name)
        if form == "general":
            assert "_pair" not in name, plan.describe()
        else:
            assert name.endswith({"pair": "_pair", "pair_lean": "_pair_lean", "tri_lean": "_pair_lean_tri"}[form]), plan.describe()
        for k, e in enumerate(exps):
            at, cases = offsets[e]
            for c, g in zip(cases, got[k, at:at + len(cases)]):
                rule = nc.fused_power_rule(c.x, e)
                tally = rules.setdefault(rule, [0, 0])
                tally[0] += 1
                if not nc.fused_power_ok(c.x, e, float(g)):
                    bad.append((form, name, e, c.name, c.x, float(g), c.exact, rule))
                elif not (nc.same_bits(g, 0.0 + c.exact) or (g == 0.0 and c.exact == 0.0)):
                    tally[1] += 1
        assert np.all(got[:, len(values):] == 1.0)                                       # the padding: 1^e
    _record("fused_pow", {"variants": {k: sorted(v) for k, v in names.items()}, "outside_contract": len(bad),
                          "cases_and_not_the_exact_value_by_rule": {k: tuple(v) for k, v in rules.items()}})
    assert not bad, (len(bad), bad[:12])
    assert set(names) == {"general", "pair", "pair_lean", "tri_lean"}
    # cases and results that are not bit for bit 0.0 + RN(x^e), per sentence of the contract (profiles/numerics_exact.txt, section 4): asserted
    assert {k: tuple(v) for k, v in rules.items()} == {"class": (45212, 2884), "one-ulp": (9044, 510), "brink": (434, 28), "zero": (7768, 2340),
                                                       "reciprocal": (4388, 704)}, rules


PACKED_EXPONENTS = (-63, -52, -9, 9, 33, 64)
PACKED_STORED = (1, -1, 0, 2, -2, 3, -3, 7, -7, 181, -256, 32767, -32768, 4)          # the stored int16 of a row of cells, repeated along it


def _packed_multipliers():
    """The float32 multipliers of the packed cube, one unpack rule each: a stored q reads as (float)q * mul in float32, so q = +-1 reaches +-mul —
    any float32 — and the other q its small multiples.  Powers of two over the float32 range; for every exponent of the plan the float32 table's
    neighbourhoods of the overflow, normal and zero roots, the band of finding 1 and the inputs of finding 2 (2^20 for e = -52 among them); and
    -1.0, under which a stored 0 reads as -0."""
    muls = {math.ldexp(1.0, k) for k in (-126, -120, -100, -64, -30, -17, -16, -1, 0, 1, 16, 17, 20, 25, 64, 100, 127)}
    for e in PACKED_EXPONENTS:
        for c in nc.power_table(e, np.float32):
            kind = c.name[1:].split("/")[0]
            if c.name[0] == "+" and kind in ("overflow-root", "normal-root", "zero-root", "f32-overflow-root", "overflown-power", "underflown-power") \
                    and 2.0 ** -126 <= c.x < 2.0 ** 112:                       # (a normal float32, and 32768 * mul stays finite)
                muls.add(c.x)
    return sorted(muls) + [-1.0]


@pytest.mark.parametrize("storage", ["int16", "float32"])
def test_fused_power_table_packed_and_float32(torch_cuda, storage):
    """The fused kernels' other instantiations on the values a packed cube reaches: an int16 cube with one unpack rule per group — x = (float)q * mul,
    rounded to float32 — through a `PackedI16` kernel, and the same float32 values through a float32 one.  Constant groups, inner max, x^e, outer sum
    of one group, `exact_order`; held to the fused kernels' contract (`fused_power_ok`), with the cases of finding 1 ("zero"), of finding 2 (a finite
    x whose power is -inf), powers of two and zeros of both signs counted."""
    import aggfly_amd as af
    from aggfly_amd import hip
    torch = torch_cuda
    muls = _packed_multipliers()
    G = -(-len(muls) // 5) * 5
    muls = muls + [1.0] * (G - len(muls))
    lens = np.tile(PATTERNS["general"], G // 5)
    ib = np.concatenate([[0], np.cumsum(lens)])
    q_row = np.resize(np.array(PACKED_STORED, dtype=np.int16), CELLS)
    q = np.tile(q_row, (int(ib[-1]), 1)).reshape(-1, 1, CELLS)
    with np.errstate(all="ignore"):
        values = np.stack([q_row.astype(np.float32) * np.float32(m) + np.float32(-0.0) for m in muls])      # [G, CELLS] float32: the unpack rule
    assert muls[len(_packed_multipliers()) - 1] == -1.0 and np.signbit(values[len(_packed_multipliers()) - 1][2])      # a stored 0 under mul = -1: -0
    cols = [dict(inner="max", transform="pow", transform_arg=float(e), outer="sum") for e in PACKED_EXPONENTS]
    if storage == "int16":
        d = torch.from_numpy(q).cuda()
        cube = af.PackedCube.concat([af.PackedCube(d[lo:hi], _pairs=[(np.float32(m), None)]) for m, lo, hi in zip(muls, ib[:-1], ib[1:])])
        assert np.all(nc.same_bits(cube.materialize().cpu().numpy().reshape(-1, CELLS)[ib[:-1]].astype(np.float64), values.astype(np.float64)))
        plan = hip.FusedPlan(int(ib[-1]), CELLS, hip.I16, ib, np.arange(G + 1), cols, exact_order=True)
        plan.bind_packing(cube)
    else:
        cube = torch.from_numpy(np.repeat(values, lens, axis=0).reshape(-1, 1, CELLS)).cuda()
        plan = hip.FusedPlan(int(ib[-1]), CELLS, hip.F32, ib, np.arange(G + 1), cols, exact_order=True)
    got = plan.run_temporal(cube).cpu().numpy()
    name = _name(plan)
    assert name.startswith("i16_" if storage == "int16" else "f32_") and "_pair" not in name, plan.describe()
    bad, verdicts, tally = [], {}, {"zero": 0, "finding-2": 0, "power-of-two": 0, "zero-in": 0, "reciprocal": 0, "class": 0, "one-ulp": 0, "brink": 0}
    for k, e in enumerate(PACKED_EXPONENTS):
        for g in range(G):
            for c in range(CELLS):
                x, r = float(values[g, c]), float(got[k, g, c])
                key = (e, x.hex(), r.hex())
                if key not in verdicts:
                    exact = nc.exact_power(x, e)
                    rule = nc.fused_power_rule(x, e)
                    verdicts[key] = nc.fused_power_ok(x, e, r)
                    tally[rule] += 1
                    tally["finding-2"] += exact == -math.inf and x != 0.0
                    tally["power-of-two"] += x != 0.0 and math.frexp(abs(x))[0] == 0.5
                    tally["zero-in"] += x == 0.0
                    if not verdicts[key]:
                        bad.append((name, e, x, r, exact, rule))
    _record(f"fused_pow_{storage}", {"variant": name, "distinct_cases": len(verdicts), "outside_contract": len(bad), "by_rule": tally})
    assert not bad, (len(bad), bad[:12])
    assert tally["zero"] >= 40 and tally["finding-2"] >= 40 and tally["power-of-two"] >= 100 and tally["zero-in"] >= 12 and tally["class"] >= 1000, tally


# ---- 6. means ----
def _mean_plan_run(torch, hip, cube, ib, ob, cols):
    plan = hip.FusedPlan(cube.shape[0], cube.shape[2], hip.F64, ib, ob, cols, exact_order=True)
    return plan.run_temporal(torch.from_numpy(np.ascontiguousarray(cube)).cuda()).cpu().numpy(), _name(plan)


def _check_means(got, cases, where, bad, missed):
    for c, g in zip(cases, got):
        want = 0.0 + c.exact                                                             # the outer sum of one group starts at +0.0
        if c.cls == "exact":
            ok = bool(nc.same_bits(g, want)) or (g == 0.0 and want == 0.0)
        else:
            ok = abs(g - want) <= nc.STEP64 and (g == 0.0 or (g < 0) == (c.s < 0))
            missed[0] += ok and g != want
        if not ok:
            bad.append((where, c.name, c.n, c.s, float(g), c.exact, c.cls))


def test_inner_means_against_exact_quotients(torch_cuda):
    """The mean table through `inner="mean"`, no transform, outer sum of one group: group lengths 1 .. 48 as the ragged groups of one cube (the general
    form: div_by(s, n, RN(1 / n))), and uniform groups of two, three and four rows and mixed one- to four-row groups in the lean short-group forms
    (s / 2 and s / 4 by a multiply, s / 3 and the mixed lengths by div_by).  `exact` cases bit for bit, `step` cases within 2^-1074."""
    from aggfly_amd import hip
    torch = torch_cuda
    bad, missed, names = [], [0], {}
    tables = {n: nc.mean_cases(n) for n in nc.MEAN_LENGTHS}
    C = max(len(t) for t in tables.values())
    C += C % 2
    # the general form: one group per length
    rows = []
    for n, cases in tables.items():
        block = np.zeros((n, C))
        for j, c in enumerate(cases):
            block[:, j] = c.rows
        rows.append(block)
    cube = np.concatenate(rows).reshape(-1, 1, C)
    ib = np.concatenate([[0], np.cumsum(nc.MEAN_LENGTHS)])
    got, name = _mean_plan_run(torch, hip, cube, ib, np.arange(len(ib)), [dict(inner="mean", outer="sum")])
    names["general"] = name
    assert "_pair" not in name
    for g, (n, cases) in enumerate(tables.items()):
        _check_means(got[0, g, :len(cases)], cases, f"general n={n}", bad, missed)
    # the lean short-group forms: two groups a cube, the second with its rows in reverse order; a max column beside the mean keeps the plan on them
    cols = [dict(inner="mean", outer="sum"), dict(inner="max", outer="sum")]
    for form, lens, suffix in (("pair", (2, 2), "_pair_lean"), ("tri", (3, 3), "_pair_lean_tri"), ("quad", (4, 4), "_pair_lean_quad"), ("rag", (1, 2, 3, 4, 4, 3, 2, 1), "_pair_lean_rag")):
        blocks = []
        for i, n in enumerate(lens):
            block = np.zeros((n, C))
            for j, c in enumerate(tables[n]):
                block[:, j] = c.rows[::-1] if i >= len(lens) // 2 else c.rows
            blocks.append(block)
        cube = np.concatenate(blocks).reshape(-1, 1, C)
        ib = np.concatenate([[0], np.cumsum(lens)])
        got, name = _mean_plan_run(torch, hip, cube, ib, np.arange(len(ib)), cols)
        names[form] = name
        assert name.endswith(suffix), name
        for g, n in enumerate(lens):
            _check_means(got[0, g, :len(tables[n])], tables[n], f"{form} n={n}", bad, missed)
    _record("inner_means", {"variants": names, "outside_bound": len(bad), "step_cases_one_step_off": missed[0]})
    assert not bad, (len(bad), bad[:12])
    assert missed[0] == 100, missed                    # (profiles/numerics_exact.txt, section 4: every one an exact tie)


def test_outer_mean_against_exact_quotients(torch_cuda):
    """`outer="mean"` over 1, 2, 3, 5, 7, 12 and 31 single-row groups whose values add up exactly: the period's sum divided by its group count, held to
    the exact quotient by the same classes."""
    from aggfly_amd import hip
    torch = torch_cuda
    counts = (1, 2, 3, 5, 7, 12, 31)
    tables = {m: nc.mean_cases(m) for m in counts}
    C = max(len(t) for t in tables.values())
    C += C % 2
    rows = []
    for m, cases in tables.items():
        block = np.zeros((m, C))
        for j, c in enumerate(cases):
            block[:, j] = c.rows
        rows.append(block)
    cube = np.concatenate(rows).reshape(-1, 1, C)
    T = cube.shape[0]
    ob = np.concatenate([[0], np.cumsum(counts)])
    bad, missed = [], [0]
    for inner in ("mean", "max"):                                # (one-row groups: either statistic is the row itself)
        got, name = _mean_plan_run(torch, hip, cube, np.arange(T + 1), ob, [dict(inner=inner, outer="mean")])
        for p, (m, cases) in enumerate(tables.items()):
            _check_outer(got[0, p, :len(cases)], cases, f"{inner} m={m}", bad, missed)
    _record("outer_mean", {"outside_bound": len(bad), "step_cases_one_step_off": missed[0]})
    assert not bad, (len(bad), bad[:12])
    assert missed[0] == 0                              # a true division: every `step` case is the exact quotient


def _check_outer(got, cases, where, bad, missed):
    for c, g in zip(cases, got):
        if c.cls == "exact":
            ok = bool(nc.same_bits(g, c.exact)) or (g == 0.0 and c.exact == 0.0)
        else:
            ok = abs(g - c.exact) <= nc.STEP64 and (g == 0.0 or (g < 0) == (c.s < 0))
            missed[0] += ok and g != c.exact
        if not ok:
            bad.append((where, c.name, c.n, c.s, float(g), c.exact, c.cls))
