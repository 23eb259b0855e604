"""Packed cubes on the region-fused period ends (gen_variants.py: packed_rf_menu; afhip_planner.cpp: twin_of, choose_packed_variant,
choose_packed_short_variant, rf_plan_ok): every twin of the loaded build on the plan of `packed_rf_recipes`, and once each: unpack rules
that change inside a period, uint16 storage, cells in up to five regions, regions of a handful of cells, the launch shape, and the rule
that chooses the cells per lane.

Per twin (`test_twin_against_the_per_cell_routes_the_float32_twin_and_the_oracle`):
  (a) `describe()` names the plain kernel, the library holds its `_rf` twin, and the run reports `last-run=region-fused`;
  (b) num / den / res against the same plan created under AFHIP_NO_PACKED_RF=1 (the per-cell routes, no "region-fused" in its
      `describe()`): rtol 1e-12, atol 1e-9 on num — the bars of tests/test_gpu_kernels.py for the float twins;
  (c) against a float32 plan on the unpacked cube on ITS region-fused route: past the unpack the packed kernel is the float32
      instantiation, the table and the lane order are the same, so where both plans run the same cells per lane the sums must agree in
      every bit (`_same_bits`); 1e-12 where the widths differ (light float32 plans and plans with four threshold slots take one cell per
      lane where the packed plan takes two: afhip_planner.cpp, load_path).  A sine_dd column on a kernel of another form — the general
      kernel's table acos against the pair forms' table of cubics — would differ by its own 1e-10; no such pair of plans occurs here
      (every packed short-group form with a sine column has its float32 form), and the test says so before it compares;
  (d) den at 1e-12 and num at 1e-12 + 1e-9 against the oracle's spatial stage (`oracle.ref_spatial.spatial_num_den`) on the plan's own
      per-cell values (`want_cells=True`, which must not report a region-fused run);
  (e) the empty period is NaN with den == 0.
"""
import functools
import re
import zlib

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import synth
from oracle.ref_spatial import spatial_num_den

import packed_recipes as pr
import packed_rf_recipes as prf
import variant_recipes as vr
import test_gpu_packed_rules as rules_mod
import test_gpu_unsigned as uns

pytestmark = pytest.mark.gpu

KIND = vr.loaded_menu_kind()
MENU = [vr.variant(t) for t in prf.menu_of(KIND)]
BY_NAME = {v.name: v for v in MENU}
KNOB = "AFHIP_NO_PACKED_RF"
RTOL, ATOL_NUM = 1e-12, 1e-9


def _same_bits(got, want, msg=""):
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, msg
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), msg
    assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]), msg


def _close(got, want, msg=""):
    for key in ("num", "den", "res"):
        np.testing.assert_allclose(got[key], want[key], rtol=RTOL, atol=ATOL_NUM if key == "num" else 0, equal_nan=True, err_msg=f"{msg} {key}")


def _np(out):
    return {k: out[k].cpu().numpy() for k in ("num", "den", "res")}


@functools.lru_cache(maxsize=None)
def _table(nx):
    from aggfly_amd import hip
    tab = synth.weights_table(prf.NY, nx, 40, seed=41, zero_frac=0.05)
    C = prf.NY * nx
    ridx, cidx, w = tab["index_right"].to_numpy(), tab["cell_id"].to_numpy(), tab["weight"].to_numpy()
    nR = int(ridx.max()) + 1
    assert tab.groupby("cell_id").size().max() == 2                  # border cells belong to two regions
    assert (tab.groupby("index_right")["weight"].sum() == 0).any()   # zero-weight regions
    return tab, hip.CSR(ridx, cidx, w, nR, C), nR


def _i16_cube(torch, q, pairs=pr.PAIRS, fill=pr.FILL):
    T, C = q.shape
    cube = af.PackedCube(torch.from_numpy(q.reshape(T, 1, C)).cuda(), scale_factor=pairs[0][0], add_offset=pairs[0][1], fill_value=fill)
    for m, a in pairs[1:]:
        cube = cube * m if m is not None else cube
        cube = cube + a if a is not None else cube                   # the preprocess fold: K -> deg C
    assert isinstance(cube, af.PackedCube) and cube.n_pairs == len(pairs)
    return cube


def _packed_plan(r, cube, monkeypatch=None, knob=False, **kw):
    from aggfly_amd import hip
    if knob:
        monkeypatch.setenv(KNOB, "1")
    plan = hip.FusedPlan(r.T, r.n_cells, hip._dtype_code(cube), r.inner_bounds, kw.pop("ob", r.outer_bounds), kw.pop("cols", r.columns), **kw)
    if knob:
        monkeypatch.delenv(KNOB)
    plan.bind_packing(cube)
    return plan


def _float_plan(r, **kw):
    from aggfly_amd import hip
    return hip.FusedPlan(r.T, r.n_cells, hip.F32, r.inner_bounds, kw.pop("ob", r.outer_bounds), kw.pop("cols", r.columns), **kw)


def _vec_of(plan):
    return int(re.search(r" vec=(\d+) ", plan.describe()).group(1))


def _form_of(name):
    """The form suffixes of a kernel name, storage, width and rows in flight aside."""
    return re.sub(r"^(f32|i16)_p0_v\d_|_d\d+(?=_)", "", name)


def _assert_twin_in_library(plan):
    name = vr.plan_name(plan)
    twins = [v.name for v in MENU if re.sub(r"_d\d+_", "_d_", v.name) == re.sub(r"_d\d+_", "_d_", name) + "_rf"]
    assert len(twins) == 1, (name, plan.describe())
    return twins[0]


def _against_float32(name, r, got, values, csr, same_width_only=False):
    """(c) of the module docstring; returns whether the compare was bit for bit."""
    f32 = _float_plan(r)
    want = _np(f32.run(values, csr))
    assert "last-run=region-fused" in f32.describe(), f32.describe()
    sine = any(c["inner"] == "sine_dd" for c in r.columns)
    assert not sine or _form_of(vr.plan_name(f32)) == _form_of(r.name), (f32.describe(), r.name)
    same = _vec_of(f32) == BY_NAME[name].vec
    if same:
        for key in ("num", "den", "res"):
            _same_bits(got[key], want[key], f"{name} against {vr.plan_name(f32)}: {key}")
    else:
        assert not same_width_only, f32.describe()
        _close(got, want, f"{name} against {vr.plan_name(f32)}")
    return same


BIT_FOR_BIT = {}


# ---- 1. every twin of the loaded build ----
@pytest.mark.parametrize("name", [v.name for v in MENU])
def test_twin_against_the_per_cell_routes_the_float32_twin_and_the_oracle(torch_cuda, monkeypatch, name):
    v = BY_NAME[name]
    r = prf.recipe(v)
    tab, csr, nR = _table(prf.NX[v.vec])
    q = prf.stored_cube(r, seed=zlib.crc32(name.encode()))
    cube = _i16_cube(torch_cuda, q)
    K, P = len(r.columns), len(r.outer_bounds) - 1
    # (a)
    plan = _packed_plan(r, cube)
    assert vr.plan_name(plan) == r.name and "storage=int16" in plan.describe() and "region-fused-capable" in plan.describe(), plan.describe()
    assert _assert_twin_in_library(plan) == name
    got = _np(plan.run(cube, csr))
    assert "last-run=region-fused" in plan.describe(), plan.describe()
    # (b)
    plain = _packed_plan(r, cube, monkeypatch, knob=True)
    assert vr.plan_name(plain) == r.name and "region-fused" not in plain.describe(), plain.describe()
    _close(got, _np(plain.run(cube, csr)), f"{name} against the per-cell route")
    assert "region-fused" not in plain.describe(), plain.describe()
    # (c)
    values = cube.materialize()
    np.testing.assert_array_equal(values.cpu().numpy().reshape(r.T, r.n_cells), pr.np_unpack(q))
    BIT_FOR_BIT[name] = _against_float32(name, r, got, values, csr)
    # (d)
    with_cells = plan.run(cube, csr, want_cells=True)
    assert "last-run=region-fused" not in plan.describe(), plan.describe()
    cells = with_cells["cells"].cpu().numpy()                        # [K, P, C]
    nums, den, _ = spatial_num_den({f"k{k}": cells[k].T for k in range(K)}, tab, np.arange(r.n_cells))
    np.testing.assert_allclose(got["den"], den, rtol=RTOL)
    for k in range(K):
        np.testing.assert_allclose(got["num"][k], nums[f"k{k}"], rtol=RTOL, atol=ATOL_NUM, err_msg=f"{name} column {k}: {r.columns[k]}")
    # (e) ... and something to compare elsewhere
    assert np.isnan(got["res"][:, :, 1]).all() and (got["den"][:, 1] == 0).all()
    assert np.isfinite(got["res"][:, :, [0] + list(range(2, P))]).mean() > 0.5


def test_the_cases_cover_the_loaded_builds_menu_and_reach_the_bit_compare(torch_cuda):
    from aggfly_amd import hip
    assert hip.menu_size(prf.KEY) == len(MENU) == len(BY_NAME)
    if KIND == "dev":
        return
    assert len(MENU) == 61 and {v.form for v in MENU} == {"", "pair", "quad", "tri", "rag"} and {v.vec for v in MENU} == {1, 2}
    # a general and a short-group twin whose float32 plan runs the same cells per lane (run here if the cases above did not)
    for name in ("i16_p0_v2_s1_t1_k6_d16_nt_rf", "i16_p0_v2_s2_t0_k6_d8_nt_pair_lean_quad_rf"):
        if name not in BIT_FOR_BIT:
            v = BY_NAME[name]
            r = prf.recipe(v)
            cube = _i16_cube(torch_cuda, prf.stored_cube(r, seed=zlib.crc32(name.encode())))
            csr = _table(prf.NX[v.vec])[1]
            BIT_FOR_BIT[name] = _against_float32(name, r, _np(_packed_plan(r, cube).run(cube, csr)), cube.materialize(), csr, same_width_only=True)
        assert BIT_FOR_BIT[name], name


# ---- 2. once each ----
RULE_TWINS = ["i16_p0_v2_s1_t1_k6_d16_nt_rf", "i16_p0_v2_s2_t0_k6_d8_nt_pair_lean_quad_rf"]


@pytest.mark.parametrize("name", RULE_TWINS)
def test_unpack_rules_that_change_inside_a_period(torch_cuda, monkeypatch, name):
    """Two unpack rules (different scale, offset and fill) whose bound falls inside a period, inside an inner group and, for the general
    kernel, inside a burst of rows: the rule of a row is picked in `consume`, before the period end sees a value."""
    if name not in BY_NAME:
        pytest.fail(f"the loaded build has no {name}")
    v = BY_NAME[name]
    r = prf.recipe(v)
    ib, ob = r.inner_bounds, r.outer_bounds
    change = int(ib[ob[4]] + (ib[ob[4] + 1] - ib[ob[4]]) // 2 + 1)       # inside the first group of period 4
    assert ib[ob[4]] < change < ib[ob[4] + 1] and ob[4] < ob[5]
    bounds = [0, change, r.T]
    shapes = rules_mod._rule_shapes(False)
    rules = [shapes[0], shapes[1]]
    assert rules[0] != rules[1]
    bits = rules_mod._stored(r.T, r.n_cells, bounds, rules, seed=zlib.crc32(name.encode()) & 0xffff)
    cube = rules_mod._cube(torch_cuda, bits.reshape(r.T, 1, r.n_cells), rules, bounds, False)
    assert cube.n_rules == 2 and cube.rule_bounds == bounds
    csr = _table(prf.NX[v.vec])[1]
    plan = _packed_plan(r, cube)
    got = _np(plan.run(cube, csr))
    assert vr.plan_name(plan) == r.name and "last-run=region-fused" in plan.describe(), plan.describe()
    plain = _packed_plan(r, cube, monkeypatch, knob=True)
    _close(got, _np(plain.run(cube, csr)), name)
    assert "region-fused" not in plain.describe(), plain.describe()
    assert np.isfinite(got["res"]).mean() > 0.3
    assert _against_float32(name, r, got, cube.materialize(), csr, same_width_only=True)


def test_uint16_storage_takes_the_same_twins(torch_cuda, monkeypatch):
    from aggfly_amd import hip
    name = "i16_p0_v2_s1_t1_k6_d16_nt_rf"
    if name not in BY_NAME:
        pytest.fail(f"the loaded build has no {name}")
    v = BY_NAME[name]
    r = prf.recipe(v)
    r.columns = uns._snap_columns(r.columns)
    fill = 65535
    rng = np.random.default_rng(7)
    q = np.clip(np.rint(uns.stored_near(12.0) + rng.normal(0.0, 9.0, (r.T, r.n_cells)) / uns.PAIRS[0][0]), 0, 65534).astype(np.uint16)
    q.reshape(-1)[rng.choice(q.size, 120, replace=False)] = np.array([0, 65534, 1, 32767, 32768, 65533] * 20, dtype=np.uint16)
    ib = r.inner_bounds
    for g in range(0, 60, 5):
        q[ib[g], rng.choice(r.n_cells, 25, replace=False)] = fill
    q[:, [3, r.n_cells // 2, r.n_cells - 1]] = fill
    cube = uns._cuda_cube(torch_cuda, q.reshape(r.T, 1, r.n_cells), scale_factor=uns.PAIRS[0][0], add_offset=uns.PAIRS[0][1], fill_value=fill) - 273.15
    assert hip._dtype_code(cube) == hip.U16 and (q > 32767).mean() > 0.05
    csr = _table(prf.NX[v.vec])[1]
    plan = _packed_plan(r, cube)
    got = _np(plan.run(cube, csr))
    assert vr.plan_name(plan) == r.name and "storage=uint16" in plan.describe() and "last-run=region-fused" in plan.describe(), plan.describe()
    plain = _packed_plan(r, cube, monkeypatch, knob=True)
    _close(got, _np(plain.run(cube, csr)), name)
    assert "region-fused" not in plain.describe(), plain.describe()
    values = cube.materialize()
    np.testing.assert_array_equal(values.cpu().numpy().reshape(r.T, r.n_cells), uns.np_unpack(q, uns.PAIRS, fill))
    assert _against_float32(name, r, got, values, csr, same_width_only=True)


def test_cells_in_up_to_five_regions_and_regions_of_a_few_cells(torch_cuda, monkeypatch):
    """The "extras" of tests/test_gpu_kernels.py (cells that sit in three, four and five regions: the run tables hold two entries per
    cell, k_rf_reduce adds the rest from values those cells write on the side) and a table of 2,500 regions of three or four cells."""
    from aggfly_amd import hip
    name = "i16_p0_v2_s1_t1_k6_d16_nt_rf"
    if name not in BY_NAME:
        pytest.fail(f"the loaded build has no {name}")
    v = BY_NAME[name]
    r = prf.recipe(v)
    C, K = r.n_cells, len(r.columns)
    tab, csr, nR = _table(prf.NX[v.vec])
    q = prf.stored_cube(r, seed=5)
    cube = _i16_cube(torch_cuda, q)
    ridx, cidx, w = tab["index_right"].to_numpy(), tab["cell_id"].to_numpy(), tab["weight"].to_numpy()
    rj = np.random.default_rng(46)
    jc = rj.choice(C, 300, replace=False)
    jc[0] = 3                                                            # an ocean cell
    more_c = np.repeat(jc, rj.integers(1, 4, 300))
    more_r = rj.integers(0, nR, len(more_c))
    r3 = np.concatenate([ridx, more_r]); c3 = np.concatenate([cidx, more_c]); w3 = np.concatenate([w, rj.uniform(0.05, 0.9, len(more_c))])
    keep = ~pd.DataFrame({"r": r3, "c": c3}).duplicated().to_numpy()
    r3, c3, w3 = r3[keep], c3[keep], w3[keep]
    o3 = np.argsort(r3, kind="stable")
    assert np.bincount(c3).max() >= 4 and (q[:, 3] == pr.FILL).all()
    jtab = pd.DataFrame({"index_right": r3[o3], "cell_id": c3[o3], "weight": w3[o3]})
    tiny = synth.weights_table(prf.NY, prf.NX[v.vec], 2500, seed=44)
    assert len(tiny) / (int(tiny["index_right"].max()) + 1) < 8
    plan = _packed_plan(r, cube)
    plain = _packed_plan(r, cube, monkeypatch, knob=True)
    cells = plan.run(cube, csr, want_cells=True)["cells"].cpu().numpy()
    for label, t in (("extras", jtab), ("tiny", tiny)):
        tcsr = hip.CSR(t["index_right"].to_numpy(), t["cell_id"].to_numpy(), t["weight"].to_numpy(), int(t["index_right"].max()) + 1, C)
        got = _np(plan.run(cube, tcsr))
        assert "last-run=region-fused" in plan.describe(), plan.describe()
        _close(got, _np(plain.run(cube, tcsr)), label)
        assert "region-fused" not in plain.describe()
        nums, den, _ = spatial_num_den({f"k{k}": cells[k].T for k in range(K)}, t, np.arange(C))
        np.testing.assert_allclose(got["den"], den, rtol=RTOL)
        for k in range(K):
            np.testing.assert_allclose(got["num"][k], nums[f"k{k}"], rtol=RTOL, atol=ATOL_NUM, err_msg=f"{label} column {k}")
        f32 = _float_plan(r)
        want = _np(f32.run(cube.materialize(), tcsr))
        assert "last-run=region-fused" in f32.describe() and _vec_of(f32) == 2, f32.describe()
        for key in ("num", "den", "res"):
            _same_bits(got[key], want[key], f"{label} {key}")


def test_sums_do_not_depend_on_the_launch_shape(torch_cuda, monkeypatch):
    """Four-wave workgroups, a caller-owned workspace, run sums laid slot-major or run-major: the same bits
    (tests/test_gpu_kernels.py: test_region_fused_sums_do_not_depend_on_the_launch_shape, on a packed cube)."""
    name = "i16_p0_v2_s1_t1_k6_d16_nt_rf"
    if name not in BY_NAME:
        pytest.fail(f"the loaded build has no {name}")
    v = BY_NAME[name]
    r = prf.recipe(v)
    csr = _table(prf.NX[v.vec])[1]
    cube = _i16_cube(torch_cuda, prf.stored_cube(r, seed=9))

    def run(env, workspace=False):
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        plan = _packed_plan(r, cube)
        for k in env:
            monkeypatch.delenv(k)
        ws = torch_cuda.empty(plan.workspace_bytes(csr), dtype=torch_cuda.uint8, device="cuda") if workspace else "library"
        out = plan.run(cube, csr, workspace=ws)
        assert vr.plan_name(plan) == r.name and "last-run=region-fused" in plan.describe(), plan.describe()
        return plan.describe(), _np(out)

    base_desc, base = run({})
    assert "wg=64" in base_desc, base_desc
    for env, ws, must in (({"AFHIP_FORCE_WG": "256"}, False, "wg=256"), ({}, True, "(caller-owned)"), ({"AFHIP_RF_LAYOUT": "run"}, False, "wg=64"),
                          ({"AFHIP_RF_LAYOUT": "slot"}, True, "wg=64")):
        desc, got = run(env, ws)
        assert must in desc, desc
        for k in base:
            _same_bits(got[k], base[k], f"{env} {k}")


# ---- 3. the cells per lane ----
def _width_case(form):
    """An eligible plan of thirteen periods on 72 x 130 = 9,360 cells, a multiple of four: (the two-cell twin, its recipe on that grid, the
    four-cell kernel such rows took before the twins)."""
    name = {"general": "i16_p0_v2_s1_t1_k6_d16_nt_rf", "quad": "i16_p0_v2_s1_t0_k6_d8_nt_pair_lean_quad_rf"}[form]
    if name not in BY_NAME:
        pytest.fail(f"the loaded build has no {name}")
    r = prf.recipe(BY_NAME[name])
    r.n_cells = 72 * 130
    r.outer_bounds = np.array([0, 5, 5, 10, 15, 20, 25, 30, 35, 40, 45, 50, 55, 60], dtype=np.int64)
    return name, r, r.name.replace("_v2_", "_v4_").replace("_d16_", "_d8_")


@pytest.mark.parametrize("form", ["general", "quad"])
def test_rows_of_a_multiple_of_four_take_two_cells_per_lane_for_the_route(torch_cuda, monkeypatch, form):
    from aggfly_amd import hip
    name, r, four = _width_case(form)
    assert r.n_cells % 4 == 0 and len(r.outer_bounds) - 1 == 13
    tab = synth.weights_table(72, 130, 40, seed=41, zero_frac=0.05)
    csr = hip.CSR(tab["index_right"].to_numpy(), tab["cell_id"].to_numpy(), tab["weight"].to_numpy(), int(tab["index_right"].max()) + 1, r.n_cells)
    cube = _i16_cube(torch_cuda, prf.stored_cube(r, seed=3))
    plan = _packed_plan(r, cube)
    assert vr.plan_name(plan) == r.name and "_v2_" in r.name and "region-fused-capable" in plan.describe(), plan.describe()
    got = _np(plan.run(cube, csr))
    assert "last-run=region-fused" in plan.describe(), plan.describe()
    # what is not a candidate for the route keeps the kernel it had before the twins (the plan under the knob): a four-cell one, and
    # no such plan says "region-fused"
    rounded = [dict(c) for c in r.columns]
    rounded[-1]["rounding"] = hip.ROUND_FINAL
    others = {
        "exact_order": dict(exact_order=True),
        "one_period": dict(ob=np.array([0, 60], dtype=np.int64)),
        "seven_periods": dict(ob=np.array([0, 9, 9, 20, 30, 40, 50, 60], dtype=np.int64)),
        "round_final": dict(cols=rounded),
        "knob": {},
    }
    if form == "general":                                                # thirteen columns: the sixteen-column kernels have no twin (and none at four cells)
        others["thirteen_columns"] = dict(cols=pr._snap_columns([dict(inner="dd", inner_args=(float(t), float(t) + 7, 0), outer="sum") for t in range(-10, 29, 3)]))
    for label, kw in others.items():
        parent = _packed_plan(r, cube, monkeypatch, knob=True, **dict(kw))
        p = parent if label == "knob" else _packed_plan(r, cube, **dict(kw))
        assert vr.plan_name(p) == vr.plan_name(parent) and "region-fused" not in p.describe() and "region-fused" not in parent.describe(), (label, p.describe())
        assert ("_k16_" in vr.plan_name(p)) if label == "thirteen_columns" else ("_v4_" in vr.plan_name(p)), (label, p.describe())
        if label == "knob":
            assert vr.plan_name(p) == four, p.describe()
            knob_plan = p
    monkeypatch.setenv("AFHIP_NO_REGION_FUSED", "1")
    off = _packed_plan(r, cube)
    monkeypatch.delenv("AFHIP_NO_REGION_FUSED")
    assert vr.plan_name(off) == four and "region-fused" not in off.describe(), off.describe()
    # the four-cell kernel's numbers are the route's to rounding
    knob = _np(knob_plan.run(cube, csr))
    assert "region-fused" not in knob_plan.describe()
    _close(got, knob, form)


def test_share_thresholds_of_packed_plans(torch_cuda):
    """Plan creation only.  The light two-row forms take the route from period values of 10 % of a packed cube's bytes (sine_dd from pairs:
    2 K / g with g groups a period), and a short-group plan gives up a four-cell kernel for a twin from 25 % (6-hourly polynomial: K / g);
    profiles/packed_region_fused.txt has the measurement behind both."""
    from aggfly_amd import hip
    sine = [dict(inner="sine_dd", inner_args=(10.0, 30.0, 0.0), outer="sum")]
    poly = [dict(inner="mean", transform="pow", transform_arg=float(e), outer="sum") for e in (1, 2, 3, 4)]

    def plan(rows, groups, per, cols, n_cells):
        ib = np.arange(0, rows * groups + 1, rows, dtype=np.int64)
        return hip.FusedPlan(rows * groups, n_cells, hip.I16, ib, np.arange(0, groups + 1, per, dtype=np.int64), cols).describe()

    monthly, fortnightly = plan(2, 240, 30, sine, 71 * 130), plan(2, 240, 15, sine, 71 * 130)           # shares 0.067 and 0.133
    assert "_v2_" in monthly and "_pair_ss" in monthly and "region-fused" not in monthly, monthly
    assert "_v2_" in fortnightly and "_pair_ss" in fortnightly and "region-fused-capable" in fortnightly, fortnightly
    for n_cells, vec, route in ((72 * 130, 4, False), (71 * 130, 2, True)):                               # share 0.133, eight periods
        d = plan(4, 240, 30, poly, n_cells)
        assert f"_v{vec}_" in d and "_pair_lean_quad" in d and ("region-fused-capable" in d) == route and ("region-fused" in d) == route, d
    d = plan(4, 240, 10, poly, 72 * 130)                                                                  # share 0.4
    assert "_v2_" in d and "_pair_lean_quad" in d and "region-fused-capable" in d, d


def test_bins_plans_keep_their_histogram_kernels(torch_cuda, monkeypatch):
    """Six contiguous 5-degree bins per day, summed by period: the LDS-histogram menus are untouched by the rule and have no twins."""
    name = "i16_p0_v2_s1_t1_k6_d16_nt_rf"
    if name not in BY_NAME:
        pytest.fail(f"the loaded build has no {name}")
    r = prf.recipe(BY_NAME[name])
    r.n_cells = 72 * 130
    cols = [dict(inner="bins", inner_args=(-5.0 + 5.0 * i, 5.0 * i, 0.0), outer="sum") for i in range(6)]
    cube = _i16_cube(torch_cuda, prf.stored_cube(r, seed=4))
    plan = _packed_plan(r, cube, cols=cols)
    parent = _packed_plan(r, cube, monkeypatch, knob=True, cols=cols)
    assert "_hist" in vr.plan_name(plan) and vr.plan_name(plan) == vr.plan_name(parent) and "region-fused" not in plan.describe(), plan.describe()
