"""Packed cubes' short-group plans on the lean short-group kernels (gen_variants.py: packed_short_menu; afhip_planner.cpp:
choose_packed_short_variant): every kernel of the menu against its float32 twin and the oracle, the A/B knob, unpack rules that change
wherever a row can stand in a block of rows, chunk and block geometry, uint16 storage, the public route, and the plans that stay on the
general packed kernel.

The yardstick of a packed short-group plan is the float32 plan of the same columns on `materialize()`'s values (tests/test_gpu_packed.py
holds those to numpy's float32 chain over all 65,536 stored values): past the unpack the packed kernel IS the float32 instantiation, so
the two must agree in every bit — NaN placement and the sign of zeros included (`_same_bits`) — under `exact_order`.

Against the oracle on the unpacked values: mean / sum / min / max columns and their integer powers bit for bit under
`exact_order` (the kernels' power chain and the oracle's `_powi` are the same double-double chain); sine_dd columns inside the §5 bound
`|got - exact| <= 1e-10 |exact| + 1e-12 max(window range, |exact|)` per window, carried through the column (`_sine_bound`): through an
integer power n as (|w| + t)^n - |w|^n, through the outer sum / mean as that reducer of the per-window bounds.  The oracle stands in
for `exact`; §5 puts its own error at 3e-14 of the window's scale, 3 % of the bound's second term, so the bound is taken x 1.05.

The float32 twin is the float32 kernel of the same form at the width float32 rows of that length take (`_twin`): two cells per lane
where the packed kernel reads four or two, one cell per lane on odd rows and for light plans (afhip_planner.cpp: load_path).  The
float32 production menu has no short-group kernel at all for the stat-1 two-column shapes on two-row, three-row and mixed groups (a
light float32 plan takes the LDS-DMA ring there, or the general direct-load kernel where the rows are no multiple of four:
short_group_form, `min_k`); for those the float32 plan is asserted to be on such a general kernel, and the bit compare is the same (mean
and sum columns are bit-exact on every route under `exact_order`).
"""
import functools
import json
import os
import re
import zlib

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import synth
from oracle import cport

import packed_recipes as pr
import packed_short_recipes as ps
import variant_recipes as vr
import test_gpu_packed_rules as rules_mod
import test_gpu_unsigned as uns
from test_gpu_variant_menu import _oracle_two_level

pytestmark = pytest.mark.gpu

KIND = vr.loaded_menu_kind()
MENU = [vr.variant(t) for t in ps.menu_of(KIND)]
BY_NAME = {v.name: v for v in MENU}
FLOAT_NAMES = {vr.variant(t).name for t in vr.production_menu(KIND)}
KNOB = "AFHIP_NO_PACKED_SHORT"


def _same_bits(got, want, msg=""):
    """float64 arrays equal bit for bit: NaN exactly where `want` has it, every other value with its sign bit (zeros included)."""
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, msg
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), msg
    assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan]), msg


def _twin(name):
    """The float32 kernel of the same form the float32 plan must land on — at the width float32 rows of that length take: two cells per
    lane on even rows, one on odd rows and for light plans — or None where the float32 production menu has none (module docstring)."""
    v = BY_NAME[name]
    tail = name[len("i16_p0_v2"):]
    for vec in ((2, 1) if v.vec >= 2 else (1,)):
        if f"f32_p0_v{vec}{tail}" in FLOAT_NAMES:
            return f"f32_p0_v{vec}{tail}"
    return None


def _assert_float_route(f32, name):
    got = vr.plan_name(f32)
    twin = _twin(name)
    if twin:
        assert got == twin, f32.describe()
    else:
        v = BY_NAME[name]
        assert v.stat == 1 and v.kmax == 2 and v.form in ("pair", "tri", "rag"), name
        assert "_pair" not in got and re.match(r"f32_p[01]_v\d_s1_t0_k2_", got), f32.describe()


def _is_general(name):
    return name.startswith("i16_p0_v") and name.endswith("_nt") and "_pair" not in name


def _sine_bound(values64, ib, ob, col):
    """The §5 bound of a sine_dd column, per output cell [P, cells] (module docstring)."""
    cube = values64
    w = np.abs(cport.resample(cube, ib, "sine_dd", col["inner_args"], False))
    with np.errstate(invalid="ignore"):
        rng = cport.resample(cube, ib, "max", None, False) - cport.resample(cube, ib, "min", None, False)
        t = 1e-10 * w + 1e-12 * np.maximum(rng, w)
        n = int(col["transform_arg"]) if col.get("transform") == "pow" else 1
        if n > 1:
            t = (w + t) ** n - w ** n
        out = cport.resample(np.ascontiguousarray(t), ob, col["outer"], None, False)
    return 1.05 * out.reshape(out.shape[0], -1)


def _assert_oracle(name, cols, got, want, values64, ib, ob):
    assert got.shape == want.shape
    for k, col in enumerate(cols):
        msg = f"{name} column {k}: {col}"
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), msg
        if col["inner"] == "sine_dd":
            tol = _sine_bound(values64, ib, ob, col)
            ok = ~np.isnan(want[k])
            err = np.abs(got[k] - want[k])[ok]
            worst = float(np.max(err / np.maximum(tol[ok], 1e-300))) if err.size else 0.0
            print(f"{msg}: worst |got - oracle| / bound = {worst:.3g}")
            assert (err <= tol[ok]).all(), f"{msg}: {worst:.3g} x the bound"
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=msg)


def _i16_cube(torch, q, pairs=pr.PAIRS, fill=pr.FILL):
    T, C = q.shape
    cube = af.PackedCube(torch.from_numpy(q.reshape(T, 1, C)).cuda(), scale_factor=pairs[0][0], add_offset=pairs[0][1], fill_value=fill)
    for m, a in pairs[1:]:
        cube = cube * m if m is not None else cube
        cube = cube + a if a is not None else cube
    assert isinstance(cube, af.PackedCube) and cube.n_pairs == len(pairs)
    return cube


def _packed_plan(r, cube, ob=None):
    from aggfly_amd import hip
    plan = hip.FusedPlan(r.T, r.n_cells, hip._dtype_code(cube), r.inner_bounds, r.outer_bounds if ob is None else ob, r.columns, exact_order=True)
    plan.bind_packing(cube)
    return plan


def _float_plan(r, ob=None):
    from aggfly_amd import hip
    return hip.FusedPlan(r.T, r.n_cells, hip.F32, r.inner_bounds, r.outer_bounds if ob is None else ob, r.columns, exact_order=True)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The recipe of kernel `name`, its stored cube in HBM, the float32 values, the new route's result and the oracle's — computed once
    and shared by the tests below (none of them writes to any of it)."""
    import torch
    r = ps.recipe(BY_NAME[name])
    q = ps.stored_cube(r, seed=zlib.crc32(name.encode()))
    cube = _i16_cube(torch, q)
    values = cube.materialize()
    plan = _packed_plan(r, cube)
    got = plan.run_temporal(cube).cpu().numpy()
    values64 = pr.np_unpack(q).astype(np.float64).reshape(r.T, 1, r.n_cells)
    want = _oracle_two_level(values64, r.inner_bounds, r.outer_bounds, r.columns)
    return dict(r=r, q=q, cube=cube, values=values, plan=plan, got=got, values64=values64, want=want)


# ---- 1. every kernel of the menu ----
@pytest.mark.parametrize("name", [v.name for v in MENU])
def test_kernel_against_its_float32_twin_and_the_oracle(torch_cuda, name):
    c = _case(name)
    r, q, plan = c["r"], c["q"], c["plan"]
    assert vr.plan_name(plan) == name and "storage=int16" in plan.describe(), plan.describe()
    np.testing.assert_array_equal(c["values"].cpu().numpy().reshape(r.T, r.n_cells), pr.np_unpack(q))
    f32 = _float_plan(r)
    _assert_float_route(f32, name)
    _same_bits(c["got"], f32.run_temporal(c["values"]).cpu().numpy(), name)
    # whole buffers: the empty second period is NaN in every column and cell
    assert r.outer_bounds[1] == r.outer_bounds[2] and np.isnan(c["got"][:, 1]).all()
    first, last, whole, ocean = ps.fill_census(r, q)
    assert first and last and whole and ocean == 3 and {32767, -32768} <= set(np.unique(q).tolist())
    _assert_oracle(name, r.columns, c["got"], c["want"], c["values64"], r.inner_bounds, r.outer_bounds)


def test_the_cases_cover_the_loaded_builds_menu(torch_cuda):
    from aggfly_amd import hip
    assert hip.menu_size(ps.KEY) == len(MENU) == len(BY_NAME)
    if KIND != "dev":
        assert {v.form for v in MENU} == {"pair", "quad", "tri", "rag"} and {v.vec for v in MENU} == {1, 2, 4}


# ---- 2. the knob ----
@pytest.mark.parametrize("name", [v.name for v in MENU])
def test_knob_sends_the_plan_to_the_general_packed_kernel(torch_cuda, monkeypatch, name):
    c = _case(name)
    r = c["r"]
    monkeypatch.setenv(KNOB, "1")
    general = _packed_plan(r, c["cube"])
    monkeypatch.delenv(KNOB)
    assert _is_general(vr.plan_name(general)), general.describe()
    assert vr.plan_name(_packed_plan(r, c["cube"])) == name                       # ... and back, once the knob is gone
    got_g = general.run_temporal(c["cube"]).cpu().numpy()
    for k, col in enumerate(r.columns):
        if col["inner"] != "sine_dd":
            _same_bits(c["got"][k], got_g[k], f"{name} column {k}: {col}")
    # the sine columns of both routes (the pair forms' table of cubics, the general kernel's table acos) are inside the §5 bound
    for got in (c["got"], got_g):
        _assert_oracle(name, r.columns, got, c["want"], c["values64"], r.inner_bounds, r.outer_bounds)


# ---- 3. rules along time ----
RULE_FORMS = {"pair": "i16_p0_v2_s2_t0_k6_d8_nt_pair_lean", "tri": "i16_p0_v2_s2_t0_k6_d6_nt_pair_lean_tri", "rag": "i16_p0_v2_s2_t0_k6_d8_nt_pair_lean_rag",
              "quad4": "i16_p0_v4_s1_t0_k6_d8_nt_pair_lean_quad", "rag4": "i16_p0_v4_s2_t0_k2_d8_nt_pair_lean_rag"}      # ... and two forms at four cells per lane


def _period_bounds(r, min_rows=33):
    """Periods of as few whole groups as hold `min_rows` rows: more than half the 64 rows a chunk packs, so every period is a chunk."""
    ib, G1 = r.inner_bounds, len(r.inner_bounds) - 1
    ob = [0]
    while ob[-1] < G1:
        g = ob[-1] + 1
        while g < G1 and ib[g] - ib[ob[-1]] < min_rows:
            g += 1
        ob.append(g)
    if ib[ob[-1]] - ib[ob[-2]] < min_rows:                   # a short rest would share the chunk of the period before it: one period
        del ob[-2]
    return np.array(ob, dtype=np.int64)


def _rule_layouts(form, r):
    """name -> (rule bounds, outer bounds or None for the recipe's)."""
    T = r.T
    out = {f"change_at_{c}": ([0, c, T], None) for c in (1, 2, 7, 8, 9)}
    out["change_at_last_row"] = ([0, T - 1, T], None)
    out["one_row_rule"] = ([0, 9, 10, T], None)
    ob = _period_bounds(r)
    ib = r.inner_bounds
    out["change_at_chunk_starts"] = ([0, int(ib[ob[2]]), int(ib[ob[4]]), T], ob)
    if form.startswith("rag"):                              # _RAG = [4, 1, 3, ...]: rows 0-3, row 4 alone, rows 5-7
        assert list(np.diff(ib[:4])) == [4, 1, 3]
        out["inside_a_three_row_group"] = ([0, 6, T], None)
        out["a_rule_for_the_one_row_group"] = ([0, 4, 5, T], None)
    return out


RULE_CASES = [(form, lay) for form in RULE_FORMS for lay in
              (["change_at_1", "change_at_2", "change_at_7", "change_at_8", "change_at_9", "change_at_last_row", "one_row_rule", "change_at_chunk_starts"]
               + (["inside_a_three_row_group", "a_rule_for_the_one_row_group"] if form.startswith("rag") else []))]


@pytest.mark.parametrize("form,layout", RULE_CASES)
def test_rule_changes_wherever_they_can_fall(torch_cuda, form, layout):
    name = RULE_FORMS[form]
    if name not in BY_NAME:
        pytest.fail(f"the loaded build has no {name}")
    r = ps.recipe(BY_NAME[name])
    bounds, ob = _rule_layouts(form, r)[layout]
    shapes = rules_mod._rule_shapes(False)                 # different scale, offset and fill from one rule to the next
    rules = [shapes[i % len(shapes)] for i in range(len(bounds) - 1)]
    assert all(a != b for a, b in zip(rules[:-1], rules[1:]))
    bits = rules_mod._stored(r.T, r.n_cells, bounds, rules, seed=zlib.crc32(f"{form}{layout}".encode()) & 0xffff)
    cube = rules_mod._cube(torch_cuda, bits.reshape(r.T, 1, r.n_cells), rules, bounds, False)
    assert cube.n_rules == len(bounds) - 1 and cube.rule_bounds == bounds
    values = cube.materialize()
    plan = _packed_plan(r, cube, ob)
    assert vr.plan_name(plan) == name, plan.describe()
    if ob is not None:
        n_chunks = int(re.search(r"chunks=(\d+)", plan.describe()).group(1))
        assert n_chunks == len(ob) - 1 >= 3, plan.describe()
    f32 = _float_plan(r, ob)
    _assert_float_route(f32, name)
    got, want = plan.run_temporal(cube).cpu().numpy(), f32.run_temporal(values).cpu().numpy()
    assert np.isfinite(want).mean() > 0.5
    _same_bits(got, want, f"{name} {layout}")


# ---- 4. geometry ----
GEOMETRY = [n for n in ("i16_p0_v2_s2_t0_k6_d8_nt_pair_lean", "i16_p0_v1_s2_t0_k6_d8_nt_pair_lean", "i16_p0_v2_s2_t0_k6_d8_nt_pair_lean_quad",
                        "i16_p0_v1_s2_t0_k6_d8_nt_pair_lean_quad", "i16_p0_v2_s2_t0_k6_d6_nt_pair_lean_tri", "i16_p0_v1_s2_t0_k6_d6_nt_pair_lean_tri",
                        "i16_p0_v2_s2_t0_k6_d8_nt_pair_lean_rag", "i16_p0_v1_s2_t0_k6_d8_nt_pair_lean_rag",
                        "i16_p0_v4_s2_t0_k2_d8_nt_pair_ss", "i16_p0_v4_s1_t0_k6_d8_nt_pair_lean_quad", "i16_p0_v4_s1_t0_k6_d6_nt_pair_lean_tri",
                        "i16_p0_v4_s2_t0_k2_d8_nt_pair_lean_rag")]


@pytest.mark.parametrize("name", GEOMETRY)
def test_short_chunks_partial_blocks_and_tail_lanes(torch_cuda, name):
    """Periods of 1, 0, 41, 1 groups and the rest: the first chunk is one group — shorter than a block of rows —, the second holds 41
    groups, which no block size divides (a last block with fewer groups than a block holds), and the rows are no multiple of a
    wave's cells (odd at one cell per lane)."""
    v = BY_NAME[name]
    r = ps.recipe(v)
    G1 = len(r.inner_bounds) - 1
    ob = np.array([0, 1, 1, 42, 43, G1], dtype=np.int64)
    gb = v.depth // {"pair": 2, "quad": 4, "tri": 3, "rag": 4}[v.form]
    assert 41 % gb != 0 and r.n_cells % (64 * v.vec) != 0 and (v.vec >= 2 or r.n_cells % 2 == 1)
    q = ps.stored_cube(r, seed=zlib.crc32(name.encode()) + 7)
    cube = _i16_cube(torch_cuda, q)
    plan = _packed_plan(r, cube, ob)
    assert vr.plan_name(plan) == name, plan.describe()
    n_chunks, lo, hi = (int(x) for x in re.search(r"chunks=(\d+) \(steps (\d+)\.\.(\d+)\)", plan.describe()).groups())
    assert n_chunks == 4 and lo == r.inner_bounds[1] < v.depth, plan.describe()
    f32 = _float_plan(r, ob)
    _assert_float_route(f32, name)
    got, want = plan.run_temporal(cube).cpu().numpy(), f32.run_temporal(cube.materialize()).cpu().numpy()
    assert np.isnan(want[:, 1]).all() and np.isfinite(want[:, [0, 2, 3, 4]]).mean() > 0.5
    _same_bits(got, want, name)


# ---- 5. uint16 storage ----
U16_NAMES = ["i16_p0_v2_s2_t0_k2_d8_nt_pair_ss", "i16_p0_v1_s2_t0_k6_d8_nt_pair_lean", "i16_p0_v2_s1_t0_k6_d8_nt_pair_lean_quad",
             "i16_p0_v2_s2_t0_k6_d6_nt_pair_lean_tri", "i16_p0_v1_s2_t0_k6_d8_nt_pair_lean_rag", "i16_p0_v4_s2_t0_k2_d8_nt_pair_lean",
             "i16_p0_v4_s1_t0_k6_d8_nt_pair_lean_rag"]


@pytest.mark.parametrize("name", U16_NAMES)
def test_uint16_storage_takes_the_same_kernels(torch_cuda, name):
    from aggfly_amd import hip
    r = ps.recipe(BY_NAME[name])
    fill = 65535
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    q = rng.integers(0, 65536, (r.T, r.n_cells)).astype(np.uint16)
    q.reshape(-1)[rng.choice(q.size, 120, replace=False)] = np.array([0, 65535, 1, 32767, 32768, 65534] * 20, dtype=np.uint16)
    ib = r.inner_bounds
    ne = np.flatnonzero(np.diff(ib) > 0)
    for g in ne[::5]:
        q[ib[g], rng.choice(r.n_cells, 25, replace=False)] = fill          # first rows of groups
    for g in ne[1::5]:
        q[ib[g + 1] - 1, rng.choice(r.n_cells, 25, replace=False)] = fill  # last rows
    q[:, [3, r.n_cells // 2, r.n_cells - 1]] = fill                        # whole cells, the last one included
    cube = uns._cuda_cube(torch_cuda, q.reshape(r.T, 1, r.n_cells), scale_factor=uns.PAIRS[0][0], add_offset=uns.PAIRS[0][1], fill_value=fill) - 273.15
    signed = af.PackedCube(cube.q, fill_value=-1, unsigned=False, _pairs=cube.pairs)
    assert hip._dtype_code(cube) == hip.U16 and hip._dtype_code(signed) == hip.I16
    pu, pi = _packed_plan(r, cube), _packed_plan(r, signed)
    assert vr.plan_name(pu) == vr.plan_name(pi) == name and "storage=uint16" in pu.describe() and "storage=int16" in pi.describe(), pu.describe()
    values = cube.materialize()
    want_values = uns.np_unpack(q, uns.PAIRS, fill)
    np.testing.assert_array_equal(values.cpu().numpy().reshape(r.T, r.n_cells), want_values)
    assert (q > 32767).mean() > 0.4 and np.isnan(want_values).sum() == (q == fill).sum() > 3 * r.T and (q == 0).any()
    f32 = _float_plan(r)
    _assert_float_route(f32, name)
    _same_bits(pu.run_temporal(cube).cpu().numpy(), f32.run_temporal(values).cpu().numpy(), name)


# ---- 6. the public interface ----
def _write_store(tmp_path, name, stored, time, ny, nx):
    from aggfly_amd import io as afio
    attrs = {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}
    tv, tattrs = afio._encode_time(time)
    store = str(tmp_path / name)
    os.makedirs(store)
    json.dump({"zarr_format": 2}, open(os.path.join(store, ".zgroup"), "w"))
    afio._write_array(store, "t2m", stored, ("time", "latitude", "longitude"), (48, ny, nx), attrs, None)
    afio._write_array(store, "time", np.asarray(tv, dtype=np.float64), ("time",), (len(time),), tattrs, None)
    afio._write_array(store, "latitude", 35 + 0.25 * np.arange(ny), ("latitude",), (ny,), {}, None)
    afio._write_array(store, "longitude", 250 + 0.25 * np.arange(nx), ("longitude",), (nx,), {}, None)
    return store


def _celsius(x):
    return x - 273.15


PUBLIC = {
    "six_hourly": ("6h", 4, "_quad", dict(tavg=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 4)}),
                                                ("aggregate", {"calc": "sum", "groupby": "month"})])),
    "tmin_tmax_pairs": ("12h", 2, "_pair", dict(sdd=[("aggregate", {"calc": "sine_dd", "groupby": "date", "ddargs": [10, 30, 0]}),
                                                     ("aggregate", {"calc": "sum", "groupby": "month"})])),
}


@pytest.mark.parametrize("case", list(PUBLIC))
def test_keep_packed_short_group_spec_through_the_public_api(torch_cuda, tmp_path, case):
    from aggfly_amd import engine as eng
    freq, per_day, suffix, spec = PUBLIC[case]
    days, ny, nx = 75, 25, 44                                           # 1,100 cells, 75 days from mid-January: four months, the last of one day
    T = days * per_day
    rng = np.random.default_rng(len(case))
    stored = np.clip(np.rint(pr.stored_near(12.0) + rng.normal(0.0, 9.0, (T, ny, nx)) / 0.0017), -32766, 32766).astype(np.int16)
    if per_day == 2:                                                    # (tmin, tmax): the second row of a day is the larger
        stored = np.sort(stored.reshape(days, 2, ny, nx), axis=1).reshape(T, ny, nx)
    stored[rng.random((T, ny, nx)) < 0.01] = -32767
    stored[:, 2, 3] = -32767                                            # an ocean cell
    time = pd.date_range("2005-01-17", periods=T, freq=freq)
    store = _write_store(tmp_path, f"{case}.zarr", stored, time, ny, nx)
    packed = af.dataset_from_path(store, "t2m", device="cuda", keep_packed=True, preprocess=_celsius)
    plain = af.dataset_from_path(store, "t2m", device="cuda", preprocess=_celsius)
    assert packed.is_packed and not plain.is_packed
    tab = synth.weights_table(ny, nx, 20, seed=3, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}), regionid="geoid")
    old = eng.config.exact_order
    try:
        for exact in (True, False):
            eng.config.exact_order = exact
            frames, descs = {}, {}
            for key, ds in (("packed", packed), ("plain", plain)):
                eng._PLAN_CACHE.clear()
                frames[key] = af.aggregate_dataset(dataset=ds, weights=af.weights_from_objects(ds, gr, table=tab), **spec)
                plans = list(eng._PLAN_CACHE.values())
                assert len(plans) == 1
                descs[key] = plans[0].describe()
            dp, df = descs["packed"], descs["plain"]
            assert dp.split()[0].startswith("variant=i16_p0_v4_") and suffix in dp.split()[0] and "storage=int16" in dp, dp      # 1,100 cells: four per lane
            assert dp.split()[0].endswith({"_quad": "_pair_lean_quad", "_pair": "_pair_ss"}[suffix]), dp
            assert df.split()[0].startswith("variant=f32_"), df
            cols = [c for c in frames["packed"].columns if c not in ("geoid", "time")]
            assert len(cols) == (3 if case == "six_hourly" else 1) and frames["packed"]["time"].nunique() == 4
            if exact:
                pd.testing.assert_frame_equal(frames["packed"], frames["plain"], check_exact=True)
            else:                                                       # the fast routes: the project's figure for them (1e-12)
                pd.testing.assert_frame_equal(frames["packed"], frames["plain"], check_exact=False, rtol=1e-12, atol=0)
            assert np.isfinite(frames["packed"][cols].values).any()
    finally:
        eng.config.exact_order = old
        eng._PLAN_CACHE.clear()


# ---- 7. what stays on the general packed kernel ----
def _staying_cases():
    e = float(pr.np_unpack([pr.stored_near(12.0)], pr.PAIRS, None)[0])
    return {
        "threshold_slot": [dict(inner="mean", outer="sum"), dict(inner="dd", inner_args=(e, e + 20.0, 0.0), outer="sum")],
        "outer_max": [dict(inner="max", outer="sum"), dict(inner="min", outer="max")],
        "non_integer_power": [dict(inner="mean", outer="sum"), dict(inner="mean", transform="pow", transform_arg=1.5, outer="sum")],
    }


@pytest.mark.parametrize("form", ["pair", "quad", "rag"])
@pytest.mark.parametrize("case", list(_staying_cases()))
def test_other_short_group_plans_stay_on_the_general_kernel(torch_cuda, monkeypatch, case, form):
    cols = _staying_cases()[case]
    lens = vr._inner_lengths(form, 0)
    ib = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    edges = sorted({float(x) for c in cols if c["inner"] == "dd" for x in c["inner_args"][:2]})
    r = vr.Recipe("", pr.I16, int(ib[-1]), 1102, ib, vr._outer_bounds(len(lens), ps.PERIOD), cols, True, 0, edges=edges)
    q = ps.stored_cube(r, seed=zlib.crc32(f"{case}{form}".encode()))
    cube = _i16_cube(torch_cuda, q)
    plan = _packed_plan(r, cube)
    monkeypatch.setenv(KNOB, "1")
    knob = _packed_plan(r, cube)
    monkeypatch.delenv(KNOB)
    assert _is_general(vr.plan_name(plan)) and plan.describe().split()[0] == knob.describe().split()[0], plan.describe()
    got = plan.run_temporal(cube).cpu().numpy()
    _same_bits(got, knob.run_temporal(cube).cpu().numpy(), f"{case} {form}")
    want = _oracle_two_level(pr.np_unpack(q).astype(np.float64).reshape(r.T, 1, r.n_cells), ib, r.outer_bounds, cols)
    for k, col in enumerate(cols):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k]))
        if col.get("transform") == "pow":                   # the device pow(): tests/test_gpu_variant_menu.py
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True)
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{case} {form} column {k}")
