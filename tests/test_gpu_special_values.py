"""Every production kernel on degenerate windows and special values.

tests/test_gpu_variant_menu.py and its packed / histogram siblings run one plan per kernel on ordinary temperatures.  Here the same
plans — `variant_recipes.recipe`, `packed_recipes`, `packed_hist_recipes`, `end_bins_recipes`: the plan must name the kernel — read
cubes whose cells hold one class of window each (tests/special_values.py: flat windows, ties, zeros of both signs, values on every
edge, infinities, subnormals, sums that overflow, NaN in the last / a middle / all rows but one), and the per-cell values go against
the oracle under `assert_same_kind`: NaN and +-inf in the same places with the same sign, zeros with their sign where the bar is
bit-exact, and the finite values at test_gpu_variant_menu._assert_cells' bars, unchanged.

Two rules are pinned with expected values of their own:
  * inner min / max of zeros of both signs: the kernels order -0 < +0, the reference keeps the first seen
    (`special_values.hardware_zero_rule`; DESIGN.md §5, include/aggfly_hip.h);
  * sine_dd on windows that hold an infinity or whose range overflows (classes pinf, ninf, both_inf, overflow): the closed forms
    subtract infinities, the reference's value is NaN or an accident of inf arithmetic, the lean forms return the mathematical
    value — outside sine_dd's contract.  Those (cell, column) pairs are left out and counted; every other class is
    held to 1e-10 on sine columns.
"""
import zlib

import numpy as np
import pytest

import end_bins_recipes as eb
import packed_hist_recipes as ph
import packed_recipes as pr
import special_values as sv
import variant_recipes as vr
from oracle import cport
from oracle.ref_spatial import spatial_num_den, scatter_block, weight_triplets
from test_gpu_packed import _run_recipe
from test_gpu_variant_menu import _csr_table, _powi

pytestmark = pytest.mark.gpu
INF = float("inf")

KIND = vr.loaded_menu_kind()
MENUS = {
    "float": ([vr.variant(v) for v in vr.production_menu(KIND)], vr.recipe),
    "packed": ([vr.variant(v) for v in vr.menu_of("packed", KIND)], pr.recipe),
    "packed_hist": ([vr.variant(t) for t in vr.menu_of("packed_hist", KIND) if t[8]], ph.recipe),
    "end_bins": ([vr.variant(t) for t in vr.menu_of("end_bins", KIND)], eb.recipe),
}
CASES = [(v.name, menu) for menu, (variants, _) in MENUS.items() for v in variants]
BY_NAME = {v.name: (v, make) for variants, make in MENUS.values() for v in variants}


def _oracle(cube, ib, ob, cols):
    """test_gpu_variant_menu._oracle_two_level with the kernels' rule for an inner min / max of zeros of both signs."""
    out = []
    for c in cols:
        a = cport.resample(cube, ib, c["inner"], c.get("inner_args"), False)
        a = sv.hardware_zero_rule(a, cube, ib, c["inner"])
        tf = c.get("transform")
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if tf == "pow":
                e = c["transform_arg"]
                a = _powi(a, e) if float(e).is_integer() and e >= 1 else np.power(a, e)
            elif tf == "hinge":
                a = (a > c["transform_arg"]) * (a - c["transform_arg"])
        outer = c.get("outer", "identity")
        if outer != "identity":
            a = cport.resample(np.ascontiguousarray(a), ob, outer, c.get("outer_args"), False)
        out.append(a.reshape(a.shape[0], -1))
    return np.stack(out)


def _class_count(n_cells, classes, names):
    """Cells of a class cube that hold one of `names` (cell c holds class c % n)."""
    n = len(classes)
    return sum((n_cells - classes.index(x) + n - 1) // n for x in names)


def _assert_cells(v, cols, got, want, cls, classes):
    """The bars of test_gpu_variant_menu._assert_cells under assert_same_kind; -> the (cell, column) pairs left out."""
    assert got.shape == want.shape, (got.shape, want.shape)
    undefined = np.isin(cls, sv.SINE_UNDEFINED) if classes is sv.CLASSES else np.zeros(len(cls), dtype=bool)
    left_out = 0
    for k, col in enumerate(cols):
        msg = f"{v.name} column {k}: {col}"
        if col["inner"] == "sine_dd":
            keep = ~undefined
            left_out += int(undefined.sum())
            sv.assert_same_kind(got[k][:, keep], want[k][:, keep], bit_exact=False, rtol=1e-10, atol=1e-10, msg=msg, cell_class=cls[keep])
        elif col.get("transform") == "pow" and not float(col["transform_arg"]).is_integer():
            sv.assert_same_kind(got[k], want[k], bit_exact=False, rtol=1e-12, msg=msg, cell_class=cls)
        elif col.get("transform") == "pow":
            sv.assert_same_kind(got[k], want[k], bit_exact=False, rtol=4e-15 if v.lean else 4e-16, msg=msg, cell_class=cls)
        else:
            sv.assert_same_kind(got[k], want[k], bit_exact=True, msg=msg, cell_class=cls)
    n_sine = sum(c["inner"] == "sine_dd" for c in cols)
    # sine columns are left out on the four classes of non-finite windows, and only those: 4 / n_classes of their cells
    expect = n_sine * _class_count(len(cls), list(classes), sv.SINE_UNDEFINED) if classes is sv.CLASSES else 0
    assert left_out == expect and abs(left_out - n_sine * len(cls) * (4 / len(sv.CLASSES) if classes is sv.CLASSES else 0)) <= 4 * n_sine
    return left_out


def _assert_region_sums(name, fused, cells, tab, n_cells):
    """A region-fused run against the oracle's spatial stage on the plan's own per-cell values: sums that are not finite agree in
    kind exactly, finite ones at the bars of test_variant_against_the_oracle; shared validity — a cell with a NaN in any column
    drops out of every sum and of the weight, a cell with an infinity does not."""
    K = cells.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        nums, den, _ = spatial_num_den({f"k{k}": cells[k].T for k in range(K)}, tab, np.arange(n_cells))
    got_den = fused["den"].cpu().numpy()
    sv.assert_same_kind(got_den, den, bit_exact=False, rtol=1e-12, msg=f"{name} den")
    got_res = fused["res"].cpu().numpy()
    for k in range(K):
        want = nums[f"k{k}"]
        sv.assert_same_kind(fused["num"][k].cpu().numpy(), want, bit_exact=False, rtol=1e-12, atol=1e-9, msg=f"{name} num {k}")
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            res = np.divide(want, den, out=np.full_like(den, np.nan), where=den != 0)
        sv.assert_same_kind(got_res[k], res, bit_exact=False, rtol=1e-12, atol=1e-9, msg=f"{name} res {k}")
    assert (got_den[:, 1] == 0).all() and np.isnan(got_res[:, :, 1]).all()          # the empty second period
    # the rule, visible: had an infinity made its cell invalid, or a NaN in one column left the cell's other columns in, den would differ
    nan_any, nan_all, inf_any = np.isnan(cells).any(axis=0), np.isnan(cells).all(axis=0), np.isinf(cells).any(axis=0)      # [P, cells]
    region_idx, cell_idx, w_vals, region_ids = weight_triplets(tab, np.arange(n_cells))
    kw = dict(region_idx=region_idx, cell_idx=cell_idx, w_vals=w_vals, n_regions=len(region_ids))
    seen = {"inf stays": False, "one NaN column drops the cell": False}
    if (inf_any & ~nan_any).any():
        other = scatter_block((~nan_any & ~inf_any).T.astype(float), **kw)
        assert not np.allclose(other, den, rtol=1e-9, atol=0) and np.allclose(got_den, den, rtol=1e-12, atol=0)
        seen["inf stays"] = True
    if (nan_any & ~nan_all).any():
        other = scatter_block((~nan_all).T.astype(float), **kw)
        assert not np.allclose(other, den, rtol=1e-9, atol=0) and np.allclose(got_den, den, rtol=1e-12, atol=0)
        seen["one NaN column drops the cell"] = True
    return seen


SEEN = {"inf stays": 0, "one NaN column drops the cell": 0, "twins": 0, "left out": 0, "sine cells": 0}


# ---- 1. one case per production kernel of all four menus ----
@pytest.mark.parametrize("name,menu", CASES, ids=[c[0] for c in CASES])
def test_kernel_on_special_values(torch_cuda, name, menu):
    from aggfly_amd import hip
    v, make = BY_NAME[name]
    r = make(v)
    if eb.is_packed(r.dtype):
        q, cls = sv.packed_class_cube(r, pr.stored_near, pr.FILL)
        plan, got, want, values = _run_recipe(torch_cuda, r, q)
        assert vr.plan_name(plan) == name, plan.describe()
        assert not ((values == 0) & np.signbit(values)).any()            # no -0.0 from the unpack rule: the oracle's min / max stand as they are
        _assert_cells(v, r.columns, got, want, cls, sv.PACKED_CLASSES)
        return
    cube, cls = sv.class_cube(r)
    plan = hip.FusedPlan(r.T, r.n_cells, r.dtype, r.inner_bounds, r.outer_bounds, r.columns, exact_order=r.exact_order, tuning=r.tuning)
    assert plan.describe().split()[0] == f"variant={r.name}", plan.describe()
    d = torch_cuda.from_numpy(cube).cuda()
    want = _oracle(cube.astype(np.float64).reshape(r.T, 1, r.n_cells), r.inner_bounds, r.outer_bounds, r.columns)
    n_sine = sum(c["inner"] == "sine_dd" for c in r.columns)
    if not r.region_fused:
        SEEN["left out"] += _assert_cells(v, r.columns, plan.run_temporal(d).cpu().numpy(), want, cls, sv.CLASSES)
        SEEN["sine cells"] += n_sine * r.n_cells
        return
    tab = _csr_table(r.n_cells, seed=zlib.crc32(name.encode()) & 0xFFFF)
    csr = hip.CSR(tab["index_right"].to_numpy(), tab["cell_id"].to_numpy(), tab["weight"].to_numpy(), int(tab["index_right"].max()) + 1, r.n_cells)
    fused = plan.run(d, csr)
    assert "last-run=region-fused" in plan.describe(), plan.describe()
    cells = plan.run(d, csr, want_cells=True)["cells"].cpu().numpy()          # the per-cell route of the same plan (the base variant)
    SEEN["left out"] += _assert_cells(v, r.columns, cells, want, cls, sv.CLASSES)
    SEEN["sine cells"] += n_sine * r.n_cells
    seen = _assert_region_sums(name, fused, cells, tab, r.n_cells)
    SEEN["twins"] += 1
    for key, hit in seen.items():
        SEEN[key] += int(hit)


def test_the_cases_cover_every_menu_of_the_loaded_build(torch_cuda):
    """One case per production kernel of the float, packed, packed-histogram and end-bin menus (each asserts that its plan selected
    that kernel), no name twice; and what the cases above saw when they ran before this one: the share of sine (cell, column) pairs
    left out is 4 / n_classes, and the twins showed both halves of the shared-validity rule."""
    from aggfly_amd import hip
    info = hip.build_info()
    assert len(MENUS["float"][0]) == info["variants"] - info["arms"]
    assert len(MENUS["packed"][0]) == info["packed_variants"]
    assert len(MENUS["packed_hist"][0]) == sum(t[8] for t in vr.menu_of("packed_hist", KIND)) and len(vr.menu_of("packed_hist", KIND)) == info["packed_hist_variants"]
    assert len(MENUS["end_bins"][0]) == info["end_bins_variants"]
    assert len(CASES) == len(BY_NAME) == sum(len(m[0]) for m in MENUS.values())
    if KIND == "full":
        assert [len(MENUS[k][0]) for k in ("float", "packed", "packed_hist", "end_bins")] == [367, 69, 10, 26]
    if SEEN["sine cells"]:
        print(f"sine_dd: {SEEN['left out']} of {SEEN['sine cells']} (cell, column) pairs left out (classes {', '.join(sv.SINE_UNDEFINED)})")
        assert abs(SEEN["left out"] / SEEN["sine cells"] - 4 / len(sv.CLASSES)) < 0.01
    if SEEN["twins"] >= 10:
        assert SEEN["inf stays"] > 0 and SEEN["one NaN column drops the cell"] > 0, SEEN


# ---- 2. the standalone entry points (k_slots_to_block's store in the cube's dtype) ----
DDA = [[10.0, 30.0, 0.0], [20.0, INF, 0.0], [-INF, 12.5, 1.0], [0.0, 5.0, 0.0]]
SINE = [[10.0, 30.0, 0.0], [5.0, 18.0, 1.0], [0.0, 5.0, 0.0]]


def _bounds(T):
    """Groups of 24 rows, one empty group, a tail of 7 rows (test_gpu_kernels._bounds_with_gaps)."""
    b = list(range(0, T, 24))
    b.insert(5, b[5])
    return np.array(sorted(b + [T]), dtype=np.int64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(24 * 9 + 7, 5, 7), (24 * 9 + 7, 6, 20)], ids=["5x7", "6x20"])
def test_group_entry_points_on_special_values(torch_cuda, shape, dtype):
    from aggfly_amd import hip
    T, ny, nx = shape
    ib = _bounds(T)
    edges = sorted({x for row in DDA + SINE for x in row[:2] if np.isfinite(x)})
    r = vr.Recipe("", vr.F64 if dtype is np.float64 else vr.F32, T, ny * nx, ib, np.array([0, len(ib) - 1]), [], True, 0, edges=edges)
    flat, cls = sv.class_cube(r)
    cube = flat.reshape(T, ny, nx)
    d = torch_cuda.from_numpy(cube).cuda()
    G = len(ib) - 1
    for calc in ("mean", "sum", "min", "max", "nanmean"):
        want = sv.hardware_zero_rule(cport.block_stat(cube, ib, calc), cube, ib, calc)
        got = hip.group_stat(d, ib, calc).cpu().numpy()
        assert got.dtype == dtype
        sv.assert_same_kind(got.reshape(G, -1), want.reshape(G, -1), bit_exact=True, msg=f"group_stat {calc}", cell_class=cls)
    for fn, ref, what in ((hip.group_dd, cport.block_dd, "group_dd"), (hip.group_bins, cport.block_bins, "group_bins")):
        got, want = fn(d, ib, DDA).cpu().numpy(), ref(cube, ib, DDA)
        assert got.dtype == dtype
        for j in range(len(DDA)):
            sv.assert_same_kind(got[..., j].reshape(G, -1), want[..., j].reshape(G, -1), bit_exact=True, msg=f"{what} {DDA[j]}", cell_class=cls)
    got, want = hip.group_sine_dd(d, ib, SINE).cpu().numpy(), cport.block_sine_dd(cube, ib, SINE)
    keep = ~np.isin(cls, sv.SINE_UNDEFINED)
    assert (~keep).sum() == _class_count(ny * nx, list(sv.CLASSES), sv.SINE_UNDEFINED)
    tol = 1e-10 if dtype is np.float64 else 2e-6          # float32: the store's rounding (test_group_sine_dd_1e10)
    for j in range(len(SINE)):
        sv.assert_same_kind(got[..., j].reshape(G, -1)[:, keep], want[..., j].reshape(G, -1)[:, keep], bit_exact=False, rtol=tol, atol=tol,
                            msg=f"group_sine_dd {SINE[j]}", cell_class=cls[keep])
    if dtype is np.float32:                                # the float32 store of a sum that float64 holds
        s = hip.group_stat(d, ib, "sum").cpu().numpy().reshape(G, -1)[:, cls == "overflow"]
        assert np.isinf(s).any() and (s == INF).any() and (s == -INF).any()


# ---- 3. k_transform ----
def _specials(dt):
    tiny, big = np.nextafter(dt(0), dt(1)), np.finfo(dt).max
    return np.array([0.0, -0.0, INF, -INF, np.nan, tiny, -tiny, big, -big, 1.0, -1.0, -2.5, -0.75, -1.5, 2.5, 0.75, 20.0, 12.25], dtype=dt)


def _kind_and_sign(got, want, *, rtol, msg):
    """assert_same_kind, and the zeros' signs whatever the bar (an exact zero is the same zero in both)."""
    sv.assert_same_kind(got, want, bit_exact=False, rtol=rtol, msg=msg)
    z = (want == 0) & (got == 0)
    assert np.array_equal(np.signbit(got[z]), np.signbit(want[z])), (msg, got[z], want[z])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_transform_on_special_values(torch_cuda, dtype):
    """`hip.transform` (k_transform) against numpy's own np.power, (x > k) * (x - k) and np.multiply, with the dtype rules of
    test_dataset_transforms_run_in_the_hip_library: float32 ** python number stays float32, ** np.int64 / np.float64 gives float64;
    float32 x float64 promotes.  Kind-strict, and sign-strict on zeros and infinities.  Integer powers: 4e-16 (the double-double
    chain is correctly rounded); the device pow(): 1e-12; a float32 result: one float32 ulp, 2^-23 — numpy's float32 pow is within an
    ulp of the rounded float64 value the kernel stores."""
    from aggfly_amd import hip
    x = _specials(dtype)
    x = np.concatenate([x, x[::-1], x[3:]])                 # 51 elements: more than one lane's four, a partly filled last thread
    d = torch_cuda.from_numpy(x).cuda()
    f32_ulp = 2.0 ** -23
    with np.errstate(all="ignore"):
        for e in (-2, -1, 0, 1, 2, 3, 0.5, -0.5, 1.5):
            exps = [e, np.int64(e)] if float(e).is_integer() else [e, np.float64(e)]
            for ev in exps:
                want = np.power(x, ev)
                out_dtype = torch_cuda.float64 if want.dtype == np.float64 else torch_cuda.float32
                got = hip.transform(d, "pow", float(e), out_dtype=out_dtype).cpu().numpy()
                assert got.dtype == want.dtype
                bar = 4e-16 if float(e).is_integer() else 1e-12
                _kind_and_sign(got, want, rtol=max(bar, f32_ulp) if want.dtype == np.float32 else bar, msg=f"{dtype.__name__} ** {ev!r}")
        for knot in (20.0, 0.0, -1.5):
            want = (x > knot) * (x - dtype(knot))
            got = hip.transform(d, "hinge", knot).cpu().numpy()
            assert got.dtype == want.dtype == dtype
            _kind_and_sign(got, want, rtol=0.0, msg=f"hinge at {knot}")
        y = np.roll(_specials(dtype), 5)
        for odt in (dtype, np.float64):
            other = np.concatenate([y, y, y[:len(x) - 2 * len(y)]]).astype(odt)
            want = np.multiply(x, other)
            out_dtype = torch_cuda.float64 if want.dtype == np.float64 else torch_cuda.float32
            got = hip.transform(d, "inter", other=torch_cuda.from_numpy(other).cuda(), out_dtype=out_dtype).cpu().numpy()
            assert got.dtype == want.dtype
            _kind_and_sign(got, want, rtol=0.0, msg=f"inter {dtype.__name__} x {np.dtype(odt).name}")
