"""Every production kernel variant against the oracle, at the edge of its template.

One case per variant of the loaded build's production menu (the test id is the variant name).  `variant_recipes.recipe` shapes a
plan that the planner answers with exactly that kernel at `tuning == 0` (the float32 depth-4 forms excepted, see there): as many
columns as the kernel holds and its threshold-slot tier filled, a cell count that leaves the last workgroup partly filled, group
lengths that are no multiple of the burst depth, empty groups and periods, NaN at group starts, whole NaN groups, ocean cells and
values on, next to, below and above every edge.  The per-cell values are held to the suite's bars: bit-exact for mean / sum /
min / max / nanmean / dd / bins (exact_order), 4e-16 relative for integer powers (4e-15 on the lean short-group forms, whose
written-out power chain is held to that in test_gpu_kernels.py), 1e-12 for non-integer powers (the device pow(), as in
test_gpu_api.py), 1e-10 for sine_dd.  A region-fused twin (`_rf`) runs its base variant's recipe with several periods and no
exact order against a CSR: the plan must take the region-fused route, and its weighted sums and their quotients must match the
oracle's spatial stage on the plan's own per-cell values (the bars of test_region_fused_period_ends_against_the_per_cell_routes),
with no weight and a NaN result in the empty period.
"""
import zlib

import numpy as np
import pandas as pd
import pytest

import variant_recipes as vr
from oracle.ref_spatial import spatial_num_den
from oracle import cport

pytestmark = pytest.mark.gpu


MENU = [vr.variant(v) for v in vr.production_menu(vr.loaded_menu_kind())]
BY_NAME = {v.name: v for v in MENU}


def _powi(x, n):
    """x ** n (integer n >= 1) correctly rounded: a double-double product chain with Dekker's exact products, no FMA needed.
    (np.power and libm's pow are not correctly rounded: np.power misses by an ulp on ~4 % of daily means.)"""
    x = np.asarray(x, dtype=np.float64)

    def split(a):
        c = 134217729.0 * a
        hi = c - (c - a)
        return hi, a - hi

    def two_prod(a, b):
        p = a * b
        ah, al = split(a)
        bh, bl = split(b)
        return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl

    with np.errstate(invalid="ignore", over="ignore"):
        hi, lo = x, np.zeros_like(x)
        for _ in range(int(n) - 1):
            p, err = two_prod(hi, x)
            hi, lo = p, lo * x + err
        out = hi + lo
    return np.where(np.isfinite(hi), out, hi)


def _oracle_two_level(cube, ib, ob, cols):
    """Per-cell oracle of a fused plan: numba_resample -> transform -> numba_resample (test_gpu_kernels.py's helper, with positive
    integer powers correctly rounded)."""
    out = []
    for c in cols:
        a = cport.resample(cube, ib, c["inner"], c.get("inner_args"), False)
        tf = c.get("transform")
        if tf == "pow":
            e = c["transform_arg"]
            a = _powi(a, e) if float(e).is_integer() and e >= 1 else np.power(a, e)      # non-integer: np.power (dataset.py:543)
        elif tf == "hinge":
            a = (a > c["transform_arg"]) * (a - c["transform_arg"])
        outer = c.get("outer", "identity")
        if outer != "identity":
            a = cport.resample(np.ascontiguousarray(a), ob, outer, c.get("outer_args"), False)
        out.append(a.reshape(a.shape[0], -1))
    return np.stack(out)      # [K, P, cells]


def _csr_table(C, R=29, seed=0):
    """Regions of contiguous cells, every seventh cell also in the next region (border cells), a few zero weights."""
    rng = np.random.default_rng(seed)
    cells = np.arange(C)
    reg = cells * R // C
    extra = cells[(cells % 7 == 0) & (reg < R - 1)]
    idx = np.concatenate([reg, reg[extra] + 1])
    cid = np.concatenate([cells, extra])
    w = rng.uniform(0.05, 1.0, len(cid))
    w[rng.choice(len(w), len(w) // 40, replace=False)] = 0.0
    order = np.argsort(idx, kind="stable")
    return pd.DataFrame({"index_right": idx[order], "cell_id": cid[order], "weight": w[order]})


def _assert_cells(v, cols, got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    for k, col in enumerate(cols):
        msg = f"{v.name} column {k}: {col}"
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), msg
        if col["inner"] == "sine_dd":
            np.testing.assert_allclose(got[k], want[k], rtol=1e-10, atol=1e-10, equal_nan=True, err_msg=msg)
        elif col.get("transform") == "pow" and not float(col["transform_arg"]).is_integer():      # the device pow(): test_non_integer_exponent_is_fused
            np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=msg)
        elif col.get("transform") == "pow":
            np.testing.assert_allclose(got[k], want[k], rtol=4e-15 if v.lean else 4e-16, atol=0, equal_nan=True, err_msg=msg)
        else:
            np.testing.assert_array_equal(got[k], want[k], err_msg=msg)


@pytest.mark.parametrize("name", [v.name for v in MENU])
def test_variant_against_the_oracle(torch_cuda, name):
    from aggfly_amd import hip
    v = BY_NAME[name]
    r = vr.recipe(v)
    cube = vr.cube_for(r, seed=zlib.crc32(name.encode()))
    plan = hip.FusedPlan(r.T, r.n_cells, r.dtype, r.inner_bounds, r.outer_bounds, r.columns, exact_order=r.exact_order, tuning=r.tuning)
    assert plan.describe().split()[0] == f"variant={r.name}", plan.describe()
    d = torch_cuda.from_numpy(cube).cuda()
    want = _oracle_two_level(cube.astype(np.float64).reshape(r.T, 1, r.n_cells), r.inner_bounds, r.outer_bounds, r.columns)
    if not r.region_fused:
        _assert_cells(v, r.columns, plan.run_temporal(d).cpu().numpy(), want)
        return
    tab = _csr_table(r.n_cells, seed=zlib.crc32(name.encode()) & 0xFFFF)
    csr = hip.CSR(tab["index_right"].to_numpy(), tab["cell_id"].to_numpy(), tab["weight"].to_numpy(), int(tab["index_right"].max()) + 1, r.n_cells)
    fused = plan.run(d, csr)
    assert "last-run=region-fused" in plan.describe(), plan.describe()
    cells = plan.run(d, csr, want_cells=True)["cells"].cpu().numpy()          # the per-cell route of the same plan (the base variant)
    _assert_cells(v, r.columns, cells, want)
    nums, den, _ = spatial_num_den({f"k{k}": cells[k].T for k in range(len(r.columns))}, tab, np.arange(r.n_cells))
    got_den = fused["den"].cpu().numpy()
    np.testing.assert_allclose(got_den, den, rtol=1e-12)
    for k in range(len(r.columns)):
        np.testing.assert_allclose(fused["num"][k].cpu().numpy(), nums[f"k{k}"], rtol=1e-12, atol=1e-9, err_msg=f"{name} column {k}")
        with np.errstate(invalid="ignore", divide="ignore"):
            res = np.divide(nums[f"k{k}"], den, out=np.full_like(den, np.nan), where=den != 0)
        np.testing.assert_allclose(fused["res"][k].cpu().numpy(), res, rtol=1e-12, atol=1e-9, equal_nan=True, err_msg=f"{name} res {k}")
    assert (got_den[:, 1] == 0).all() and np.isnan(fused["res"].cpu().numpy()[:, :, 1]).all()          # the empty second period


def test_the_cases_cover_the_loaded_builds_production_menu(torch_cuda):
    """The cases above are one per production kernel of the loaded build (each asserts that its plan selected that kernel): the
    menu they were drawn from has as many production entries as the library reports, with no name twice."""
    from aggfly_amd import hip
    info = hip.build_info()
    assert info["variants"] - info["arms"] == len(MENU) == len(BY_NAME)
