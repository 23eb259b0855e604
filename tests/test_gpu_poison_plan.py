"""A `FusedPlan`'s results do not depend on what its workspace and its outputs held before the run.

Every production variant of the loaded build runs through the existing test of its menu (`test_gpu_variant_menu`, `test_gpu_packed`,
`_packed_hist`, `_packed_short`, `_packed_rf`, `_end_bins`, `_cell_map`: its recipe, its oracle, its bars, unchanged), and the four
spatial routes of `afhip_plan_run` through the existing route tests of tests/test_gpu_weight_tables.py (region-fused in both layouts,
count gather in table order and at 4, 8 and 16 lanes, slot gather, panel + spmm with whole and cut rows, each confirmed there by
`describe()`) on the smallest tables with empty regions, zero weights, cells in three or more regions and a row that is cut.  While
such a test runs, every `run_temporal` (afhip_plan_run_temporal) and `run` (afhip_plan_run) of a plan is executed once per fill of tests/poison.py — a fresh workspace and fresh
outputs from a poisoned `torch.empty` each time, one fill twice first — and once more in an explicit `workspace=` that is larger than
needed and filled; all results must be the same bits, and the existing test then holds the last of them to its own expectation.
(The kernels use no float atomics on global memory: bitwise equality is the derived expectation.)

The reuse test keeps one plan and one caller-owned workspace, never refilled, through per-cell and gather runs, a second table with
more and cut rows, the first table again, a second cube and a rebound packing rule, each step against a fresh plan on a zeroed
workspace."""
import numpy as np
import pytest

import poison
import weight_tables as wt

pytestmark = pytest.mark.gpu

ORDER = ("random", "random", "zero", "ones", "plausible")       # one fill twice first, then the others


def _bits_equal(torch, a, b):
    if isinstance(a, dict):
        return set(a) - {"kernel_ms"} == set(b) - {"kernel_ms"} and all(_bits_equal(torch, a[k], b[k]) for k in a if k != "kernel_ms")
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)))


def _keep(r):
    return {k: v.clone() for k, v in r.items() if k != "kernel_ms"} if isinstance(r, dict) else r.clone()


@pytest.fixture
def every_fill(torch_cuda, monkeypatch):
    """While the test runs, `FusedPlan.run_temporal` and `FusedPlan.run` execute under every fill and compare their results bit for
    bit.  -> a dict that counts the runs."""
    from aggfly_amd import hip
    torch = torch_cuda
    real = {"run_temporal": hip.FusedPlan.run_temporal, "run": hip.FusedPlan.run}
    count = {"run_temporal": 0, "run": 0, "explicit": 0}

    def under_fills(plan, name, call, explicit=None):
        first = None
        for fill in ORDER:
            with pytest.MonkeyPatch.context() as mp:
                handed = poison.poisoned_empty(mp, torch, fill)
                plan._ws = None                                   # a fresh block of the (poisoned) allocator, not the last run's
                r = call()
                assert handed, "the run took nothing from torch.empty"
            if first is None:
                first = _keep(r)
            else:
                assert _bits_equal(torch, first, r), f"{plan.describe()}: {name} under {fill!r} differs from the first run"
        if explicit is not None:
            r = explicit()
            assert _bits_equal(torch, first, r), f"{plan.describe()}: {name} in an explicit filled workspace differs"
            count["explicit"] += 1
        count[name] += 1
        return r

    def run_temporal(self, cube):
        return under_fills(self, "run_temporal", lambda: real["run_temporal"](self, cube))

    def run(self, cube, csr, want_cells=False, timed=False, out=None, workspace=None):
        if out is not None or workspace is not None:              # the caller's own buffers: as the caller says
            return real["run"](self, cube, csr, want_cells=want_cells, timed=timed, out=out, workspace=workspace)
        big = lambda: poison.filled(torch, self.workspace_bytes(csr) + 4096 + 256 * 7, "random")
        return under_fills(self, "run", lambda: real["run"](self, cube, csr, want_cells=want_cells, timed=timed),
                           lambda: real["run"](self, cube, csr, want_cells=want_cells, timed=timed, workspace=big()))

    monkeypatch.setattr(hip.FusedPlan, "run_temporal", run_temporal)
    monkeypatch.setattr(hip.FusedPlan, "run", run)
    return count


# ---------------------------------------------------------------------------------------
# every production variant, by the existing test of its menu
# ---------------------------------------------------------------------------------------
def _menus():
    import test_gpu_cell_map as cm
    import test_gpu_end_bins as eb
    import test_gpu_packed as pk
    import test_gpu_packed_hist as ph
    import test_gpu_packed_rf as prf
    import test_gpu_packed_short as ps
    import test_gpu_variant_menu as vm
    return {"float": (vm.MENU, lambda t, mp, n: vm.test_variant_against_the_oracle(t, n)),
            "packed": (pk.MENU, lambda t, mp, n: pk.test_packed_variant_against_the_oracle(t, n)),
            "packed_hist": (ph.MENU, lambda t, mp, n: ph.test_packed_hist_variant_against_the_oracle(t, n)),
            "packed_short": (ps.MENU, lambda t, mp, n: ps.test_kernel_against_its_float32_twin_and_the_oracle(t, n)),
            "packed_rf": (prf.MENU, lambda t, mp, n: prf.test_twin_against_the_per_cell_routes_the_float32_twin_and_the_oracle(t, mp, n)),
            "end_bins": (eb.MENU, lambda t, mp, n: eb.test_end_bins_variant_against_the_oracle(t, n)),
            "cell_map": (cm.MENU, lambda t, mp, n: cm.test_cell_map_variant_against_the_oracle(t, n))}


MENUS = _menus()
CASES = [(key, v.name) for key, (menu, _) in MENUS.items() for v in menu]


@pytest.mark.parametrize("menu,name", CASES, ids=[f"{k}-{n}" for k, n in CASES])
def test_variant_under_every_fill(torch_cuda, monkeypatch, every_fill, menu, name):
    MENUS[menu][1](torch_cuda, monkeypatch, name)
    assert every_fill["run_temporal"] + every_fill["run"] >= 1
    if menu == "float" and name.endswith("_rf"):                  # a region-fused twin: run(..., csr) with and without want_cells
        assert every_fill["run"] >= 2 and every_fill["explicit"] >= 2


def test_the_cases_cover_every_menu_of_the_loaded_build(torch_cuda):
    from aggfly_amd import hip
    info = hip.build_info()
    assert len({c for c in CASES}) == len(CASES)
    assert sum(k == "float" for k, _ in CASES) == info["variants"] - info["arms"]
    for key in ("packed", "packed_hist", "packed_short", "packed_rf", "end_bins", "cell_map"):
        assert 0 < sum(k == key for k, _ in CASES) <= hip.menu_size(key), key


# ---------------------------------------------------------------------------------------
# the four spatial routes, on purpose
# ---------------------------------------------------------------------------------------
def _route_tables():
    """The smallest live table of tests/weight_tables.py with each property a skipped store can hide behind."""
    live = [t for t in wt.tables() if t.regime != "refused" and len(t.cell_idx)]
    smallest = lambda ok: min((t for t in live if ok(t)), key=lambda t: len(t.cell_idx)).name
    picked = {"an empty region": smallest(lambda t: (wt.row_lengths(t) == 0).any()),
              "zero weights": smallest(lambda t: (np.asarray(t.weight) == 0).any()),
              "a cell in three or more regions": smallest(lambda t: wt.regions_per_cell(t).max() >= 3),
              "a row that is cut": smallest(lambda t: wt.row_lengths(t).max() > 8192)}
    return picked


ROUTE_TABLES = _route_tables()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("table", sorted(set(ROUTE_TABLES.values())))
def test_region_fused_slot_gather_and_panel_routes_under_every_fill(torch_cuda, monkeypatch, every_fill, table, dtype):
    """`test_fused_plans`: default and run-major region-fused, slot gather at every lane count and order, panel + spmm by the knob and by
    exact order, on the cut-row table also with segments of 128 (the second combine kernel), several periods with an empty one."""
    import test_gpu_weight_tables as W
    W.test_fused_plans(torch_cuda, monkeypatch, table, dtype)
    assert every_fill["run"] >= 2 * len(W.VARIATIONS) and every_fill["explicit"] == every_fill["run"]


@pytest.mark.parametrize("table", sorted(set(ROUTE_TABLES.values())))
def test_count_gather_routes_under_every_fill(torch_cuda, monkeypatch, every_fill, table):
    """`test_bin_count_plan`: the packed-count gather in the table's order and at 4, 8 and 16 lanes per pair."""
    import test_gpu_weight_tables as W
    W.test_bin_count_plan(torch_cuda, monkeypatch, table)
    assert every_fill["run"] >= 5


def test_the_route_tables_have_what_they_were_picked_for():
    by = {t.name: t for t in wt.tables()}
    assert (wt.row_lengths(by[ROUTE_TABLES["an empty region"]]) == 0).any()
    assert (np.asarray(by[ROUTE_TABLES["zero weights"]].weight) == 0).any()
    assert wt.regions_per_cell(by[ROUTE_TABLES["a cell in three or more regions"]]).max() >= 3
    assert wt.pieces_of(int(wt.row_lengths(by[ROUTE_TABLES["a row that is cut"]]).max()), 128) > 1


# ---------------------------------------------------------------------------------------
# one plan, one workspace, never refilled
# ---------------------------------------------------------------------------------------
def _csr(t, monkeypatch=None, seg=None):
    from aggfly_amd import hip
    if seg:
        monkeypatch.setenv("AFHIP_SPMM_SEG", str(seg))
    try:
        return hip.CSR(t.region_idx, t.cell_idx, wt.real_weights(t), t.n_regions, t.n_cells)
    finally:
        if seg:
            monkeypatch.delenv("AFHIP_SPMM_SEG")


def _reuse_cases(torch):
    """name -> (make_plan(), [cube, second cube], bind(plan, which) or None, the route describe() must name without want_cells)."""
    import aggfly_amd as af
    from aggfly_amd import hip, synth
    import packed_recipes as pr
    C = 9230
    T = 24 * 6
    ib = synth.hourly_bounds(T)
    ob = np.array([0, 2, 2, 5, 6], dtype=np.int64)
    rng = np.random.default_rng(12)
    f64 = [torch.from_numpy(wt.cube_of_days(wt.day_values(C, 6, "real", seed=s), 24, np.float64, jitter=True)).cuda() for s in (0, 1)]
    cols = [dict(inner="mean", outer="sum"), dict(inner="mean", transform="pow", transform_arg=2.0, outer="sum"), dict(inner="dd", inner_args=(10, 30, 0), outer="sum")]
    q = [torch.from_numpy(rng.integers(-20000, 20000, size=(12, C)).astype(np.int16)).cuda() for _ in (0, 1)]
    for x in q:
        x[:, ::97] = pr.FILL
    q = [af.PackedCube(x.reshape(12, 1, C), scale_factor=0.0017, add_offset=281.3, fill_value=pr.FILL) for x in q]      # (the plan reads the rule it was bound)
    rules = [hip.Packing(2, 1, pr.FILL, 0, (0.0017, 1.0, 1.0), (281.3 - 273.15, -0.0, -0.0)), hip.Packing(1, 1, pr.FILL, 0, (0.0021, 1.0, 1.0), (3.5, -0.0, -0.0))]
    edges = [(-30 + 5 * k, -25 + 5 * k, 0) for k in range(12)]
    bins = [dict(inner="bins", inner_args=e) for e in edges]
    yb = np.array([0, 4, 8, 12], dtype=np.int64)
    return {
        "float64 one period": (lambda: hip.FusedPlan(T, C, hip.F64, ib, np.array([0, 6], dtype=np.int64), cols), f64, None, "slot-gather"),
        "int16 bins": (lambda: hip.FusedPlan(12, C, hip.I16, yb, np.arange(4, dtype=np.int64), bins), q, lambda p, i: p.bind_packing(rules[i]), "count-gather"),
        "float64 periods region-fused": (lambda: hip.FusedPlan(T, C, hip.F64, ib, ob, cols), f64, None, "region-fused"),
    }


@pytest.mark.parametrize("case", ["float64 one period", "int16 bins", "float64 periods region-fused"])
def test_one_plan_and_one_workspace_never_refilled(torch_cuda, monkeypatch, case):
    torch = torch_cuda
    by = {t.name: t for t in wt.tables()}
    t1, t2 = by["five_regions"], by["row_lengths"]
    assert t1.n_cells == t2.n_cells and t2.n_regions > t1.n_regions and wt.row_lengths(t2).max() > 8 * 128
    csr1, csr2 = _csr(t1), _csr(t2, monkeypatch, seg=128)
    make, cubes, bind, route = _reuse_cases(torch)[case]
    plan = make()
    if bind:
        bind(plan, 0)
    nbytes = max(plan.workspace_bytes(csr1), plan.workspace_bytes(csr2)) + 8192
    ws = poison.filled(torch, nbytes, "random")
    steps = [("want_cells", cubes[0], csr1, True, 0), ("gather", cubes[0], csr1, False, 0), ("more and cut rows", cubes[0], csr2, False, 0),
             ("more and cut rows, cells", cubes[0], csr2, True, 0), ("the first table again", cubes[0], csr1, False, 0),
             ("a second cube", cubes[1], csr1, False, 0), ("a second cube, cells", cubes[1], csr2, True, 0)]
    if bind:
        steps += [("a rebound rule", cubes[1], csr1, False, 1), ("a rebound rule, cells", cubes[0], csr2, True, 1), ("the first rule again", cubes[0], csr1, False, 0)]
    seen = set()
    for what, cube, csr, want_cells, rule in steps:
        if bind:
            bind(plan, rule)
        got = plan.run(cube, csr, want_cells=want_cells, workspace=ws)
        desc = plan.describe()
        seen.add(desc.split("last-run=")[1].split()[0])
        fresh = make()
        if bind:
            bind(fresh, rule)
        want = fresh.run(cube, csr, want_cells=want_cells, workspace=torch.zeros(nbytes, dtype=torch.uint8, device="cuda"))
        assert fresh.describe().split("last-run=")[1].split()[0] == desc.split("last-run=")[1].split()[0]
        assert _bits_equal(torch, want, got), f"{case}: {what}: {desc}"
        fresh.close()
    assert any(s.startswith(route) for s in seen) and "panel" in seen, seen
