"""Every route of the spatial stage on the hand-built weight tables of tests/weight_tables.py.

Routes: `CSR.scatter_block` (k_csr_spmm in table order), `CSR.wavg` (k_validity_panel, k_csr_spmm_wave<2|4|8|16> / k_csr_spmm by segment,
k_csr_combine_segments, k_panel_divide), fused plans on the region-fused period ends (k_rf_reduce), the slot gather
(k_csr_spmm_slots<KB, SUB>), the panel route and `exact_order`, and a bin-count plan on the packed-count gathers (k_csr_spmm_counts,
k_csr_spmm_counts_sub<4|8|16>).  Two value regimes (weight_tables' docstring): integers — every route bit-equal to `np.add.at` on int64 —
and reals — every route inside (n + 2) * 2^-52 * sum |w x| of the extended-precision sum.  On all routes res is bit-identical to num / den
of the same run where den != 0 and NaN where den == 0.  The plans' per-cell values are the plan's own (integer regime: equal to the values
worked out on the host); `plan.describe()` says which route a run took, and the tables that are there for the region-fused route must be seen on it.
"""
import numpy as np
import pandas as pd
import pytest

import weight_tables as wt
from aggfly_amd import synth
from oracle.ref_spatial import scatter_block as ref_scatter

pytestmark = pytest.mark.gpu

TABLES = wt.tables()
LIVE = [t for t in TABLES if t.regime != "refused"]
NAMES = [t.name for t in LIVE]
BY_NAME = {t.name: t for t in TABLES}

T_HOURS, DAYS = 144, 6
OB = np.array([0, 2, 2, 5, 6], dtype=np.int64)                        # four periods, the second one empty
COLS_SUM = [dict(inner="mean", outer="sum"), dict(inner="mean", transform="pow", transform_arg=2.0, outer="sum"),
            dict(inner="dd", inner_args=(10, 30, 0), outer="sum")]
COLS_MEAN = [dict(inner="mean", outer="mean")]
WAVG_SHAPES = ((1, 1), (1, 2), (2, 2), (3, 3), (7, 2), (16, 1), (2, 10))    # Q = (K + 1) nt = 2, 4, 6, 12, 16, 17, 30
BIN_EDGES = ((-20, -10), (-8, 0), (0, 7), (10, 22), (25, 45))
_cache = {}


def _regimes(t):
    return ("int", "real") if t.regime == "both" else ("real",)


def _weights(t, regime):
    return t.weight if regime == "int" else wt.real_weights(t)


def _csr(t, w):
    from aggfly_amd import hip
    return hip.CSR(t.region_idx, t.cell_idx, w, t.n_regions, t.n_cells)


def _check_sums(t, w, regime, X, got, what):
    """got [R, Q] against the reference of sum_j w_j X[cell_j]: bit for bit (integers) or inside the bound (reals)."""
    if regime == "int":
        want = wt.ref_int(t.region_idx, t.cell_idx, w, X, t.n_regions).astype(np.float64)
        bad = np.argwhere(got != want)
        assert not len(bad), f"{t.name} {what}: {len(bad)} sums differ from the int64 reference, first (region, column) {bad[0].tolist()}: " \
                             f"{got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
    else:
        E, A = wt.ref_ext(t.region_idx, t.cell_idx, w, X, t.n_regions)
        assert np.isfinite(got).all(), f"{t.name} {what}: non-finite sums"
        excess = wt.bound_excess(got, E, A, wt.row_lengths(t))
        assert excess <= 0, f"{t.name} {what}: {excess:.3e} beyond (n + 2) 2^-52 sum |w x|"


def _check_panel(t, w, regime, vals, out, what):
    """One run's num [K, R, P], den [R, P], res [K, R, P] against the per-cell values vals [K, C, P] (NaN = not valid)."""
    K, C, P = vals.shape
    valid = ~np.isnan(vals).any(axis=0)                                        # shared validity [C, P]
    X = np.concatenate([np.where(valid, vals[k], 0.0) for k in range(K)] + [valid.astype(np.float64)], axis=1)     # [C, (K + 1) P]
    num, den, res = (out[k].cpu().numpy() for k in ("num", "den", "res"))
    got = np.concatenate([num[k] for k in range(K)] + [den], axis=1)
    _check_sums(t, w, regime, X, got, what)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = num / den
    nz = np.broadcast_to(den != 0, num.shape)
    assert np.array_equal(res[nz].view(np.int64), q[nz].view(np.int64)), f"{t.name} {what}: res is not num / den of the same run"
    assert np.isnan(res[~nz]).all(), f"{t.name} {what}: res is not NaN where den == 0"
    if regime == "int":
        # den == 0 exactly: regions without entries, regions of zero weights, and regions whose weights cancel — the last wherever the
        # validity treats all their cells alike
        R = t.n_regions
        lo, hi = np.ones((R, P)), np.zeros((R, P))
        np.minimum.at(lo, t.region_idx, valid[t.cell_idx].astype(np.float64))
        np.maximum.at(hi, t.region_idx, valid[t.cell_idx].astype(np.float64))
        cancels = (np.bincount(t.region_idx, w, minlength=R) == 0)[:, None] & (lo >= hi)
        must_zero = cancels | (np.bincount(t.region_idx, np.abs(w), minlength=R) == 0)[:, None]
        assert (den[must_zero] == 0).all() and np.isnan(res[:, must_zero]).all(), f"{t.name} {what}: den != 0 for an empty, zero-weight or cancelling region"


def _check_table_order(t, w, vals, out, what):
    """`exact_order`: num and den bit for bit the oracle's scatter, in table order, on the per-cell values vals [K, C, P]."""
    valid = ~np.isnan(vals).any(axis=0)
    o = np.argsort(t.region_idx, kind="stable")
    tab = (t.region_idx[o], t.cell_idx[o], w[o], t.n_regions)
    num, den = out["num"].cpu().numpy(), out["den"].cpu().numpy()
    assert np.array_equal(den, ref_scatter(valid.astype(np.float64), *tab)), f"{t.name} {what}: den is not the sum in table order"
    for k in range(len(vals)):
        assert np.array_equal(num[k], ref_scatter(np.where(valid, vals[k], 0.0), *tab)), f"{t.name} {what}: num[{k}] is not the sum in table order"


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [t.name for t in TABLES if t.regime == "refused"])
def test_non_finite_weights_are_refused(torch_cuda, name):
    t = BY_NAME[name]
    with pytest.raises(ValueError, match="not finite"):
        _csr(t, t.weight)


@pytest.mark.parametrize("name", NAMES)
def test_scatter_block(torch_cuda, name):
    t = BY_NAME[name]
    for regime in _regimes(t):
        w = _weights(t, regime)
        csr = _csr(t, w)
        for nt in (1, 3, 17):
            X = wt.block_values(t.n_cells, nt, regime, seed=nt)
            got = csr.scatter_block(torch_cuda.from_numpy(X).cuda()).cpu().numpy()
            _check_sums(t, w, regime, X, got, f"scatter_block nt={nt} {regime}")
            o = np.argsort(t.region_idx, kind="stable")                        # table order inside each region
            assert np.array_equal(got, ref_scatter(X, t.region_idx[o], t.cell_idx[o], w[o], t.n_regions)), f"{name} nt={nt} {regime}: not table order"


def _wavg_input(C, K, nt, regime):
    x = wt.block_values(C, K * nt, regime, seed=K * 100 + nt).reshape(C, K, nt).transpose(1, 0, 2).copy()
    bad = wt.nan_cells(C)
    x[bad % K, bad, bad % nt] = np.nan
    x[:, bad[::11], :] = np.nan
    return x


@pytest.mark.parametrize("name", NAMES)
def test_wavg(torch_cuda, monkeypatch, name):
    t = BY_NAME[name]
    segs = (None, "128") if name == "row_lengths" else (None,)                 # (the knob is read when the CSR is created)
    for regime in _regimes(t):
        w = _weights(t, regime)
        for seg in segs:
            if seg:
                monkeypatch.setenv("AFHIP_SPMM_SEG", seg)
            csr = _csr(t, w)
            monkeypatch.delenv("AFHIP_SPMM_SEG", raising=False)
            for K, nt in WAVG_SHAPES:
                x = _wavg_input(t.n_cells, K, nt, regime)
                num, den, res = csr.wavg(torch_cuda.from_numpy(x).cuda())
                _check_panel(t, w, regime, x, dict(num=num, den=den, res=res), f"wavg K={K} nt={nt} seg={seg} {regime}")
                if (K, nt) == (3, 3):                                          # the divide on its own (k_divide_num_den): the same bits
                    from aggfly_amd import hip
                    assert np.array_equal(hip.panel_divide(num, den).cpu().numpy(), res.cpu().numpy(), equal_nan=True), f"{name} {regime}: panel_divide"


@pytest.mark.parametrize("K,nt", [(17, 1), (17, 4), (23, 3)])
def test_wavg_of_more_names_than_one_pass_holds(torch_cuda, K, nt):
    """`aggregate_dataset` on a spec of more than sixteen columns gathers the passes' outputs and hands all K of them to ONE
    `CSR.wavg` (found by tests/test_gpu_packed_fuzz.py, seed 10: seventeen columns): the divide then reads records of K + 1 > 17 sums."""
    for name in ("row_lengths", NAMES[0]):
        t = BY_NAME[name]
        for regime in _regimes(t):
            w = _weights(t, regime)
            x = _wavg_input(t.n_cells, K, nt, regime)
            num, den, res = _csr(t, w).wavg(torch_cuda.from_numpy(x).cuda())
            _check_panel(t, w, regime, x, dict(num=num, den=den, res=res), f"wavg K={K} nt={nt} {regime}")
            assert np.isfinite(res.cpu().numpy()[K - 1]).any()


def test_segment_rule_piece_counts(torch_cuda, monkeypatch):
    """The pieces `afhip_csr_create` cuts the rows of the row-length table into, read off the scratch rows a run's workspace holds for them
    (sums [R + pieces][Q]): 234 with the default segment length — 257 -> 5, 320 -> 5, 321 -> 6, 511 -> 8, 512 -> 8, 513 -> 9, 8192 -> 128,
    8193 -> 65 — and with AFHIP_SPMM_SEG=128, where 512 stays whole and 513 is cut in 5."""
    from aggfly_amd import hip
    t = BY_NAME["row_lengths"]
    # seven columns, four periods: a row of the sums is (K + 1) P = 32 doubles = 256 bytes, the unit the library rounds the sums area up
    # to — so the rounding changes nothing and every scratch row shows as exactly 256 bytes of workspace
    plan = hip.FusedPlan(T_HOURS, t.n_cells, hip.F64, synth.hourly_bounds(T_HOURS), np.array([0, 2, 4, 5, 6], dtype=np.int64), COLS_SUM + COLS_SUM + COLS_SUM[:1])
    Q = 8 * 4
    assert Q * 8 == 256
    none = hip.CSR([], [], [], t.n_regions, t.n_cells)                          # the same regions, no piece
    for seg in (None, "128"):
        if seg:
            monkeypatch.setenv("AFHIP_SPMM_SEG", seg)
        csr = _csr(t, t.weight)
        monkeypatch.delenv("AFHIP_SPMM_SEG", raising=False)
        pieces = sum(wt.pieces_of(n, int(seg or 64)) for n in wt.ROW_LENGTHS if n > 4 * int(seg or 64))
        assert pieces == (234 if seg is None else 5 + 64 + 65)
        got = plan.workspace_bytes(csr) - plan.workspace_bytes(none)
        assert got == pieces * 256, f"seg={seg}: {got / 256:.1f} scratch rows, {pieces} pieces by the rule"


# ---------------------------------------------------------------------------------------------------------------------------------
# fused plans
# ---------------------------------------------------------------------------------------------------------------------------------
def _cube(torch, C, dtype, regime):
    key = ("cube", C, np.dtype(dtype).name, regime)
    if key not in _cache:
        v = wt.day_values(C, DAYS, regime)
        host = wt.cube_of_days(v, 24, dtype, jitter=regime == "real")
        _cache[key] = (v, torch.from_numpy(host).cuda())
    return _cache[key]


def _host_cells(v, cols):
    """The per-cell period values [K, C, P] of the integer regime, worked out on the host from the day values v [days, C]."""
    out = []
    for c in cols:
        if c["inner"] == "dd":
            t0, t1 = c["inner_args"][:2]
            d = np.where(np.isnan(v), np.nan, np.where((v > t0) & (v < t1), 24.0 * np.abs(v - t0), 0.0))
        else:
            d = v ** 2 if c.get("transform") == "pow" else v
        per = []
        for p in range(len(OB) - 1):
            if OB[p + 1] == OB[p]:
                per.append(np.full(v.shape[1], np.nan))
            else:
                s = d[OB[p]:OB[p + 1]].sum(axis=0)
                per.append(s / (OB[p + 1] - OB[p]) if c["outer"] == "mean" else s)
        out.append(np.stack(per, axis=1))
    return np.stack(out)


VARIATIONS = (
    # name, environment, exact_order, the route `describe()` must name after the run (None: region-fused where the table fits it, else the
    # slot gather).  The slot gather and the panel route come after the region-fused route in the library's choice, so their knobs are
    # set with that route switched off: alone they would not be reached on a table that fits it.
    ("default", {}, False, None),
    ("rf-run-major", {"AFHIP_RF_LAYOUT": "r"}, False, None),
    ("no-region-fused", {"AFHIP_NO_REGION_FUSED": "1"}, False, "slot-gather"),
    ("no-slot-spmm", {"AFHIP_NO_REGION_FUSED": "1", "AFHIP_NO_SLOT_SPMM": "1"}, False, "panel"),
    ("exact-order", {}, True, "panel"),
) + tuple((f"slots-sub{sub}-{order}", {"AFHIP_NO_REGION_FUSED": "1", "AFHIP_SLOT_SPMM_SUB": str(sub), "AFHIP_SLOT_SPMM_ORDER": order}, False, "slot-gather")
          for sub in (8, 64) for order in ("v", "p"))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_fused_plans(torch_cuda, monkeypatch, name, dtype):
    from aggfly_amd import hip
    t = BY_NAME[name]
    C = t.n_cells
    code = hip.F64 if dtype == np.float64 else hip.F32
    ib = synth.hourly_bounds(T_HOURS)
    seen = []
    for regime in _regimes(t):
        w = _weights(t, regime)
        csrs = [("", _csr(t, w))]
        if name == "row_lengths":                                              # segments of 128: 512 whole, 513 cut in 5
            monkeypatch.setenv("AFHIP_SPMM_SEG", "128")
            csrs.append((" seg=128", _csr(t, w)))
            monkeypatch.delenv("AFHIP_SPMM_SEG")
        v, cube = _cube(torch_cuda, C, dtype, regime)
        for cols in (COLS_SUM, COLS_MEAN):
            for (vname, env, exact, route), (seg, csr) in ((a, b) for a in VARIATIONS for b in csrs):
                for k, val in env.items():
                    monkeypatch.setenv(k, val)
                plan = hip.FusedPlan(T_HOURS, C, code, ib, OB, cols, exact_order=exact)
                for k in env:
                    monkeypatch.delenv(k)
                what = f"{vname}{seg} K={len(cols)} {regime} {np.dtype(dtype).name}"
                out = plan.run(cube, csr, want_cells=exact)
                desc = plan.describe()
                cells = (out["cells"] if exact else plan.run_temporal(cube)).cpu().numpy().transpose(0, 2, 1)      # [K, C, P]
                if regime == "int":
                    assert np.array_equal(cells, _host_cells(v, cols), equal_nan=True), f"{name} {what}: per-cell values differ from the host's"
                _check_panel(t, w, regime, cells, out, what)
                rf = "last-run=region-fused" in desc
                if vname in ("default", "rf-run-major"):
                    assert "region-fused-capable" in desc or rf, f"{name} {what}: the plan is not region-fused-capable: {desc}"
                    if t.expect["rf"] is not None:
                        assert rf == t.expect["rf"], f"{name} {what}: expected region-fused={t.expect['rf']} ({t.expect['why']}): {desc}"
                    if rf:
                        seen.append(desc.split()[0])
                    else:
                        assert "last-run=slot-gather" in desc, f"{name} {what}: {desc}"
                else:
                    assert f"last-run={route}" in desc.split(), f"{name} {what}: {desc}"
                if exact:
                    _check_table_order(t, w, cells, out, what)
    if t.expect["rf"]:
        # both run-table widths of `rf_table()` were built and read: the float64 plans and the one-column float32 plan hold one cell per
        # lane (64-cell tiles), the three-column float32 plan two (128-cell tiles)
        assert any("_v1_" in s for s in seen), (name, seen)
        assert dtype == np.float64 or any("_v2_" in s for s in seen), (name, seen)


@pytest.mark.parametrize("name", NAMES)
def test_bin_count_plan(torch_cuda, monkeypatch, name):
    """A daily cube, three yearly periods of four days, five bins: the packed-count gathers at one, four, eight and sixteen lanes per
    (row, period) pair and in table order.  Counts are integers: with integer weights this is the integer regime as it stands."""
    from aggfly_amd import hip
    t = BY_NAME[name]
    C = t.n_cells
    v = wt.day_values(C, 12, "int", seed=5)                                    # NaN days are out of every bin, never NaN
    key = ("daily", C)
    if key not in _cache:
        _cache[key] = torch_cuda.from_numpy(wt.cube_of_days(v, 1, np.float32)).cuda()
    cube = _cache[key]
    yb = np.array([0, 4, 8, 12], dtype=np.int64)
    cols = [dict(inner="bins", inner_args=(lo, hi, 0)) for lo, hi in BIN_EDGES]
    with np.errstate(invalid="ignore"):
        counts = np.stack([np.stack([((v[yb[p]:yb[p + 1]] > lo) & (v[yb[p]:yb[p + 1]] < hi)).sum(axis=0).astype(np.float64) for p in range(3)], axis=1)
                           for lo, hi in BIN_EDGES])                           # [K, C, P]
    for regime in _regimes(t):
        w = _weights(t, regime)
        csr = _csr(t, w)
        for sub, exact in ((0, False), (4, False), (8, False), (16, False), (None, True)):
            if sub is not None:
                monkeypatch.setenv("AFHIP_COUNTS_SPMM_SUB", str(sub))
            plan = hip.FusedPlan(12, C, hip.F32, yb, np.arange(4, dtype=np.int64), cols, exact_order=exact)
            monkeypatch.delenv("AFHIP_COUNTS_SPMM_SUB", raising=False)
            out = plan.run(cube, csr)
            desc = plan.describe()
            assert "packed-counts" in desc and f"last-run=count-gather/{sub or 1}-lane" in desc, desc
            _check_panel(t, w, regime, counts, out, f"bins sub={sub} exact={exact} {regime}")
            if exact:
                _check_table_order(t, w, counts, out, f"bins exact {regime}")
            if regime == "int" and sub == 0:
                cells = plan.run_temporal(cube).cpu().numpy().transpose(0, 2, 1)
                assert np.array_equal(cells, counts), f"{name}: per-cell counts differ from the host's"


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groupby", ["month", "year"])
def test_everything_table_through_aggregate_dataset(torch_cuda, groupby):
    """One table with empty regions, a cut row, junction cells, a zero-weight region and a cancelling pair, laid over a 0-360 dataset (the
    engine folds the longitude permutation into the columns: rotated order), through the public entry — grouped by month (three periods:
    the region-fused route) and by year (one period) — against `oracle.ref_aggregate`.  Day values are integers repeated over the day's
    steps and the weights are multiples of 1 / 1024, so every sum is exact whatever its order: the rows that are kept and dropped and every
    value must equal the oracle's bit for bit (which is inside the bound of the real regime a fortiori)."""
    import aggfly_amd as af
    from aggfly_amd import engine as eng
    from oracle import ref_aggregate as ra
    ny, nx = wt.LARGE
    days = 42                                                                   # 20 January .. 1 March: three months
    v = wt.day_values(ny * nx, days, "int", seed=9)
    cube = wt.cube_of_days(v, 4, np.float64).reshape(days * 4, ny, nx)          # 6-hourly steps: no month is long enough to be cut into chunks
    time = pd.date_range("2003-01-20", periods=days * 4, freq="6h")
    lat, lon = 20.0 + 0.25 * np.arange(ny), (np.arange(nx) + 0.5) * 360.0 / nx
    r, c, w, R = wt.everything_table()
    tab = pd.DataFrame({"cell_id": c, "index_right": r, "weight": w})
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i:02d}" for i in range(R)]}), regionid="geoid")
    spec = dict(dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": groupby})],
                tavg=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 3)}),
                      ("aggregate", {"calc": "sum", "groupby": groupby})])
    ds = af.Dataset(af.DataArray(data=cube, dims=["time", "latitude", "longitude"], coords={"time": time, "latitude": lat, "longitude": lon}), lon_is_360=True)
    wts = af.weights_from_objects(ds, gr, table=tab)
    want = ra.aggregate_dataset(ra.OWeights(tab, np.arange(ny * nx), gr.shp["geoid"], "geoid", "nan"), ra.ODataset(cube, time, lat, lon, True),
                                engine="numba", **spec)
    old = eng.config.exact_order
    try:
        eng.config.exact_order = False
        eng._PLAN_CACHE.clear()
        got = af.aggregate_dataset(dataset=ds.to_device(), weights=wts, **spec)
        descs = [p.describe() for p in eng._PLAN_CACHE.values()]
    finally:
        eng.config.exact_order = old
        eng._PLAN_CACHE.clear()
    assert len(descs) == 1 and ("last-run=region-fused" in descs[0]) == (groupby == "month"), descs
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    assert (got["geoid"].values == want["geoid"].values).all() and (got["time"].values == want["time"].values).all()
    cols = [k for k in got.columns if k not in ("geoid", "time")]
    assert np.array_equal(got[cols].values, want[cols].values, equal_nan=True)
    # the rows: no empty region, the zero-weight and the cancelling region as NaN rows, every other region with values
    assert set(got["geoid"]) == {f"r{i:02d}" for i in (1, 2, 3, 4, 7, 8, 9, 10, 11, 12, 13, 14)}
    nan_rows = got[cols].isna().all(axis=1)
    assert set(got.loc[nan_rows, "geoid"]) == {"r03", "r14"} and got.loc[~nan_rows, cols].notna().all().all()
