"""`keep_packed=True` datasets through `aggregate_dataset` on specs that reach the region-fused period ends of packed cubes: a daily
panel of degree days (`dd` by `date`: one output period per day) and the `tavg` polynomial summed by month.  A small int16 Zarr store —
20 days of hourly steps on 12 x 17 cells — read three ways: kept packed in HBM, unpacked to float32 in HBM, and on the host for the
oracle (`oracle.ref_aggregate`).  Not `exact_order`: the packed frame against the float32 device dataset's at 1e-12, both against the
oracle at 1e-10 (the figures of tests/test_gpu_packed.py for the fast routes)."""
import json
import os

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af
from aggfly_amd import synth
from oracle import ref_aggregate as ra

import packed_recipes as pr

pytestmark = pytest.mark.gpu

SPECS = {
    "daily_dd_panel": dict(dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]})]),
    "monthly_polynomial": dict(tavg=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 4)}),
                                     ("aggregate", {"calc": "sum", "groupby": "month"})]),
}


def _celsius(x):
    return x - 273.15


def _write_store(tmp_path, stored, time, ny, nx):
    from aggfly_amd import io as afio
    attrs = {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}
    tv, tattrs = afio._encode_time(time)
    store = str(tmp_path / "rf.zarr")
    os.makedirs(store)
    json.dump({"zarr_format": 2}, open(os.path.join(store, ".zgroup"), "w"))
    afio._write_array(store, "t2m", stored, ("time", "latitude", "longitude"), (48, ny, nx), attrs, None)
    afio._write_array(store, "time", np.asarray(tv, dtype=np.float64), ("time",), (len(time),), tattrs, None)
    afio._write_array(store, "latitude", 35 + 0.25 * np.arange(ny), ("latitude",), (ny,), {}, None)
    afio._write_array(store, "longitude", 250 + 0.25 * np.arange(nx), ("longitude",), (nx,), {}, None)
    return store


@pytest.mark.parametrize("case", list(SPECS))
def test_keep_packed_many_period_spec_through_the_public_api(torch_cuda, tmp_path, case):
    from aggfly_amd import engine as eng
    spec = SPECS[case]
    days, ny, nx = 20, 12, 17                                           # 204 cells; 20 days from 20 January: two months
    T = 24 * days
    rng = np.random.default_rng(len(case))
    stored = np.clip(np.rint(pr.stored_near(12.0) + rng.normal(0.0, 9.0, (T, ny, nx)) / 0.0017), -32766, 32766).astype(np.int16)
    stored[rng.random((T, ny, nx)) < 0.01] = -32767
    stored[:, 2, 3] = -32767                                            # an ocean cell
    stored[24 * 4:24 * 5, 5, 6] = -32767                                # a whole day of fills
    time = pd.date_range("2005-01-20", periods=T, freq="h")
    store = _write_store(tmp_path, stored, time, ny, nx)
    host = af.dataset_from_path(store, "t2m", preprocess=_celsius)
    plain = af.dataset_from_path(store, "t2m", device="cuda", preprocess=_celsius)
    packed = af.dataset_from_path(store, "t2m", device="cuda", keep_packed=True, preprocess=_celsius)
    assert packed.is_packed and not plain.is_packed and not host.is_packed
    tab = synth.weights_table(ny, nx, 6, seed=3, secondary=True)
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]}), regionid="geoid")
    ods = ra.ODataset(host.cube().astype(np.float64), host.time, host.latitude, host.longitude, True)
    ow = ra.OWeights(tab, np.arange(ny * nx), gr.shp["geoid"], "geoid", "nan")
    want = ra.aggregate_dataset(ow, ods, engine="numba", **spec)
    old = eng.config.exact_order
    try:
        eng.config.exact_order = False
        frames, descs = {}, {}
        for key, ds in (("packed", packed), ("plain", plain)):
            eng._PLAN_CACHE.clear()
            frames[key] = af.aggregate_dataset(dataset=ds, weights=af.weights_from_objects(ds, gr, table=tab), **spec)
            plans = list(eng._PLAN_CACHE.values())
            assert len(plans) == 1
            descs[key] = plans[0].describe()
    finally:
        eng.config.exact_order = old
        eng._PLAN_CACHE.clear()
    dp = descs["packed"]
    assert dp.startswith("variant=i16_p0_") and "storage=int16" in dp, dp
    if case == "daily_dd_panel":                                        # twenty periods: two cells per lane and the route
        assert "_v2_" in dp.split()[0] and "last-run=region-fused" in dp, dp
    cols = [c for c in want.columns if c not in ("geoid", "time")]
    got_p, got_f = frames["packed"], frames["plain"]
    assert list(got_p.columns) == list(want.columns) and len(got_p) == len(want)
    assert len(cols) == (1 if case == "daily_dd_panel" else 3) and got_p["time"].nunique() == (days if case == "daily_dd_panel" else 2)
    np.testing.assert_allclose(got_p[cols].values, got_f[cols].values, rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(got_p[cols].values, want[cols].values, rtol=1e-10, atol=0, equal_nan=True)
    np.testing.assert_allclose(got_f[cols].values, want[cols].values, rtol=1e-10, atol=0, equal_nan=True)
    assert np.isfinite(got_p[cols].values).any()
