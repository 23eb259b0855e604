"""Randomised spec fuzz on PACKED cubes: the packed counterpart of tests/test_gpu_fuzz.py.  `packed_fuzz.case(seed)` draws an int16 /
uint16 cube with one to four unpack rules, a `preprocess` that folds into them, a calendar with gaps, and four to seven specs; every
spec runs through `aggregate_dataset` three ways — the oracle on the host-unpacked values, the product on the packed dataset (built in
memory, or for a quarter of the seeds read from a multi-store Zarr with `keep_packed=True` and a time selection across the first rule
boundary) and the product on a plain float32 dataset of the host values.

Held: equal labels in the three frames; packed and plain against the oracle, and packed against plain, at the float fuzz's bars
(rtol = atol = 1e-10); every plan that reads the cube says its storage and none of the packed run has a float dtype on the cube's time
axis (later steps of a staged name read float step outputs: those plans are told apart by their `T=`), nor is the cube ever
materialised; every seed reaches its stratum's kernel family; over the seed list one, two and four cells per lane and both storages
occur.  A spec is never skipped: what the library refuses on a packed cube must be accepted on the plain one, be refused as
`HipUnsupported` / `ValueError` with a message, and stay below one trial in ten.  The largest packed-against-plain and
packed-against-oracle differences per seed go into packed_fuzz_census.json beside the reports of tests/test_gpu_sine_fixtures.py, when
that directory exists (`_report_dir`)."""
import glob
import json
import os
import re

import numpy as np
import pandas as pd
import pytest

import aggfly_amd as af

import packed_fuzz as pf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RTOL = ATOL = 1e-10           # tests/test_gpu_fuzz.py
_RESULTS = {}


def _report_dir():
    """The run's output directory — the `*_out` directory at the repository's root that tests/test_gpu_sine_fixtures.py writes its
    error reports into — or None where there is none."""
    found = sorted(d for d in glob.glob(os.path.join(os.path.dirname(HERE), "*_out")) if os.path.isdir(d))
    return found[0] if found else None


def _packed_dataset(c, tmp_path):
    """The packed dataset of case `c` in HBM."""
    from aggfly_amd import io as afio
    fn = pf.PREPROCESS_FN[c.preprocess]
    if c.build == "zarr":
        ny, nx = c.bits.shape[1:]
        paths = []
        for i, ((s, o, f), a, b) in enumerate(zip(c.rules, c.bounds[:-1], c.bounds[1:])):
            attrs = {"scale_factor": s}
            if o is not None:
                attrs["add_offset"] = o
            if f is not None:
                attrs["_FillValue"] = f
            stored = c.bits[a:b].view(np.uint16) if c.unsigned else c.bits[a:b]
            tv, tattrs = afio._encode_time(c.full_time[np.arange(a, b)])
            store = str(tmp_path / f"part{i}.zarr")
            os.makedirs(store)
            json.dump({"zarr_format": 2}, open(os.path.join(store, ".zgroup"), "w"))
            comp = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0} if (c.seed + i) % 2 else None
            afio._write_array(store, "t2m", stored, ("time", "latitude", "longitude"), (48, ny, nx), attrs, comp)
            afio._write_array(store, "time", np.asarray(tv, dtype=np.float64), ("time",), (b - a,), tattrs, None)
            afio._write_array(store, "latitude", c.lat, ("latitude",), (ny,), {}, None)
            afio._write_array(store, "longitude", c.lon, ("longitude",), (nx,), {}, None)
            paths.append(store)
        ds = af.dataset_from_path(paths, "t2m", device="cuda", keep_packed=True, preprocess=fn, lon_is_360=c.lon360,
                                  time_sel=slice(c.time[0], c.time[-1]))
        assert len(ds.time) == len(c.time) and (pd.DatetimeIndex(ds.time) == c.time).all()
        return ds
    if c.build == "concat":          # parts of different packings joined, as the loaders join the stores of a record
        cube = af.PackedCube.concat([af.PackedCube(np.ascontiguousarray(c.bits[a:b]), s, o, f, unsigned=c.unsigned)
                                     for (s, o, f), a, b in zip(c.rules, c.bounds[:-1], c.bounds[1:])])
    else:                            # the rules and their bounds, as `io.packed_rules_of` hands them on
        f32 = lambda x: None if x is None else np.float32(x)      # noqa: E731
        cube = af.PackedCube(c.bits, unsigned=c.unsigned, _rules=[([(f32(s), f32(o))], f) for s, o, f in c.rules], _bounds=c.bounds)
    da = af.DataArray(cube, ["time", "latitude", "longitude"], {"time": c.time, "latitude": c.lat, "longitude": c.lon})
    return af.Dataset(da, lon_is_360=c.lon360, preprocess=fn).to_device()


def _labels_equal(c, a, b):
    if isinstance(c.time, pd.DatetimeIndex):
        return bool((a["time"].values == b["time"].values).all())
    return [(t.year, t.month, t.day) for t in a["time"]] == [(t.year, t.month, t.day) for t in b["time"]]


def _max_diff(a, b):
    """(largest absolute, largest relative) difference over the cells where both are finite."""
    ok = np.isfinite(a) & np.isfinite(b)
    if not ok.any():
        return 0.0, 0.0
    d = np.abs(a[ok] - b[ok])
    return float(d.max()), float((d / np.maximum(np.abs(b[ok]), 1e-300)).max())


def _variants(descs):
    return [d.split()[0][len("variant="):] for d in descs]


def _on_cube(descs, T):
    return [d for d in descs if int(re.search(r"\bT=(\d+)", d).group(1)) == T]


def _family_reached(stratum, descs):
    names = _variants(descs)
    if stratum == "general":
        return any(n.startswith("i16_") and "_pair" not in n and "_hist" not in n for n in names)
    if stratum == "short":
        return any("_pair" in n for n in names)
    if stratum == "hist-equal":
        return any("_hist" in n and "_ends" not in n for n in names)
    if stratum == "hist-ends":
        return any("_ends" in n and "_cmap" not in n for n in names)
    if stratum == "hist-cellmap":
        return any("_cmap" in n for n in names)
    if stratum == "region-fused":
        return any("last-run=region-fused" in d for d in descs)
    if stratum == "wide":
        return len(descs) >= 2
    raise KeyError(stratum)


def _run_seed(seed, tmp_path, monkeypatch):
    import torch
    from aggfly_amd import engine as eng
    from aggfly_amd import hip
    c = pf.case(seed)
    T = len(c.time)
    packed = _packed_dataset(c, tmp_path)
    assert packed.is_packed and packed.packed_cube().storage == c.storage and packed.packed_cube().q.is_cuda
    assert packed.packed_cube().n_rules == sum(b > a for a, b in zip(c.window_bounds[:-1], c.window_bounds[1:]))
    plain = af.Dataset(af.DataArray(torch.from_numpy(c.host).cuda(), ["time", "latitude", "longitude"],
                                    {"time": c.time, "latitude": c.lat, "longitude": c.lon}), lon_is_360=c.lon360)
    assert not plain.is_packed
    gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i}" for i in range(int(c.tab.index_right.max()) + 1)]}))
    weights = {"packed": af.weights_from_objects(packed, gr, table=c.tab), "plain": af.weights_from_objects(plain, gr, table=c.tab)}
    materialised = []
    real = af.PackedCube.materialize
    monkeypatch.setattr(af.PackedCube, "materialize", lambda self: (materialised.append(1), real(self))[1])
    rec = {"stratum": c.stratum, "storage": c.storage, "build": c.build, "rules": len(c.rules), "variants": [], "routes": [], "refusals": [],
           "trials": 0, "reached": False, "max_packed_vs_plain": [0.0, 0.0], "max_packed_vs_oracle": [0.0, 0.0]}
    default = eng.config.exact_order
    try:
        for t, trial in enumerate(c.trials):
            ospec, spec = pf.resolve_inter(c, trial["spec"], (c.seed, t))
            want = pf.oracle_frame(c, ospec)
            cols = [k for k in want.columns if k not in ("geoid", "time")]
            for exact in [default] + ([not default] if c.other_knob else []):
                eng.config.exact_order = exact
                rec["trials"] += 1
                msg = repr((seed, t, exact, pf._plain(trial["spec"])))
                eng._PLAN_CACHE.clear()
                got_f = af.aggregate_dataset(dataset=plain, weights=weights["plain"], **spec)
                descs_f = [p.describe() for p in eng._PLAN_CACHE.values()]
                assert descs_f and all("storage=" not in d for d in descs_f) and all(d.startswith("variant=f32_") for d in _on_cube(descs_f, T)), (descs_f, msg)
                eng._PLAN_CACHE.clear()
                del materialised[:]
                try:
                    got_p = af.aggregate_dataset(dataset=packed, weights=weights["packed"], **spec)
                except (hip.HipUnsupported, ValueError) as e:
                    # refused on the packed cube (and accepted on the plain one, above): by its error text only
                    assert str(e).strip() and re.search(r"packed|unsupported|not supported|no .*kernel|cannot|int16|uint16", str(e), re.I), (str(e), msg)
                    rec["refusals"].append({"trial": t, "exact_order": exact, "error": f"{type(e).__name__}: {e}"[:300]})
                    got_p = None
                descs = [p.describe() for p in eng._PLAN_CACHE.values()]
                for key, got in (("plain", got_f), ("packed", got_p)):
                    if got is None:
                        continue
                    assert list(got.columns) == list(want.columns), (key, list(got.columns), list(want.columns), msg)
                    assert len(got) == len(want), (key, len(got), len(want), msg)
                    assert (got["geoid"].values == want["geoid"].values).all() and _labels_equal(c, got, want), (key, msg)
                    assert got[cols].shape == want[cols].shape, (key, msg)
                w = want[cols].values.astype(float)
                f = got_f[cols].values.astype(float)
                np.testing.assert_allclose(f, w, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg="plain against the oracle: " + msg)
                if got_p is None:
                    continue
                p = got_p[cols].values.astype(float)
                for k, other in (("max_packed_vs_plain", f), ("max_packed_vs_oracle", w)):
                    rec[k] = [max(x, y) for x, y in zip(rec[k], _max_diff(p, other))]
                np.testing.assert_allclose(p, w, rtol=RTOL, atol=ATOL, equal_nan=True,
                                           err_msg="packed against the oracle (plain agrees with it: the packed menu or the rules): " + msg)
                np.testing.assert_allclose(p, f, rtol=RTOL, atol=ATOL, equal_nan=True, err_msg="packed against plain: " + msg)
                # the plans of the packed run: those on the cube's time axis read the stored integers
                assert not materialised, "the packed cube was materialised on the public route: " + msg
                on_cube = _on_cube(descs, T)
                assert on_cube and all(f"storage={c.storage}" in d and d.startswith("variant=i16_") for d in on_cube), (descs, msg)
                assert all("storage=" in d or int(re.search(r"\bT=(\d+)", d).group(1)) < T for d in descs), (descs, msg)
                rec["variants"] += [v for v in _variants(on_cube) if v not in rec["variants"]]
                rec["routes"] += [r for d in on_cube for r in re.findall(r"last-run=\S+", d) if r not in rec["routes"]]
                if trial["expect"] == "no-hist":
                    assert not any("_hist" in v for v in _variants(on_cube)), (descs, msg)
                if exact == default and (c.stratum != "wide" or trial["kind"] == "wide"):
                    rec["reached"] = rec["reached"] or _family_reached(c.stratum, on_cube)
    finally:
        eng.config.exact_order = default
        eng._PLAN_CACHE.clear()
    return rec


@pytest.mark.parametrize("seed", pf.SEEDS)
def test_random_specs_on_packed_cubes_match_oracle(torch_cuda, tmp_path, monkeypatch, seed):
    rec = _run_seed(seed, tmp_path, monkeypatch)
    _RESULTS[seed] = rec
    assert rec["reached"], f"no trial of seed {seed} reached the kernels of its stratum ({rec['stratum']}): {rec['variants']} {rec['routes']}"


def test_census_over_the_seed_list(torch_cuda, tmp_path, monkeypatch):
    """Over the whole seed list (seeds that have not run in this process run here): one, two and four cells per lane, both storages,
    every family, and refusals on fewer than one trial in ten."""
    for seed in pf.SEEDS:
        if seed not in _RESULTS:
            d = tmp_path / f"s{seed}"
            d.mkdir()
            _RESULTS[seed] = _run_seed(seed, d, monkeypatch)
    recs = [_RESULTS[s] for s in pf.SEEDS]
    out = _report_dir()
    if out is not None:
        with open(os.path.join(out, "packed_fuzz_census.json"), "w") as fh:
            json.dump({"bars": {"rtol": RTOL, "atol": ATOL}, "seeds": {str(s): _RESULTS[s] for s in pf.SEEDS}}, fh, indent=1)
    names = [v for r in recs for v in r["variants"]]
    assert {m for v in names for m in re.findall(r"_v(\d)_", v)} == {"1", "2", "4"}, sorted(set(names))
    assert {r["storage"] for r in recs} == {"int16", "uint16"}
    assert all(r["reached"] for r in recs), [s for s in pf.SEEDS if not _RESULTS[s]["reached"]]
    assert any("_pair" in v for v in names) and any("_cmap" in v for v in names) and any(v.endswith("_hist") or "_hist_arith" in v for v in names)
    assert any("_ends" in v and "_cmap" not in v for v in names) and any("last-run=region-fused" in x for r in recs for x in r["routes"])
    refused, trials = sum(len(r["refusals"]) for r in recs), sum(r["trials"] for r in recs)
    assert refused * 10 <= trials, (refused, trials, [x for r in recs for x in r["refusals"]])
