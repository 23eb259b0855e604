"""What the generator of the packed-cube fuzz (tests/packed_fuzz.py) promises, checked without a GPU — so that
tests/test_gpu_packed_fuzz.py cannot pass by drawing nothing interesting: determinism, the census of rule-boundary positions,
storages, fills, pair counts, row lengths and strata over the seed list, what every seed's cube holds, the generator's own
consistency (multi-rule host values are the parts' values), and that the oracle's frame of every seed's first trial is no empty
statement."""
import functools

import numpy as np
import pytest

import packed_fuzz as pf


@functools.lru_cache(maxsize=None)
def _case(seed):
    return pf.case(seed)


def test_case_is_deterministic():
    for seed in (1, 10, 17, 26, 103):
        a, b = pf.case(seed), pf.case(seed)
        assert a.digest() == b.digest()
        assert a.bits.tobytes() == b.bits.tobytes() and a.host.tobytes() == b.host.tobytes()
        assert repr(pf._plain(a.trials)) == repr(pf._plain(b.trials))
    assert pf.case(1).digest() != pf.case(3).digest()


def test_census_over_the_seed_list():
    cases = [_case(s) for s in pf.SEEDS]
    assert len(pf.SMALL_SEEDS) == 36 and len(pf.RF_SEEDS) == 8
    seen = set().union(*(c.boundary_classes() for c in cases))
    assert seen == set(pf.BOUNDARY_CLASSES), set(pf.BOUNDARY_CLASSES) - seen
    assert {c.storage for c in cases} == {"int16", "uint16"}
    assert all(c.storage == ("uint16" if c.seed % 2 else "int16") for c in cases)
    fills = {(c.storage, f) for c in cases for _, _, f in c.rules}
    assert fills == {("int16", None), ("int16", -32767), ("int16", -32768), ("uint16", None), ("uint16", 65535), ("uint16", 0)}, fills
    assert {n for c in cases for n in c.n_pairs} == {1, 2, 3}
    assert {len(c.rules) for c in cases} == {1, 2, 3, 4}
    assert {c.build for c in cases} == {"concat", "rules", "zarr"}
    assert 0.2 <= sum(c.build == "zarr" for c in cases) / len(cases) <= 0.3
    small = [c for c in cases if c.stratum != "region-fused"]
    assert {(len(c.lat) * len(c.lon)) % 4 for c in small} == {0, 1, 2, 3}
    for res, wg in ((0, 1024), (2, 512), (1, 256), (3, 256)):             # below and above one 256-thread workgroup's cells
        cells = [len(c.lat) * len(c.lon) for c in small if (len(c.lat) * len(c.lon)) % 4 == res]
        assert min(cells) < wg < max(cells), (res, cells)
    by = {}
    for c in cases:
        by.setdefault(c.stratum, []).append(c.seed)
    assert set(by) == set(pf.SMALL_STRATA) | {"region-fused"} and all(len(v) >= 3 for v in by.values()), by
    assert sum(c.other_knob for c in cases) == len(cases) // 4
    assert all(4 <= len(c.trials) <= 7 for c in cases)
    # the strata's own draws
    short = [c for c in cases if c.stratum == "short"]
    lens = [set(np.diff(pf.group_bounds(c.otime)[0]).tolist()) for c in short]
    assert {2} in lens and {3} in lens and {4} in lens and any(len(x) > 1 and max(x) <= 4 and min(x) >= 1 for x in lens), lens
    for name in ("hist-equal", "hist-ends", "hist-cellmap"):
        kinds = [t["expect"] for c in cases if c.stratum == name for t in c.trials if t["kind"] == name]
        assert {"hist-equal": "hist", "hist-ends": "ends", "hist-cellmap": "cmap"}[name] in kinds
    assert all(any(t["expect"] == "no-hist" for t in c.trials) for c in cases if c.stratum == "hist-cellmap")
    from aggfly_amd import engine as eng
    for c in cases:
        if c.stratum == "wide":
            assert any(sum(len(eng.lower_spec(k, st)[0]) for k, st in t["spec"].items()) > 16 for t in c.trials)
        if c.stratum == "region-fused":
            assert c.bits.shape[1:] == (48, 80) and 12 <= c.tab.index_right.nunique() <= 13
    assert any(c.tab.groupby("cell_id").size().max() >= 3 for c in cases if c.stratum == "region-fused")


@pytest.mark.parametrize("seed", pf.SEEDS)
def test_what_a_seeds_cube_holds(seed):
    c = _case(seed)
    lo, hi = c.window
    T = hi - lo
    assert c.host.dtype == np.float32 and c.host.shape == (T,) + c.bits.shape[1:] and len(c.time) == len(c.otime) == T
    stored = c.bits[lo:hi].view(np.uint16) if c.unsigned else c.bits[lo:hi]
    have = set(np.unique(stored).tolist())
    assert set(pf.RANGE[c.storage]) <= have
    wb = c.window_bounds
    fills = [(f, a, b) for (_, _, f), a, b in zip(c.rules, wb[:-1], wb[1:]) if f is not None and b > a]
    assert fills and all((stored[a:b] == f).any() for f, a, b in fills)
    # NaN exactly at a rule's own fill
    want_nan = np.zeros(c.host.shape, bool)
    for (_, _, f), a, b in zip(c.rules, wb[:-1], wb[1:]):
        if f is not None:
            want_nan[a:b] = stored[a:b] == f
    assert np.array_equal(np.isnan(c.host), want_nan) and want_nan.any() and not want_nan.all()
    # a snapped threshold that is a host value, bit for bit
    assert c.snapped
    flat = c.host.reshape(-1)
    assert any((flat == np.float32(v)).any() and float(np.float32(v)) == v for v, _, _ in c.snapped)
    used = {float(x) for t in c.trials for st in t["spec"].values() for k, p in st if k == "aggregate" and "ddargs" in p
            for x in np.asarray(p["ddargs"], dtype=float).reshape(-1, 3)[:, :2].ravel()}
    assert any(v in used and (flat == np.float32(v)).any() for v, _, _ in c.snapped)
    # some date group is all fill for some cell that is not all fill
    ib, _ = pf.group_bounds(c.otime)
    h2 = np.isnan(c.host.reshape(T, -1))
    ocean = h2.all(axis=0)
    assert any((h2[a:b].all(axis=0) & ~ocean).any() for a, b in zip(ib[:-1], ib[1:]))
    assert np.isnan(c.host[wb[0]:, :, :].reshape(T, -1)[:, -1]).any()                   # the last cell holds fills
    # values are temperatures in the cube's unit: continuous across the rule changes (a tenth of a kelvin is the coarsest packing)
    med = np.nanmedian(c.host.reshape(T, -1), axis=1)
    assert abs(np.nanmedian(med) - pf.to_unit(15.0, c.preprocess)) < 25 * pf.unit_step(c.preprocess)
    for k, b in enumerate(wb[1:-1], 1):             # (rules of a few rows hold mostly planted values: left out)
        if wb[k] - wb[k - 1] >= 8 and wb[k + 1] - wb[k] >= 8:
            assert abs(med[b] - med[b - 1]) < 12 * pf.unit_step(c.preprocess), (b, med[b - 2:b + 2])


@pytest.mark.parametrize("seed", pf.SEEDS[::3])
def test_multi_rule_host_values_are_the_parts_values(seed):
    c = _case(seed)
    lo, hi = c.window
    full = pf.host_values(c.bits, c.rule_pairs, [f for _, _, f in c.rules], c.bounds, c.unsigned)
    assert np.array_equal(full[lo:hi].view(np.uint32), c.host.view(np.uint32))
    for (s, o, f), pairs, a, b in zip(c.rules, c.rule_pairs, c.bounds[:-1], c.bounds[1:]):
        part = pf.np_unpack(c.bits[a:b], pairs, f, c.unsigned)
        assert np.array_equal(part.view(np.uint32), full[a:b].view(np.uint32))
        # ... and the chain is the packing followed by the preprocess, one rounded float32 operation at a time
        w = (c.bits[a:b].view(np.uint16) if c.unsigned else c.bits[a:b]).astype(np.float32)
        w = w * np.float32(s)
        if o is not None:
            w = w + np.float32(o)
        if c.preprocess != "none":
            w = w - np.float32(273.15)
        if c.preprocess == "fahrenheit":
            w = w * np.float32(1.8)
            w = w + np.float32(32)
        ok = ~np.isnan(part)
        assert np.array_equal(w[ok], part[ok])


@pytest.mark.parametrize("seed", pf.SEEDS)
def test_the_oracle_alone_says_something_on_the_first_trial(seed):
    c = _case(seed)
    ospec, _ = pf.resolve_inter(c, c.trials[0]["spec"], (c.seed, 0))
    want = pf.oracle_frame(c, ospec)
    cols = [k for k in want.columns if k not in ("geoid", "time")]
    vals = want[cols].values.astype(float)
    assert vals.size and np.isnan(vals).mean() < 0.5, np.isnan(vals).mean()
    assert any(len(np.unique(v[np.isfinite(v)])) > 1 for v in vals.T)
