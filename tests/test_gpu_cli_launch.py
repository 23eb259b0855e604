"""`aggfly run` starts its own ranks: the plain command with ``--gpus 2`` or ``execution: {n_workers: 2}`` — no torchrun
around it — writes what the one-process run writes, on the year route and on the single-store route; a failing rank fails
the command; and the sample year is read once per job.  The two ranks share the box's card (AGGFLY_DIST_BACKEND=gloo), as
in the rehearsals of tests/test_cli.py, whose way of writing inputs is copied here."""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import yaml

import aggfly_amd as af

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = [sys.executable, "-m", "aggfly_amd.cli.main"]
YEARS = (2000, 2001, 2002)


def _write_run_inputs(tmp_path, years=(2000,)):
    """8x8 grid, seed 7, a box region well inside it; the weights table is what area weights give for that box: whole
    cells 1, edge cells their overlap."""
    lon = np.arange(-100.0, -60.0, 5.0)
    lat = np.arange(20.0, 60.0, 5.0)
    np.random.seed(7)
    paths = []
    for y in years:
        time = pd.date_range(f"{y}-07-01", periods=4, freq="12h")
        arr = np.random.normal(20, 15, (len(time), len(lat), len(lon))) + 273.15
        ds = af.Dataset(af.DataArray(arr, ["time", "latitude", "longitude"], {"time": time, "latitude": lat, "longitude": lon}),
                        lon_is_360=False)
        p = str(tmp_path / f"ds_{y}.zarr")
        af.dataset_to_zarr(ds, p, var="t2m")
        paths.append(p)
    box = (-92.0, 28.0, -68.0, 52.0)
    regions = pd.DataFrame({"geoid": ["r1"], "minx": [box[0]], "miny": [box[1]], "maxx": [box[2]], "maxy": [box[3]]})
    rpath = str(tmp_path / "regions.csv")
    regions.to_csv(rpath, index=False)
    keep_lon = lon[(lon >= box[0] - 2.5) & (lon <= box[2] + 2.5)]
    keep_lat = lat[(lat >= box[1] - 2.5) & (lat <= box[3] + 2.5)]
    rows = []
    for iy, la in enumerate(keep_lat):
        for ix, lo in enumerate(keep_lon):
            ox = max(0.0, min(lo + 2.5, box[2]) - max(lo - 2.5, box[0])) / 5.0
            oy = max(0.0, min(la + 2.5, box[3]) - max(la - 2.5, box[1])) / 5.0
            if ox * oy > 0:
                rows.append((iy * len(keep_lon) + ix, 0, ox * oy * np.cos(np.deg2rad(la))))
    tab = pd.DataFrame(rows, columns=["cell_id", "index_right", "weight"])
    wpath = str(tmp_path / "weights.parquet")
    tab.to_parquet(wpath, index=False)
    return paths, rpath, wpath


def _run_config(dpath, rpath, wpath, out, **extra):
    c = {"regions": {"path": rpath, "regionid": "geoid"},
         "dataset": {"path": dpath, "var": "t2m", "lon_is_360": False, "preprocess": "kelvin_to_celsius"},
         "weights": {"table": wpath},
         "aggregate": {"engine": "auto", "variables": {"tavg": [["aggregate", {"calc": "mean", "groupby": "date"}],
                                                                ["transform", {"transform": "power", "exp": [1, 2]}],
                                                                ["aggregate", {"calc": "sum", "groupby": "month"}]]}},
         "output": {"path": out}}
    c.update(extra)
    return c


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "AGGFLY_CLI_DRY_LAUNCH")}
    env.update(PYTHONPATH=ROOT, AGGFLY_DIST_BACKEND="gloo", **extra)
    return env


def _cli(args, **extra):
    return subprocess.run(CLI + args, capture_output=True, text=True, timeout=300, env=_env(**extra))


class _Inputs:
    """Written once for the module; nothing below changes them."""

    def __init__(self, root):
        self.root = root
        self.paths, self.rpath, self.wpath = _write_run_inputs(root, years=YEARS)
        self.template = str(root / "ds_{year}.zarr")
        # the 300-step store of tests/test_cli.py::test_run_single_store_is_cut_inside_the_store: Nov 2001 .. Apr 2002, 6 months
        lon, lat = np.arange(-100.0, -60.0, 5.0), np.arange(20.0, 60.0, 5.0)
        time = pd.date_range("2001-11-15", periods=300, freq="12h")
        arr = np.random.default_rng(11).normal(20, 15, (len(time), len(lat), len(lon))) + 273.15
        arr[37, 3, 4] = np.nan
        self.store = str(root / "long.zarr")
        af.dataset_to_zarr(af.Dataset(af.DataArray(arr, ["time", "latitude", "longitude"], {"time": time, "latitude": lat, "longitude": lon}),
                                      lon_is_360=False), self.store, var="t2m", chunks={"time": 40, "latitude": 8, "longitude": 8})

    def config(self, name, dpath, out, **extra):
        cpath = self.root / f"{name}.yaml"
        cpath.write_text(yaml.safe_dump(_run_config(dpath, self.rpath, self.wpath, out, **extra)))
        return str(cpath)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return _Inputs(tmp_path_factory.mktemp("cli_launch"))


@pytest.fixture(scope="module")
def year_panel_one_process(inputs):
    """The one-process run of the three-year config: the panel every launch below has to reproduce."""
    out = str(inputs.root / "years_one.csv")
    r = _cli(["run", inputs.config("years_one", inputs.template, out, years="2000:2002"), "--quiet"])
    assert r.returncode == 0, r.stderr[-2000:]
    df = pd.read_csv(out)
    assert len(df) == 3
    return df


@pytest.mark.gpu
def test_gpus_flag_starts_the_ranks_year_route(torch_cuda, inputs, year_panel_one_process):
    out = str(inputs.root / "years_gpus2.csv")
    r = _cli(["run", inputs.config("years_gpus2", inputs.template, out, years="2000:2002"), "--gpus", "2"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "torch.distributed backend: gloo" in r.stderr, r.stderr[-2000:]
    assert "Wrote 3 rows" in r.stdout and r.stdout.count("Wrote") == 1, r.stdout     # rank 0 of the child writes, nobody else
    pd.testing.assert_frame_equal(pd.read_csv(out), year_panel_one_process)


@pytest.mark.gpu
def test_n_workers_in_the_config_starts_the_ranks(torch_cuda, inputs, year_panel_one_process):
    out = str(inputs.root / "years_workers2.csv")
    cpath = inputs.config("years_workers2", inputs.template, out, years="2000:2002", execution={"n_workers": 2})
    r = _cli(["run", cpath])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "torch.distributed backend: gloo" in r.stderr and "2 local rank(s)" in r.stderr, r.stderr[-2000:]
    pd.testing.assert_frame_equal(pd.read_csv(out), year_panel_one_process)


@pytest.mark.gpu
def test_gpus_flag_single_store_route(torch_cuda, inputs):
    panels = {}
    for tag, flags in (("one", []), ("gpus2", ["--gpus", "2"])):
        out = str(inputs.root / f"store_{tag}.csv")
        r = _cli(["run", inputs.config(f"store_{tag}", inputs.store, out), "-v"] + flags)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "streamed through HBM in windows" in r.stdout, r.stdout
        assert (f"split over {2 if flags else 1} rank(s)") in r.stdout, r.stdout
        panels[tag] = pd.read_csv(out, parse_dates=["time"])
    one, two = panels["one"], panels["gpus2"]
    assert len(one) == 6 and list(two.columns) == list(one.columns)
    assert two["geoid"].tolist() == one["geoid"].tolist() and two["time"].tolist() == one["time"].tolist()
    np.testing.assert_allclose(two[["tavg_1", "tavg_2"]].values, one[["tavg_1", "tavg_2"]].values, rtol=1e-13)


@pytest.mark.gpu
def test_a_failing_rank_fails_the_command(torch_cuda, inputs):
    out = str(inputs.root / "never.csv")
    cpath = inputs.config("missing", str(inputs.root / "absent_{year}.zarr"), out, years="2000:2002")
    r = _cli(["run", cpath, "--gpus", "2"])                                           # (timeout=300: the parent does not hang)
    assert r.returncode != 0, r.stdout
    assert not os.path.exists(out)


SPY = '''\
"""preprocess_from module of the test: counts, per rank, the chunks of year 2000's data variable that the rank locates on
disk (every read route of a Zarr array asks `chunk_locator`) and hands to the native decoders."""
import os
from aggfly_amd import codec, io as afio

MARK = os.path.join("ds_2000.zarr", "t2m")
OUT = os.path.join(os.environ["AGGFLY_TEST_SPY_DIR"], "rank%s.txt" % os.environ.get("RANK", "0"))

if not hasattr(codec, "_year0_counts"):
    codec._year0_counts = counts = {"located": 0, "decoded": 0}

    def _note(key, n):
        counts[key] += n
        with open(OUT, "w") as f:
            f.write("%d %d" % (counts["located"], counts["decoded"]))

    def _hits(locators):
        return sum(1 for loc in locators if loc is not None and MARK in loc[0])

    real_ranges, real_packed, real_locator = codec.decode_ranges, codec.read_packed, afio.ZarrArray.chunk_locator
    codec.decode_ranges = lambda kind, locators, *a, **k: _note("decoded", _hits(locators)) or real_ranges(kind, locators, *a, **k)
    codec.read_packed = lambda locators, *a, **k: _note("decoded", _hits(locators)) or real_packed(locators, *a, **k)

    def chunk_locator(self, *a, **k):
        _note("located", int(MARK in self.path))
        return real_locator(self, *a, **k)
    afio.ZarrArray.chunk_locator = chunk_locator
    _note("located", 0)


def clean(x):
    return x - 273.15
'''


@pytest.mark.gpu
def test_sample_year_is_read_by_its_owner_only(torch_cuda, inputs, year_panel_one_process):
    spy_dir = inputs.root / "spy"
    spy_dir.mkdir()
    mod = inputs.root / "spy_prep.py"
    mod.write_text(SPY)
    out = str(inputs.root / "years_spy.csv")
    raw = _run_config(inputs.template, inputs.rpath, inputs.wpath, out, years="2000:2002")
    del raw["dataset"]["preprocess"]
    raw["dataset"]["preprocess_from"] = f"{mod}:clean"
    cpath = inputs.root / "years_spy.yaml"
    cpath.write_text(yaml.safe_dump(raw))
    r = _cli(["run", str(cpath), "--gpus", "2"], AGGFLY_TEST_SPY_DIR=str(spy_dir))
    assert r.returncode == 0, r.stderr[-2000:]
    pd.testing.assert_frame_equal(pd.read_csv(out), year_panel_one_process)
    seen = {rank: tuple(int(v) for v in (spy_dir / f"rank{rank}.txt").read_text().split()) for rank in (0, 1)}
    assert seen[0][0] > 0 and seen[0][1] > 0, seen          # rank 0 owns year 2000 (and 2002): it read the sample, the spy sees reads
    assert seen[1] == (0, 0), seen                          # rank 1 owns 2001: the grid of year 2000, none of its chunks
