"""bench.py's own interface: a plain run measures the headline only, `--full` adds the rest, `--dump-outputs DIR` writes
what the last timed step computed, and `--steps` is the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
ENV = {k: v for k, v in os.environ.items() if k not in ("AGGFLY_BENCH_BACKEND", "AGGFLY_BENCH_DRY_LAUNCH", "AGGFLY_BENCH_ONLY",
                                                         "WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}


def _line(r):
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_bench_options_and_dump_sampling(tmp_path, monkeypatch):
    """The options exist, a run of no timed steps is refused before anything starts, and an output past its share of the
    dump budget is written as the same seeded sample on every run (small ones whole), float64."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--help"], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr and r.stdout.strip() == ""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 * 8 * 1000)          # two arrays: 1,000 elements each
    big = np.arange(5000, dtype=np.float32).reshape(50, 100)
    small = np.arange(12, dtype=np.float64).reshape(3, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = (np.load(tmp_path / d / "big.npy") for d in ("a", "b"))
    assert a.dtype == np.float64 and a.shape == (1000,) and np.array_equal(a, b)
    assert len(np.unique(a)) == 1000 and np.all(np.diff(a) > 0)               # distinct elements, in the array's order
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)


@pytest.mark.gpu
def test_bench_dumps_the_timed_paths_outputs(torch_cuda, tmp_path):
    """Two plain runs with the same arguments dump the same panel, which is the timed plan's own result on the seeded inputs
    and the divide of the dumped sums; the line carries exactly the requested steps and none of --full's figures, which
    --full then adds."""
    torch = torch_cuda
    T, ny, nx, regions, steps = 720, 40, 64, 30, 3
    args = ["--gpus", "1", "--steps", str(steps), "--warmup", "1", "--ny", str(ny), "--nx", str(nx), "--T", str(T), "--regions", str(regions)]
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f"run{i}"
        lines.append(_line(subprocess.run([sys.executable, BENCH] + args + ["--dump-outputs", str(d)],
                                          capture_output=True, text=True, timeout=600, env=ENV)))
        dumps.append({n: np.load(d / f"{n}.npy") for n in ("res", "num", "den")})
    for line in lines:
        assert line["steps"] == steps and line["roofline"]["launches"] == steps and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "grid-cell-timesteps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert "cpu_baseline" not in line and "other_configs" not in line and "measured_read_ceiling_GBps" not in line["roofline"]
    a, b = dumps
    R = lines[0]["config"]["regions"]
    assert a["res"].shape == (5, R, 1) and a["num"].shape == (5, R, 1) and a["den"].shape == (R, 1)
    assert all(x.dtype == np.float64 for x in a.values()) and np.isfinite(a["res"]).any()
    for n in a:
        np.testing.assert_array_equal(a[n], b[n])                            # same arguments, same inputs, same numbers
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_allclose(a["res"], np.where(a["den"] != 0, a["num"] / a["den"], np.nan), rtol=1e-12, equal_nan=True)
    # the timed path itself, in this process, on the inputs the bench seeds
    sys.path.insert(0, ROOT)
    import bench
    from aggfly_amd import hip, synth
    cube = bench.make_cube(torch, T, ny, nx, torch.float64, seed=20260101)
    tab = synth.weights_table(ny, nx, regions, seed=7)
    csr = hip.CSR(tab["index_right"].to_numpy(), tab["cell_id"].to_numpy(), tab["weight"].to_numpy(), R, ny * nx)
    ib = synth.hourly_bounds(T)
    plan = hip.FusedPlan(T, ny * nx, hip.F64, ib, np.array([0, len(ib) - 1], dtype=np.int64), bench.c2_columns())
    out = plan.run(cube, csr)
    torch.cuda.synchronize()
    np.testing.assert_allclose(out["res"].cpu().numpy(), a["res"], rtol=1e-13, atol=0, equal_nan=True)
    del cube, csr, plan, out
    torch.cuda.empty_cache()
    line = _line(subprocess.run([sys.executable, BENCH] + args + ["--full"], capture_output=True, text=True, timeout=600, env=ENV))
    assert line["steps"] == steps and "cpu_baseline" in line and "measured_read_ceiling_GBps" in line["roofline"]
