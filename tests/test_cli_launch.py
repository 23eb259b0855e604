"""`aggfly run` as a one-rank-per-GPU job, host side: the rank plan (`cli.launch.plan_ranks`) as a table, the child command
(dry launch), no GPU code in the parent before the launch, the OMP_NUM_THREADS rule, and the help text."""
import json
import os
import subprocess
import sys

import pytest
import yaml
from click.testing import CliRunner

from aggfly_amd.cli import config as cfg, launch
from aggfly_amd.cli.main import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFUSAL = "--gpus 4 but only 2 GPU(s) visible; one GPU per rank, or set AGGFLY_DIST_BACKEND=gloo to rehearse"


def _raw(path="d.zarr", years=None, **execution):
    raw = {"regions": {"path": "r.csv", "regionid": "geoid"},
           "dataset": {"path": path, "var": "t2m"},
           "aggregate": {"variables": {"tavg": [["aggregate", {"calc": "mean", "groupby": "date"}],
                                                ["aggregate", {"calc": "sum", "groupby": "year"}]]}},
           "output": {"path": "out.csv"}}
    if years is not None:
        raw["years"] = years
    if execution:
        raw["execution"] = execution
    return raw


def _plan(raw, gpus=None, env=None, visible=1):
    c = cfg.parse_config(raw)
    return launch.plan_ranks(c, launch.parse_gpus(gpus), env or {}, visible, len(c.resolved_paths()))[0]


GLOO = {"AGGFLY_DIST_BACKEND": "gloo"}
YEARS3 = dict(path="era5_{year}.zarr", years="2000:2002")


@pytest.mark.parametrize("raw, gpus, env, visible, want", [
    (_raw(), None, {}, 8, 1),                                                        # defaults: today's path
    (_raw(n_workers=8), "8", {"WORLD_SIZE": "8", "RANK": "3"}, 8, 1),                # a rank never launches again
    (_raw(n_workers=8), None, {}, 1, 1),
    (_raw(n_workers=8), None, {}, 0, 1),
    (_raw(n_workers=8), None, {}, 4, 4),
    (_raw(n_workers=8, **YEARS3), None, {}, 8, 3),                                   # a rank without a year has nothing to do
    (_raw(n_workers=8), None, {}, 8, 8),                                             # single store: dealt out inside the store
    (_raw(), "all", {}, 8, 8),
    (_raw(), "all", {}, 0, 1),
    (_raw(n_workers=2), "4", {}, 4, 4),                                              # --gpus wins over n_workers
    (_raw(**YEARS3), "4", {}, 4, 4),                                                 # an explicit N is strict
    (_raw(), "4", GLOO, 2, 4),                                                       # the labelled rehearsal on fewer cards
    (_raw(n_workers=8), None, GLOO, 1, 8),
    (_raw(n_workers=8, **YEARS3), None, GLOO, 1, 3),
])
def test_plan_ranks_table(raw, gpus, env, visible, want):
    assert _plan(raw, gpus, env, visible) == want


def test_plan_ranks_refuses_more_ranks_than_gpus():
    with pytest.raises(launch.LaunchRefused) as e:
        _plan(_raw(), "4", {}, 2)
    assert str(e.value) == REFUSAL
    assert launch.plan_ranks(cfg.parse_config(_raw()), 4, {"WORLD_SIZE": "4"}, 2, 1) == (1, "under a launcher")


def test_gpu_count_is_taken_only_when_needed():
    c1, c8 = cfg.parse_config(_raw()), cfg.parse_config(_raw(n_workers=8))
    assert not launch.needs_gpu_count(c1, None, {})                                   # the plain command counts nothing
    assert launch.needs_gpu_count(c8, None, {}) and launch.needs_gpu_count(c1, 4, {}) and launch.needs_gpu_count(c1, "all", GLOO)
    assert not launch.needs_gpu_count(c8, 4, {"WORLD_SIZE": "4"})
    assert not launch.needs_gpu_count(c8, 4, GLOO)


def _write_config(tmp_path, **kw):
    cpath = tmp_path / "cfg.yaml"
    raw = _raw(**kw)
    raw["output"]["path"] = str(tmp_path / "configured.csv")
    cpath.write_text(yaml.safe_dump(raw))
    return str(cpath)


def test_gpus_option_is_checked_in_the_parent(tmp_path, monkeypatch):
    cpath = _write_config(tmp_path)
    for bad in ("0", "x", "-2"):
        r = CliRunner().invoke(cli, ["run", cpath, "--gpus", bad])
        assert r.exit_code == 2 and "--gpus" in r.output and "Usage:" in r.output, r.output
    import aggfly_amd.cli.main as main
    monkeypatch.setattr(main, "_visible_gpus", lambda: 2)
    monkeypatch.delenv("AGGFLY_DIST_BACKEND", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("AGGFLY_CLI_DRY_LAUNCH", "1")
    r = CliRunner().invoke(cli, ["run", cpath, "--gpus", "4"])
    assert r.exit_code == 1 and REFUSAL in r.output and "launch" not in r.output.replace(REFUSAL, ""), r.output
    # a config error and a bad --years exit in the parent too, with the messages they always had
    r = CliRunner().invoke(cli, ["run", str(tmp_path / "missing.yaml"), "--gpus", "2"])
    assert r.exit_code == 1 and "Config is invalid:" in r.output and "launch" not in r.output
    r = CliRunner().invoke(cli, ["run", cpath, "--gpus", "2", "--years", "19x0"])
    assert r.exit_code == 1 and "could not parse '19x0'" in r.output and '"launch"' not in r.output
    # ... and n_workers is clamped to what is visible: 8 wished, 2 there
    r = CliRunner().invoke(cli, ["run", cpath, "--n-workers", "8"])
    assert r.exit_code == 0, r.output
    assert json.loads(r.output)["launch"][4:6] == ["--nproc-per-node", "2"]


def _cli_env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "AGGFLY_DIST_BACKEND", "AGGFLY_CLI_DRY_LAUNCH")}
    env.update(PYTHONPATH=ROOT, **extra)
    return env


def test_dry_launch_prints_the_child_command(tmp_path):
    cpath = _write_config(tmp_path)
    out = str(tmp_path / "out.csv")
    argv = ["run", cpath, "--gpus", "2", "-o", out, "-v"]
    r = subprocess.run([sys.executable, "-m", "aggfly_amd.cli.main"] + argv, capture_output=True, text=True, timeout=300,
                       env=_cli_env(AGGFLY_CLI_DRY_LAUNCH="1", AGGFLY_DIST_BACKEND="gloo"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout                                                  # exactly one JSON object
    obj = json.loads(lines[0])
    assert list(obj) == ["launch"]
    cmd = obj["launch"]
    at = cmd.index("aggfly_amd.cli.main")
    assert cmd[at + 1:] == argv                                                       # the original arguments, in order
    port = cmd[cmd.index("--master-port") + 1]
    assert str(int(port)) == port and 0 < int(port) < 65536
    assert cmd == launch.child_command(2, argv, int(port))
    assert cmd[1:5] == ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node"] and cmd[5] == "2"
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "configured.csv"))
    # under a launcher the same command is a rank: it plans no launch (and then fails for want of its inputs, which is fine)
    r = subprocess.run([sys.executable, "-m", "aggfly_amd.cli.main"] + argv, capture_output=True, text=True, timeout=300,
                       env=_cli_env(AGGFLY_CLI_DRY_LAUNCH="1", AGGFLY_DIST_BACKEND="gloo", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert '"launch"' not in r.stdout and "Starting" not in r.stderr, (r.stdout, r.stderr[-500:])


def test_n_workers_in_the_config_plans_a_launch(tmp_path):
    """`execution.n_workers` alone, on a {year}-templated config: clamped to the years, and --n-workers overrides it."""
    cpath = _write_config(tmp_path, n_workers=8, threads_per_worker=2, **YEARS3)
    env = _cli_env(AGGFLY_CLI_DRY_LAUNCH="1", AGGFLY_DIST_BACKEND="gloo")
    for extra, want in (([], "3"), (["--n-workers", "2"], "2"), (["--years", "2000:2001"], "2")):
        r = subprocess.run([sys.executable, "-m", "aggfly_amd.cli.main", "run", cpath] + extra, capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        cmd = json.loads(r.stdout)["launch"]
        assert cmd[cmd.index("--nproc-per-node") + 1] == want and cmd[-2 - len(extra):] == ["run", cpath] + extra
    r = subprocess.run([sys.executable, "-m", "aggfly_amd.cli.main", "run", cpath, "--n-workers", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert '"launch"' not in r.stdout                                                 # one worker: this process does the work


def test_no_gpu_code_before_the_launch(tmp_path):
    cpath = _write_config(tmp_path)
    script = tmp_path / "probe.py"
    script.write_text(
        "import sys\n"
        "from aggfly_amd.cli.main import cli\n"
        "try:\n"
        f"    cli.main(args=['run', {cpath!r}, '--gpus', '2'], standalone_mode=False)\n"
        "except SystemExit as e:\n"
        "    assert e.code == 0, e.code\n"
        "import aggfly_amd.hip as hip\n"
        "torch = sys.modules.get('torch')\n"
        "print('PROBE', hip._lib is None, torch is None or not torch.cuda.is_initialized())\n")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300,
                       env=_cli_env(AGGFLY_CLI_DRY_LAUNCH="1", AGGFLY_DIST_BACKEND="gloo"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert '"launch"' in r.stdout and "PROBE True True" in r.stdout, r.stdout


def test_omp_threads_rule():
    c = cfg.parse_config(_raw())
    assert launch.child_env(2, c, {})["OMP_NUM_THREADS"] == "8"                      # an even share of 16 host threads
    assert launch.child_env(8, c, {})["OMP_NUM_THREADS"] == "2"
    assert launch.child_env(32, c, {})["OMP_NUM_THREADS"] == "1"
    assert launch.child_env(2, c, {"OMP_NUM_THREADS": "5", "X": "y"}) == {"OMP_NUM_THREADS": "5", "X": "y"}      # never overridden
    c4 = cfg.parse_config(_raw(threads_per_worker=4))
    assert launch.child_env(2, c4, {})["OMP_NUM_THREADS"] == "4"
    assert launch.child_env(2, c4, {"OMP_NUM_THREADS": "5"})["OMP_NUM_THREADS"] == "5"
    env = {"A": "b"}
    assert launch.child_env(2, c, env)["A"] == "b" and env == {"A": "b"}              # the parent's own environment stays as it is


def test_help_lists_gpus_and_the_reference_flags():
    r = CliRunner().invoke(cli, ["run", "--help"])
    assert r.exit_code == 0
    for flag in ("--gpus", "-o, --output", "--engine", "--years", "--project-dir", "--backend", "--n-workers", "-v, --verbose"):
        assert flag in r.output, flag
    assert "unused" not in r.output
