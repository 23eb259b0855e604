"""``aggfly run`` as a one-rank-per-GPU job: how many ranks a command asks for (`plan_ranks`), and how they are started
(`launch`).  Host only: nothing here imports torch or touches a GPU.

The reference's knob for parallelism is ``execution.n_workers`` / ``--n-workers`` (`aggfly/cli/main.py:180-239`), a dask
worker count.  Here a worker is a rank with a GPU of its own: the parent starts ``python -m torch.distributed.run`` as a
CHILD process with the original command line (never an exec), waits for it and returns its exit code; the ranks find
``WORLD_SIZE`` in their environment, join the process group (`main._maybe_init_distributed`) and share the years or the
store between them (`pipeline.run_pipeline`).  The parent allocates nothing and writes nothing.
"""
from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

HOST_THREADS = 16       # host threads a job may count on; the ranks share them (never sized from os.cpu_count())
REHEARSAL_ENV = "AGGFLY_DIST_BACKEND"
DRY_ENV = "AGGFLY_CLI_DRY_LAUNCH"


class LaunchRefused(Exception):
    """The command asks for more ranks than there are GPUs."""


def parse_gpus(value):
    """``--gpus``: None | "all" | an int >= 1.  ValueError for anything else."""
    if value is None:
        return None
    if isinstance(value, str) and value.strip().lower() == "all":
        return "all"
    try:
        n = int(value)
    except (TypeError, ValueError):
        raise ValueError(f"{value!r} is neither a positive integer nor 'all'") from None
    if n < 1:
        raise ValueError(f"{n} is not a positive rank count")
    return n


def _rehearsal(env) -> bool:
    """Ranks may share a card only in the labelled gloo rehearsal (as in bench.py)."""
    return env.get(REHEARSAL_ENV) == "gloo"


def needs_gpu_count(config, gpus_opt, env) -> bool:
    """Does `plan_ranks` need the number of visible GPUs for this command?  The plain command never counts devices."""
    if "WORLD_SIZE" in env:
        return False
    if gpus_opt == "all":
        return True
    if _rehearsal(env):
        return False
    return gpus_opt is not None or config.n_workers > 1


def plan_ranks(config, gpus_opt, env, visible_gpus, n_paths):
    """-> (n_ranks, why).  First match wins:

    1. ``WORLD_SIZE`` in ``env``: this process IS a rank and never launches again;
    2. ``--gpus N | all``: strict; more ranks than visible GPUs raises `LaunchRefused` outside the gloo rehearsal;
    3. ``config.n_workers`` (a wish written for dask): clamped to the visible GPUs, unclamped in the rehearsal;
    4. a ``{year}``-templated config: clamped further to its paths, since a rank without a year has nothing to do (the
       single-store route takes any number: its periods or latitude bands are dealt out inside the store);
    5. 1 = one process, no child, no process group.
    """
    if "WORLD_SIZE" in env:
        return 1, "under a launcher"
    if gpus_opt is not None:
        if gpus_opt == "all":
            return max(1, int(visible_gpus)), f"--gpus all: {visible_gpus} GPU(s) visible"
        n = int(gpus_opt)
        if n > visible_gpus and not _rehearsal(env):
            raise LaunchRefused(f"--gpus {n} but only {visible_gpus} GPU(s) visible; one GPU per rank, "
                                f"or set {REHEARSAL_ENV}=gloo to rehearse")
        return n, f"--gpus {n}"
    n = max(1, int(config.n_workers))
    why = f"execution.n_workers = {config.n_workers}"
    if not _rehearsal(env) and n > max(1, visible_gpus):
        n = max(1, visible_gpus)
        why += f", {visible_gpus} GPU(s) visible"
    if config.templated and n > max(1, n_paths):
        n = max(1, n_paths)
        why += f", {n_paths} path(s)"
    return n, why


def child_command(n, argv, port):
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
            "--master-addr", "127.0.0.1", "--master-port", str(port), "-m", "aggfly_amd.cli.main", *argv]


def child_env(n, config, env):
    """The parent's environment; OMP_NUM_THREADS only when the caller left it unset: ``execution.threads_per_worker``
    when the config gives more than 1, else an even share of the host's threads."""
    out = dict(env)
    if "OMP_NUM_THREADS" not in out:
        tpw = int(getattr(config, "threads_per_worker", 1) or 1)
        out["OMP_NUM_THREADS"] = str(tpw if tpw > 1 else max(1, HOST_THREADS // n))
    return out


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch(n, argv, config=None) -> int:
    """Start the ``n`` ranks as a child ``torch.distributed.run``, pass its output through, -> its exit code.
    ``AGGFLY_CLI_DRY_LAUNCH=1`` prints the child command as one JSON object and starts nothing."""
    cmd = child_command(n, argv, _free_port())
    if os.environ.get(DRY_ENV):
        print(json.dumps({"launch": cmd}), flush=True)
        return 0
    proc = subprocess.Popen(cmd, env=child_env(n, config, os.environ))      # stdout / stderr inherited
    try:
        return proc.wait()
    except KeyboardInterrupt:       # SIGTERM, not SIGKILL: the launcher takes its ranks down with it
        proc.terminate()
        try:
            proc.wait(timeout=30)
        except subprocess.TimeoutExpired:
            proc.kill()
            proc.wait()
        return proc.returncode or 130
