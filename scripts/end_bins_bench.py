#!/usr/bin/env python3
"""Bins with open end bins on the LDS-histogram kernels with FEAT_END_BINS (gen_variants.py: end_bins_menu) against the route such a
plan took before, on the configs[1] shape (T = 8760 x 309,600 cells), in ONE process.

The plan: thirteen 5-degree bins from -20 to 45 C between two open ends, (-inf, -20) and (45, inf) — fifteen slots — single level
(one period, every column a count) and two-level with a mean column (daily groups, one yearly period).  The cube: `packed_bench`'s
ERA5-like field as int16 storage, its float32 unpacking and that as float64.  Per storage and plan three kernels, each on a fresh plan
(the knobs are read when a plan is created), timed with HIP-event pairs around the temporal kernel (`afhip_plan_profile_*`;
`--launches` back to back after `--warmup`; min / median / max):

    ends     the end-bin histogram kernel, the planner's own choice
    earlier  the same plan under AFHIP_NO_END_BINS_HIST=1: the sixteen-slot integer-bin form (float) / the general packed kernel
    closed   the thirteen closed bins alone on their histogram kernel: the floor, and what the extra predicate costs against it

The decision rule, per storage (the one the packed histogram forms were held to): the end-bin route is the default where its MEDIAN
is below the earlier route's MINIMUM in this process, on both plans; the last lines say which storages meet it.

    python scripts/end_bins_bench.py [--out FILE]

`profiles/end_bins.txt` holds this script's output as its section 2, pasted whole; its section 1 — the new kernels' resource lines and the
comparison of the existing kernels' with the parent's — comes from the compiler's remarks on the build machine
(`make -Otarget EXTRA=-Rpass-analysis=kernel-resource-usage` in aggfly_amd/csrc), not from this script.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import hip, synth  # noqa: E402
from packed_bench import stats, stored_cube  # noqa: E402

INF = float("inf")


def columns(ends, single, mean):
    e = [float(x) for x in np.arange(-20, 50, 5.0)]
    bins = list(zip(e[:-1], e[1:]))
    if ends:
        bins = [(-INF, e[0])] + bins + [(e[-1], INF)]
    outer = {} if single else dict(outer="sum")
    return [dict(inner="bins", inner_args=(t0, t1, 0), **outer) for t0, t1 in bins] + ([dict(inner="mean", **outer)] if mean else [])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--ny", type=int, default=215)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--spd", type=int, default=24)
    ap.add_argument("--regions", type=int, default=3100)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--storages", default="packed,float32,float64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    C = a.ny * a.nx
    packed = af.PackedCube(stored_cube(a.T, a.ny, a.nx, a.spd), scale_factor=0.0017, add_offset=281.3, fill_value=-32767) - 273.15
    say(f"cube T={a.T} x {a.ny} x {a.nx} = {C} cells; device {hip.device_info(hip._device_index(packed.q))['name']}; build {hip.build_info()}")
    wdf = synth.weights_table(a.ny, a.nx, a.regions, seed=7)
    R = int(wdf["index_right"].max()) + 1
    csr = hip.CSR(wdf["index_right"].to_numpy(), wdf["cell_id"].to_numpy(), wdf["weight"].to_numpy(), R, C)
    ib0 = synth.hourly_bounds(a.T, a.spd)
    verdict = {}
    for storage in a.storages.split(","):
        if storage == "packed":
            cube, code = packed, hip._dtype_code(packed)
        else:
            cube = packed.materialize()
            if storage == "float64":
                cube = cube.double()
            code = hip.F64 if storage == "float64" else hip.F32
        wins = []
        for single in (True, False):
            title = "single level" if single else "two-level with a mean (daily groups, one period)"
            ib, ob = (np.array([0, a.T]), np.array([0, 1])) if single else (ib0, np.array([0, len(ib0) - 1]))
            say()
            say(f"{storage}, thirteen 5-degree bins + two open ends, {title}")
            ms_of, res = {}, {}
            for route, ends, env in (("ends", True, {}), ("earlier", True, {"AFHIP_NO_END_BINS_HIST": "1"}), ("closed", False, {})):
                cols = columns(ends, single, mean=not single)
                os.environ.update(env)
                p = hip.FusedPlan(a.T, C, code, ib, ob, cols)
                for k in env:
                    del os.environ[k]
                if storage == "packed":
                    p.bind_packing(cube)
                out = p.run(cube, csr)
                for _ in range(a.warmup):
                    p.run(cube, csr, out=out)
                torch.cuda.synchronize()
                p.profile_begin(a.launches)
                for _ in range(a.launches):
                    p.run(cube, csr, out=out)
                torch.cuda.synchronize()
                ms_of[route], res[route] = p.profile_end(), out["res"].cpu().numpy()
                say(f"  {route:8s} {p.describe().split()[0]:60s} {stats(ms_of[route])}")
            with np.errstate(invalid="ignore", divide="ignore"):
                d = np.nanmax(np.abs(res["ends"] - res["earlier"]) / np.maximum(np.abs(res["earlier"]), 1e-300))
            med = {k: float(np.median(v)) for k, v in ms_of.items()}
            wins.append(med["ends"] < min(ms_of["earlier"]))
            say(f"  ends median / earlier minimum: {med['ends'] / min(ms_of['earlier']):.3f}   ends / closed (medians): {med['ends'] / med['closed']:.3f}"
                f"   panels of ends and earlier differ by at most {d:.1e} relative")
        verdict[storage] = all(wins)
        del cube
    say()
    for storage, ok in verdict.items():
        say(f"decision rule, {storage}: the end-bin route's median is {'below' if ok else 'NOT below'} the earlier route's minimum on both plans"
            f" -> {'the default' if ok else 'NOT the default by the rule'}")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
