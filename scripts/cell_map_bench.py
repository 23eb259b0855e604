#!/usr/bin/env python3
"""Bins of unequal interior widths on the LDS-histogram kernels with FEAT_CELL_MAP (gen_variants.py: cell_map_menu; afhip_cell_map.h)
against the route such a plan took before, on the configs[1] shape (T = 8760 x 309,600 cells), in ONE process.

The specs:
    eight     (-inf,-10] (-10,0] (0,10] (10,20] (20,25] (25,30] (30,35] (35,inf): two interior widths, 18 cells
    fourteen  twelve interior bins of 10, 5 and 2.5 degrees from -30 to 35 C between two open ends, 52 cells
    six       (-20,-10) (-10,0) (0,7.5) (7.5,10) (10,30) (30,50), closed: the smallest plan the route takes, 32 cells
each single level (one period, every column a count) and two-level with a mean column (daily groups, one yearly period).  The cube:
`packed_bench`'s ERA5-like field as int16 storage, its float32 unpacking and that as float64.  Per storage and plan two kernels, each on
its own plan (the knobs are read when a plan is created):

    cmap     the cell-map histogram kernel, the planner's own choice
    earlier  the same plan under AFHIP_NO_CELL_MAP_HIST=1: the sixteen-slot integer-bin form (float) / the general packed kernel

timed with HIP-event pairs around the temporal kernel (`afhip_plan_profile_*`), INTERLEAVED: after `--warmup` launches of each, `--rounds`
rounds of `--launches` back-to-back launches of one and then of the other; min / median / max over all of a route's launches.

The decision rule, per storage (the planner's own, afhip_planner.cpp above choose_hist_variant): the route is the default where its MEDIAN
is below the earlier route's MINIMUM in this process on the eight- and the fourteen-bin spec, in both level forms; the six-bin spec says
whether the floor of six bins holds on that storage.  The last lines say which storages meet it.

    python scripts/cell_map_bench.py [--out FILE]

`profiles/cell_map_bins.txt` holds this script's output as its section 2, pasted whole; its section 1 — the new kernels' resource lines and
the comparison of the existing kernels' with the parent's — comes from the compiler's remarks on the build machine
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
KNOB = "AFHIP_NO_CELL_MAP_HIST"


def edges_of(e0, widths):
    return [float(x) for x in e0 + np.concatenate([[0.0], np.cumsum(widths)])]


SPECS = {
    "eight": [-INF, -10.0, 0.0, 10.0, 20.0, 25.0, 30.0, 35.0, INF],
    "fourteen": [-INF] + edges_of(-30.0, [10.0, 10.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 2.5, 2.5]) + [INF],      # -30 ... 35 C
    "six": [-20.0, -10.0, 0.0, 7.5, 10.0, 30.0, 50.0],
}
TITLES = {"eight": "eight bins, two open ends", "fourteen": "fourteen bins of three interior widths, two open ends", "six": "six closed bins"}


def columns(spec, single, mean):
    e = SPECS[spec]
    outer = {} if single else dict(outer="sum")
    return [dict(inner="bins", inner_args=(t0, t1, 0), **outer) for t0, t1 in zip(e[:-1], e[1:])] + ([dict(inner="mean", **outer)] if mean else [])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--ny", type=int, default=215)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--spd", type=int, default=24)
    ap.add_argument("--regions", type=int, default=3100)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--storages", default="packed,float32,float64")
    ap.add_argument("--specs", default="eight,fourteen,six")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    C = a.ny * a.nx
    packed = af.PackedCube(stored_cube(a.T, a.ny, a.nx, a.spd), scale_factor=0.0017, add_offset=281.3, fill_value=-32767) - 273.15
    say(f"cube T={a.T} x {a.ny} x {a.nx} = {C} cells; device {hip.device_info(hip._device_index(packed.q))['name']}; build {hip.build_info()}; "
        f"cell_map kernels {hip.menu_size('cell_map')}")
    say(f"{a.warmup} warm-up launches per route, then {a.rounds} rounds of {a.launches} launches, the routes alternating")
    wdf = synth.weights_table(a.ny, a.nx, a.regions, seed=7)
    R = int(wdf["index_right"].max()) + 1
    csr = hip.CSR(wdf["index_right"].to_numpy(), wdf["cell_id"].to_numpy(), wdf["weight"].to_numpy(), R, C)
    ib0 = synth.hourly_bounds(a.T, a.spd)
    ratio = {}
    for storage in a.storages.split(","):
        if storage == "packed":
            cube, code = packed, hip._dtype_code(packed)
        else:
            cube = packed.materialize()
            if storage == "float64":
                cube = cube.double()
            code = hip.F64 if storage == "float64" else hip.F32
        for spec in a.specs.split(","):
            for single in (True, False):
                title = "single level" if single else "two-level with a mean (daily groups, one period)"
                ib, ob = (np.array([0, a.T]), np.array([0, 1])) if single else (ib0, np.array([0, len(ib0) - 1]))
                say()
                say(f"{storage}, {TITLES[spec]}, {title}")
                cols = columns(spec, single, mean=not single)
                plans, outs, ms_of = {}, {}, {"cmap": [], "earlier": []}
                for route, env in (("cmap", {}), ("earlier", {KNOB: "1"})):
                    os.environ.update(env)
                    p = hip.FusedPlan(a.T, C, code, ib, ob, cols)
                    for k in env:
                        del os.environ[k]
                    if storage == "packed":
                        p.bind_packing(cube)
                    plans[route], outs[route] = p, p.run(cube, csr)
                    for _ in range(a.warmup):
                        p.run(cube, csr, out=outs[route])
                torch.cuda.synchronize()
                for _ in range(a.rounds):
                    for route, p in plans.items():
                        p.profile_begin(a.launches)
                        for _ in range(a.launches):
                            p.run(cube, csr, out=outs[route])
                        torch.cuda.synchronize()
                        ms_of[route] += list(p.profile_end())
                res = {k: o["res"].cpu().numpy() for k, o in outs.items()}
                for route, p in plans.items():
                    say(f"  {route:8s} {p.describe().split()[0]:60s} {stats(ms_of[route])}")
                with np.errstate(invalid="ignore", divide="ignore"):
                    d = np.nanmax(np.abs(res["cmap"] - res["earlier"]) / np.maximum(np.abs(res["earlier"]), 1e-300))
                ratio[(storage, spec, single)] = float(np.median(ms_of["cmap"])) / min(ms_of["earlier"])
                say(f"  cmap median / earlier minimum: {ratio[(storage, spec, single)]:.3f}   panels of cmap and earlier differ by at most {d:.1e} relative"
                    f"   on the route: {'_cmap' in plans['cmap'].describe().split()[0]}")
                del plans, outs
        del cube
    say()
    for storage in a.storages.split(","):
        got = {spec: [ratio.get((storage, spec, s)) for s in (True, False)] for spec in ("eight", "fourteen", "six")}
        ruled = [x for spec in ("eight", "fourteen") for x in got[spec]]
        if None in ruled:
            continue
        ok = all(x < 1.0 for x in ruled)
        say(f"decision rule, {storage}: the cell-map route's median is {'below' if ok else 'NOT below'} the earlier route's minimum on the eight- and "
            f"fourteen-bin specs in both level forms -> {'the default' if ok else 'NOT the default by the rule'}"
            + ("" if None in got["six"] else f"; six bins: {'wins too, the floor stays at six' if all(x < 1.0 for x in got['six']) else 'does NOT win: raise the floor'}"))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
