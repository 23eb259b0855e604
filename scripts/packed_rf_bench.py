#!/usr/bin/env python3
"""Packed cubes' many-period plans on the region-fused period ends (gen_variants.py: packed_rf_menu; afhip_planner.cpp: twin_of,
choose_packed_variant, choose_packed_short_variant, rf_plan_ok) against the per-cell routes such a plan took before, on the configs[1]
shape held as int16 (T = 8760 x 309,600 cells), in ONE process.

Classes of plans (`poly`: mean -> power 1 ... 4 -> sum; `dd`: degree days [10, 30] -> sum; a period is a number of inner groups):
    hourly steps (24 rows a group)     daily panel of dd + poly (K = 5) | daily dd alone | weekly poly | monthly poly (30 groups: P = 13)
    6-hourly steps (4 rows a group)    monthly poly
    8-hourly steps (3 rows a group)    daily poly
    mixed groups of one to four rows   daily poly
    (tmin, tmax) pairs (2 rows)        sine_dd [10, 30]: daily | weekly | monthly
Each class is timed two ways, each route on a plan of its own (the knobs are read when a plan is created):
    fused     the default: the region-fused route where the planner takes it (the kernel's name and `last-run=` tell)
    percell   AFHIP_NO_PACKED_RF=1: the kernel and the route the plan took before the twins — the yardstick
by the whole step (`run(timed=True)`: HIP events around the temporal kernel AND the spatial stage — the two routes differ in both),
INTERLEAVED: after `--warmup` runs of each, `--rounds` rounds of `--launches` runs of one route after the other; min / median / max
over all of a route's runs.  `--nx 1440` gives rows that are a multiple of four — `percell` then runs a FOUR-cell kernel and `fused` gives
it up for the two-cell twin —, `--nx 1442` rows that take two cells per lane on both routes, `--nx 1441` one.

The decision rule (the one the histogram routes and the short-group forms were held to), per class and row length: the class takes the
route by default only if the region-fused MEDIAN lies below the per-cell route's MINIMUM in this process.  The last lines state it per class.

    python scripts/packed_rf_bench.py [--nx 1440] [--out FILE]

`profiles/packed_region_fused.txt` holds this script's output, pasted whole, beside the twins' resource lines.
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
from packed_short_bench import inner_bounds  # noqa: E402

KNOB = "AFHIP_NO_PACKED_RF"
POLY = [dict(inner="mean", transform="pow", transform_arg=float(e), outer="sum") for e in (1, 2, 3, 4)]
DD = dict(inner="dd", inner_args=(10, 30, 0), outer="sum")
SINE = [dict(inner="sine_dd", inner_args=(10, 30, 0), outer="sum")]
# (title, rows per group or "mixed", groups per period, columns)
CLASSES = [
    ("hourly, daily panel of dd + poly", 24, 1, [DD] + POLY),
    ("hourly, daily dd alone", 24, 1, [DD]),
    ("hourly, weekly poly", 24, 7, POLY),
    ("hourly, monthly poly", 24, 30, POLY),
    ("6-hourly, monthly poly", 4, 30, POLY),
    ("8-hourly, daily poly", 3, 1, POLY),
    ("mixed one to four rows, daily poly", "mixed", 1, POLY),
    ("pairs, daily sine_dd", 2, 1, SINE),
    ("pairs, weekly sine_dd", 2, 7, SINE),
    ("pairs, monthly sine_dd", 2, 30, SINE),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--ny", type=int, default=215)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--regions", type=int, default=3100)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--classes", default=None, help="comma-separated indices into the class list (default: all)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    C = a.ny * a.nx
    packed = af.PackedCube(stored_cube(a.T, a.ny, a.nx, 24), scale_factor=0.0017, add_offset=281.3, fill_value=-32767) - 273.15
    say(f"cube T={a.T} x {a.ny} x {a.nx} = {C} cells, int16; device {hip.device_info(hip._device_index(packed.q))['name']}; build {hip.build_info()}; "
        f"packed_rf kernels {hip.menu_size('packed_rf')}")
    say(f"{a.warmup} warm-up runs per route, then {a.rounds} rounds of {a.launches} runs, the routes alternating; times are whole steps")
    wdf = synth.weights_table(a.ny, a.nx, a.regions, seed=7)
    R = int(wdf["index_right"].max()) + 1
    csr = hip.CSR(wdf["index_right"].to_numpy(), wdf["cell_id"].to_numpy(), wdf["weight"].to_numpy(), R, C)
    verdict = []
    picked = range(len(CLASSES)) if a.classes is None else [int(x) for x in a.classes.split(",")]
    for title, rows, per, cols in (CLASSES[i] for i in picked):
        ib = inner_bounds(a.T, rows)
        G1 = len(ib) - 1
        ob = np.unique(np.concatenate([np.arange(0, G1, per), [G1]])).astype(np.int64)
        P, K = len(ob) - 1, len(cols)
        say()
        say(f"{title} (K = {K}, P = {P}, period values / cube = {P * K * 8.0 / (a.T * 2.0):.4f})")
        plans, outs, ms_of = {}, {}, {}
        for route, env in (("fused", {}), ("percell", {KNOB: "1"})):
            os.environ.update(env)
            p = hip.FusedPlan(a.T, C, hip._dtype_code(packed), ib, ob, cols)
            for k in env:
                del os.environ[k]
            p.bind_packing(packed)
            plans[route], outs[route], ms_of[route] = p, p.run(packed, csr), []
            for _ in range(a.warmup):
                p.run(packed, csr, out=outs[route])
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for route, p in plans.items():
                for _ in range(a.launches):
                    ms_of[route].append(p.run(packed, csr, out=outs[route], timed=True)["kernel_ms"][1])
        res = {k: o["res"].cpu().numpy() for k, o in outs.items()}
        for route, p in plans.items():
            d = p.describe()
            last = "region-fused" if "last-run=region-fused" in d else "per-cell"
            say(f"  {route:8s} {d.split()[0]:52s} {last:13s} {stats(ms_of[route])}")
        with np.errstate(invalid="ignore", divide="ignore"):
            diff = float(np.nanmax(np.abs(res["fused"] - res["percell"]) / np.maximum(np.abs(res["percell"]), 1e-300)))
        took = "last-run=region-fused" in plans["fused"].describe()
        ratio = float(np.median(ms_of["fused"])) / min(ms_of["percell"])
        say(f"  fused median / per-cell minimum: {ratio:.3f}   took the route: {took}   panels differ by at most (relative): {diff:.1e}")
        verdict.append((title, took, ratio))
        del plans, outs
    say()
    say("decision rule: a class takes the region-fused route by default only if its median lies below the per-cell route's minimum")
    for title, took, ratio in verdict:
        if took:
            say(f"  {title}: x{ratio:.3f} of the per-cell minimum -> {'the default' if ratio < 1.0 else 'BEHIND: the rule must keep this class off the route'}")
        else:
            say(f"  {title}: the planner keeps the per-cell route (x{ratio:.3f}: the same route twice)")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
