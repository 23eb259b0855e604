#!/usr/bin/env python3
"""Packed cubes' short-group plans on the lean short-group kernels (gen_variants.py: packed_short_menu; afhip_planner.cpp:
choose_packed_short_variant) against the general packed kernel such a plan took before, on the configs[1] shape held as int16
(T = 8760 x 309,600 cells; 8760 divides by 2, 3 and 4), in ONE process.

Per group length — 2, 3, 4 rows, and mixed one to four (the cycle 4 1 3 4 2 4 4 1 3 2 4 3) — four plans, each with one yearly period:
    light     one column: mean -> sum                                        (the stat-1 two-column kernels)
    heavy     K = 5: mean -> power 1 ... 5 -> sum                            (stat 1, six columns)
    minmax    two columns: min -> sum, max -> sum                            (stat 2, two columns)
    extremes  K = 4: min -> sum, max -> sum, mean -> sum, max -> power 2 -> sum    (stat 2, six columns)
and for two-row groups (tmin, tmax pairs) also
    sine      two columns: sine_dd[10, 30] -> sum and sine_dd[5, 18] -> sum   (the sine-only kernel)
Each plan is timed five ways, every route on a plan of its own (the knobs are read when a plan is created):
    short4   the lean short-group kernel at four cells per lane (AFHIP_PACKED_SHORT_VEC=4)
    short2   ... at two cells per lane (AFHIP_PACKED_SHORT_VEC=2)
    short1   ... at one cell per lane (AFHIP_PACKED_SHORT_VEC=1)
             (a width the rows do not divide by, or that the library does not hold for the form, falls to the planner's own choice: the
             kernel's name tells, and the width is then left out of the rule; `--nx 1442` / `--nx 1441` give rows that take two cells / one)
    general  AFHIP_NO_PACKED_SHORT=1: the general packed kernel — the yardstick
    float32  the float32 cube of the same values (its short-group twin, or the LDS-DMA ring for a light plan): for orientation only
with HIP-event pairs around the temporal kernel (`afhip_plan_profile_*`), INTERLEAVED: after `--warmup` launches of each, `--rounds`
rounds of `--launches` back-to-back launches of one route after the other; min / median / max over all of a route's launches.

The decision rule (the one the histogram routes were held to), per class of plans — group length x light / heavy / minmax / extremes /
sine: a wider kernel enters the production menu only if its MEDIAN is below the next narrower width's MINIMUM in this process (four
against two cells; two against one), and the class takes the short-group form by default only if the median of its widest production
width is below the general packed kernel's minimum.  The last lines state both per class.

    python scripts/packed_short_bench.py [--out FILE]

`profiles/packed_short_groups.txt` holds this script's output, pasted whole, beside the new kernels' resource lines, which come from the
compiler's remarks on the build machine (`make -Otarget EXTRA=-Rpass-analysis=kernel-resource-usage` in aggfly_amd/csrc).
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

RAG = [4, 1, 3, 4, 2, 4, 4, 1, 3, 2, 4, 3]
ROUTES = (("short4", {"AFHIP_PACKED_SHORT_VEC": "4"}), ("short2", {"AFHIP_PACKED_SHORT_VEC": "2"}), ("short1", {"AFHIP_PACKED_SHORT_VEC": "1"}),
          ("general", {"AFHIP_NO_PACKED_SHORT": "1"}), ("float32", {}))


def inner_bounds(T, form):
    if form == "mixed":
        lens = []
        while sum(lens) < T:
            lens.append(min(RAG[len(lens) % len(RAG)], T - sum(lens)))
    else:
        assert T % form == 0
        lens = [form] * (T // form)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def plans_columns(form):
    out = {"light": [dict(inner="mean", outer="sum")],
           "heavy": [dict(inner="mean", transform="pow", transform_arg=float(e), outer="sum") for e in (1, 2, 3, 4, 5)],
           "minmax": [dict(inner="min", outer="sum"), dict(inner="max", outer="sum")],
           "extremes": [dict(inner="min", outer="sum"), dict(inner="max", outer="sum"), dict(inner="mean", outer="sum"),
                        dict(inner="max", transform="pow", transform_arg=2.0, outer="sum")]}
    if form == 2:
        out["sine"] = [dict(inner="sine_dd", inner_args=(10, 30, 0), outer="sum"), dict(inner="sine_dd", inner_args=(5, 18, 0), outer="sum")]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--ny", type=int, default=215)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--regions", type=int, default=3100)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--forms", default="2,3,4,mixed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    C = a.ny * a.nx
    packed = af.PackedCube(stored_cube(a.T, a.ny, a.nx, 4), scale_factor=0.0017, add_offset=281.3, fill_value=-32767) - 273.15
    values = packed.materialize()
    say(f"cube T={a.T} x {a.ny} x {a.nx} = {C} cells, int16; device {hip.device_info(hip._device_index(packed.q))['name']}; build {hip.build_info()}; "
        f"packed_short kernels {hip.menu_size('packed_short')}")
    say(f"{a.warmup} warm-up launches per route, then {a.rounds} rounds of {a.launches} launches, the routes alternating")
    wdf = synth.weights_table(a.ny, a.nx, a.regions, seed=7)
    R = int(wdf["index_right"].max()) + 1
    csr = hip.CSR(wdf["index_right"].to_numpy(), wdf["cell_id"].to_numpy(), wdf["weight"].to_numpy(), R, C)
    verdict = []
    for form in [f if f == "mixed" else int(f) for f in a.forms.split(",")]:
        ib = inner_bounds(a.T, form)
        ob = np.array([0, len(ib) - 1], dtype=np.int64)
        title = "mixed groups of one to four rows" if form == "mixed" else f"groups of {form} rows"
        for kind, cols in plans_columns(form).items():
            say()
            say(f"{title}, {kind} (K = {len(cols)})")
            plans, outs, ms_of = {}, {}, {}
            for route, env in ROUTES:
                os.environ.update(env)
                p = hip.FusedPlan(a.T, C, hip.F32 if route == "float32" else hip._dtype_code(packed), ib, ob, cols)
                for k in env:
                    del os.environ[k]
                cube = values if route == "float32" else packed
                if route != "float32":
                    p.bind_packing(packed)
                plans[route], outs[route], ms_of[route] = (p, cube), p.run(cube, csr), []
                for _ in range(a.warmup):
                    p.run(cube, csr, out=outs[route])
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for route, (p, cube) in plans.items():
                    p.profile_begin(a.launches)
                    for _ in range(a.launches):
                        p.run(cube, csr, out=outs[route])
                    torch.cuda.synchronize()
                    ms_of[route] += list(p.profile_end())
            res = {k: o["res"].cpu().numpy() for k, o in outs.items()}
            for route, (p, _) in plans.items():
                say(f"  {route:8s} {p.describe().split()[0]:52s} {stats(ms_of[route])}")
            names = {k: p.describe().split()[0] for k, (p, _) in plans.items()}
            with np.errstate(invalid="ignore", divide="ignore"):
                d = {k: float(np.nanmax(np.abs(res[k] - res["general"]) / np.maximum(np.abs(res["general"]), 1e-300))) for k in ("short4", "short2", "short1", "float32")}
            med = {k: float(np.median(v)) for k, v in ms_of.items()}
            has4, has2 = "_v4_" in names["short4"], "_v2_" in names["short2"]
            on = all("_pair" in names[k] for k in ("short4", "short2", "short1")) and "_v1_" in names["short1"] and "_pair" not in names["general"]
            w42 = med["short4"] / min(ms_of["short2"]) if has4 else float("nan")
            w21 = med["short2"] / min(ms_of["short1"]) if has2 else float("nan")
            widest = "short4" if has4 and w42 < 1.0 else ("short2" if has2 and w21 < 1.0 else "short1")
            ratio = med[widest] / min(ms_of["general"])
            say(f"  four cells' median / two cells' minimum: {w42:.3f}   two cells' median / one cell's minimum: {w21:.3f}   widest production width: {widest}"
                f"   its median / general minimum: {ratio:.3f}   its median / float32's: {med[widest] / med['float32']:.3f}   on the routes: {on}")
            say("  panels differ from the general kernel's by at most (relative): " + "  ".join(f"{k} {v:.1e}" for k, v in d.items()))
            verdict.append((title, kind, has4, has2, w42, w21, widest, ratio))
            del plans, outs
    say()
    say("decision rule: a wider kernel is production if its median is below the next narrower width's minimum; the class takes the short-group")
    say("form by default if the median of its widest production width is below the general kernel's minimum")
    for title, kind, has4, has2, w42, w21, widest, ratio in verdict:
        four = f"four cells x{w42:.3f} of two cells' minimum -> {'production' if w42 < 1.0 else 'an arm'}" if has4 else "no four-cell kernel"
        two = f"two cells x{w21:.3f} of one cell's minimum -> {'production' if w21 < 1.0 else 'an arm'}" if has2 else "no two-cell kernel"
        say(f"  {title}, {kind}: {four}; {two};"
            f" {widest} x{ratio:.3f} of the general minimum -> {'the default' if ratio < 1.0 else 'stays on the general kernel'}")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
