#!/usr/bin/env python3
"""An int16- (or uint16-) packed cube against its float32 unpacking, on the configs[1] shape (T = 8760 x 309,600 cells), in ONE process.

The stored integers are synthesised in HBM (an ERA5-like seasonal + diurnal field in steps of 0.0017 K around 281.3 K, then
- 273.15 as a second pair); the float32 cube is `PackedCube.materialize()` of them — what the default device route holds for the
same store.  Three plans: the K = 5 polynomial columns of configs[1], four degree-day thresholds, thirteen 5-degree bins.  For
each plan: the temporal kernel's ms on the packed and on the float32 cube (HIP-event pairs around the kernel,
`afhip_plan_profile_*`; `--launches` back to back after `--warmup`; min / median / max), the bare read of each cube
(`hip.read_probe`), the kernel variants, and the largest relative difference of the two panels.

``--storage uint16``: the same field as uint16 storage — every stored integer offset by 32768 into 0...65535 (the sign bit flipped),
the add_offset lowered by 32768 steps, the fill value 1 — read by the same kernels under an AFHIP_U16 plan.

Beside the single-rule cube each plan also runs with the same cube bound as 1, 40 and 480 equal-length unpack rules (`--rules`;
`afhip_plan_bind_packings` with the one rule repeated — what a record of that many stores costs the kernel, whatever the stores'
packings are: the kernel reads a rule from its table at every change and cannot know they are equal).  Each is reported against the
single-rule row of the same run; the single-rule row carries its run-to-run spread, (max - min) / median.

The bins plan is a partition of equal-width bins: the packed cube takes an LDS-histogram kernel (gen_variants.py: packed_hist_menu).  It
is also timed on a fresh plan created under AFHIP_NO_PACKED_HIST — the general packed kernel, what the plan took before the menu had
the histogram forms — and under AFHIP_PACKED_HIST_VEC=2, the two-cell kernel of the form where the library holds it (an arm of most forms:
`make MENU=arms`; else the row repeats the planner's pick): three figures beside the float32 route's, each with its kernel's name.  ``--hist-forms`` times instead every form of that menu — single-level / two-level (daily groups,
one yearly period), arithmetic edges / edge table, without / with a mean column — at two cells per lane against one (a `make MENU=arms`
library holds all sixteen kernels): the pairs behind the widths of the production menu (gen_variants.py: packed_hist_menu).

    python scripts/packed_bench.py [--storage int16|uint16] [--rules 1,40,480] [--out profiles/packed_cube_measured.txt]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import hip, synth  # noqa: E402


def plans_columns():
    edges = np.arange(-20, 50, 5.0)
    return {
        "configs[1] K=5: dd[10,30] + mean -> power[1..4] -> sum": (
            [dict(inner="dd", inner_args=(10, 30, 0), outer="sum")] +
            [dict(inner="mean", transform="pow", transform_arg=e, outer="sum") for e in (1, 2, 3, 4)], False),
        "4 degree-day thresholds -> sum": ([dict(inner="dd", inner_args=(float(t), float(t) + 10, 0), outer="sum") for t in (0, 8, 16, 24)], False),
        "13 bins of 5 degC (single level)": ([dict(inner="bins", inner_args=(edges[i], edges[i + 1], 0)) for i in range(13)], True),
    }


def hist_forms(T, ib0):
    """(title, columns, inner bounds, outer bounds) of the eight LDS-histogram forms: thirteen bins of 5 C with integer edges
    (arithmetic) or of 4.9 C from -19.85 (no float32 holds those: the edge table)."""
    out = []
    for single in (True, False):
        for arith in (True, False):
            for mean in (False, True):
                e = np.arange(-20, 50, 5.0) if arith else -19.85 + 4.9 * np.arange(14)
                outer = {} if single else dict(outer="sum")
                cols = [dict(inner="bins", inner_args=(e[i], e[i + 1], 0), **outer) for i in range(13)] + ([dict(inner="mean", **outer)] if mean else [])
                ib, ob = (np.array([0, T]), np.array([0, 1])) if single else (ib0, np.array([0, len(ib0) - 1]))
                title = f"{'single-level' if single else 'two-level'}, {'arithmetic edges' if arith else 'edge table'}{', + mean' if mean else ''}"
                out.append((title, cols, ib, ob))
    return out


def stored_cube(T, ny, nx, spd):
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.empty((T, ny, nx), dtype=torch.int16, device="cuda")
    lat = torch.linspace(0.6, 1.4, ny, device="cuda", dtype=torch.float32)[None, :, None]
    for k0 in range(0, T, 512):
        k1 = min(T, k0 + 512)
        noise = torch.randn((k1 - k0, ny, nx), generator=g, device="cuda", dtype=torch.float32)
        k = torch.arange(k0, k1, device="cuda", dtype=torch.float32)
        base = 15.0 + 12.0 * torch.sin(2 * np.pi * torch.floor(k / spd) / 365.0) + 6.0 * torch.sin(2 * np.pi * (k % spd) / spd - np.pi / 2)
        celsius = base[:, None, None] * lat + 3.0 * noise
        q[k0:k1] = torch.clamp(torch.round((celsius + 273.15 - 281.3) / 0.0017), -32766, 32767).to(torch.int16)
    return q


def stats(ms):
    return f"min {min(ms):.4f}  median {float(np.median(ms)):.4f}  max {max(ms):.4f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=8760)
    ap.add_argument("--ny", type=int, default=215)
    ap.add_argument("--nx", type=int, default=1440)
    ap.add_argument("--spd", type=int, default=24)
    ap.add_argument("--regions", type=int, default=3100)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--storage", choices=("int16", "uint16"), default="int16")
    ap.add_argument("--rules", default="1,40,480", help="rule counts the packed cube is also bound as (equal-length ranges of time steps)")
    ap.add_argument("--hist-forms", action="store_true", help="time the LDS-histogram forms at two cells per lane against one, and nothing else")
    ap.add_argument("--plan", default="", help="run only the plans whose title holds this text")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    C = a.ny * a.nx
    if a.storage == "uint16":
        q = stored_cube(a.T, a.ny, a.nx, a.spd)
        q.bitwise_xor_(-32768)                      # + 32768 modulo 2^16: the int16 tensor now holds the uint16 bits
        packed = af.PackedCube(q, scale_factor=0.0017, add_offset=281.3 - 32768 * 0.0017, fill_value=1, unsigned=True) - 273.15
    else:
        packed = af.PackedCube(stored_cube(a.T, a.ny, a.nx, a.spd), scale_factor=0.0017, add_offset=281.3, fill_value=-32767) - 273.15
    packed_code = hip._dtype_code(packed)
    plain = packed.materialize()
    say(f"cube T={a.T} x {a.ny} x {a.nx} = {C} cells: packed {packed.nbytes() / 1e9:.2f} GB ({a.storage}, pairs {packed.pairs}), "
        f"float32 {plain.numel() * 4 / 1e9:.2f} GB; device {hip.device_info(hip._device_index(plain))['name']}; build {hip.build_info()}")
    for name, cube in (("packed", packed), ("float32", plain)):
        ms = hip.read_probe(cube, launches=a.launches)[a.warmup // 2:]
        nbytes = a.T * C * (2 if name == "packed" else 4)
        say(f"bare read, {name:8s}: {stats(ms)}   ({nbytes / min(ms) / 1e9:.2f} TB/s at the minimum)")
    wdf = synth.weights_table(a.ny, a.nx, a.regions, seed=7)
    R = int(wdf["index_right"].max()) + 1
    csr = hip.CSR(wdf["index_right"].to_numpy(), wdf["cell_id"].to_numpy(), wdf["weight"].to_numpy(), R, C)
    ib0 = synth.hourly_bounds(a.T, a.spd)
    for title, cols, ib, ob in (hist_forms(a.T, ib0) if a.hist_forms else []):
        say()
        say(title)
        med = {}
        for vec in (2, 1):
            os.environ["AFHIP_PACKED_HIST_VEC"] = str(vec)
            p = hip.FusedPlan(a.T, C, packed_code, ib, ob, cols)
            del os.environ["AFHIP_PACKED_HIST_VEC"]
            p.bind_packing(packed)
            out = p.run(packed, csr)
            for _ in range(a.warmup):
                p.run(packed, csr, out=out)
            torch.cuda.synchronize()
            p.profile_begin(a.launches)
            for _ in range(a.launches):
                p.run(packed, csr, out=out)
            torch.cuda.synchronize()
            ms = p.profile_end()
            med[vec] = float(np.median(ms))
            say(f"  {vec} cell{'s' if vec > 1 else ' '}  {p.describe().split()[0]:56s} {stats(ms)}")
        say(f"  two cells / one cell (medians): {med[2] / med[1]:.3f}")
    for title, (cols, single) in ({} if a.hist_forms else plans_columns()).items():
        if a.plan not in title:
            continue
        ib, ob = (np.array([0, a.T]), np.array([0, 1])) if single else (ib0, np.array([0, len(ib0) - 1]))
        say()
        say(title)
        med, res = {}, {}
        runs = [("packed", packed, packed_code, 0, {})] + [(f"{n} rules", packed, packed_code, n, {}) for n in map(int, a.rules.split(",")) if n]
        if single:      # the knobs are read when a plan is created
            runs += [("general", packed, packed_code, 0, {"AFHIP_NO_PACKED_HIST": "1"}), ("two cells", packed, packed_code, 0, {"AFHIP_PACKED_HIST_VEC": "2"})]
        runs += [("float32", plain, hip.F32, 0, {})]
        for name, cube, code, n_rules, env in runs:
            os.environ.update(env)
            p = hip.FusedPlan(a.T, C, code, ib, ob, cols)
            for k in env:
                del os.environ[k]
            if n_rules:
                p.bind_packings([cube.packing()] * n_rules, [a.T * i // n_rules for i in range(n_rules + 1)])
            elif code == packed_code:
                p.bind_packing(cube)
            out = p.run(cube, csr)
            for _ in range(a.warmup):
                p.run(cube, csr, out=out)
            torch.cuda.synchronize()
            p.profile_begin(a.launches)
            for _ in range(a.launches):
                p.run(cube, csr, out=out)
            torch.cuda.synchronize()
            ms = p.profile_end()
            med[name], res[name] = float(np.median(ms)), out["res"].cpu().numpy()
            nbytes = a.T * C * (2 if code == packed_code else 4)
            extra = f"   spread (max - min) / median {(max(ms) - min(ms)) / med[name]:.4f}" if name == "packed" else \
                    (f"   x {med[name] / med['packed']:.4f} of the single-rule median" if n_rules else
                     (f"   x {med[name] / med['packed']:.3f} of the packed plan's median; minimum {min(ms):.4f} ms" if env else ""))
            say(f"  {name:9s} {p.describe().split()[0]:56s} {stats(ms)}   {nbytes / med[name] / 1e9:.2f} TB/s of its own bytes at the median{extra}")
            if n_rules:
                assert np.array_equal(res[name], res["packed"], equal_nan=True), f"{name}: the panel differs from the single-rule cube's"
            if env:     # (the general kernel's plan has no count records: its weighted sums take another spatial route, and another order of adds)
                with np.errstate(invalid="ignore", divide="ignore"):
                    d = np.nanmax(np.abs(res[name] - res["packed"]) / np.maximum(np.abs(res["packed"]), 1e-300))
                say(f"            its panel differs from the packed plan's by at most {d:.1e} relative ({p.describe().split('|')[2].strip()})")
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.nanmax(np.abs(res["packed"] - res["float32"]) / np.maximum(np.abs(res["float32"]), 1e-300))
        say(f"  packed / float32 kernel time (medians): {med['packed'] / med['float32']:.3f};  panels differ by at most {err:.1e} relative")
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
