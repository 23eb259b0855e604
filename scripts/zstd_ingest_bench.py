#!/usr/bin/env python3
"""Zstandard stores into HBM: the decode-in-HBM route (`afhip_zstd_decode`) against the host route (libzstd, a chunk per
host thread), next to the Blosc-LZ4 store of scripts/e2e_bench.py.

Workload: the BASELINE configs[0] cube (8760 x 104 x 236 f32, synth.temperature_cube) written by
`dataset_to_zarr(compress="zstd", zarr_format=3)` with default chunks — the layout the reference's converter writes (whole
time series in square tiles: 6 chunks of 265 MB, one frame each) — into /dev/shm.  In one process, after a warm-up and
alternating between the routes, it times store -> HBM and the whole configs[0] job (open + decode + H2D, weights, kernels,
frame).  Smaller requests of the same layout (--sizes) place the `auto` threshold.  One JSON line per result.

    python scripts/zstd_ingest_bench.py [--reps 5] [--sizes 730,2190,4380]
    python scripts/zstd_ingest_bench.py --profile     # one GPU-route read only: run it under rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import synth  # noqa: E402

NY, NX, R = 104, 236, 3100


def dataset(T):
    arr = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1) + np.float32(273.15)
    tindex = pd.date_range("2001-01-01", periods=T, freq="h")
    lat, lon = 25 + 0.25 * np.arange(NY), 235 + 0.25 * np.arange(NX)
    return af.Dataset(af.DataArray(arr, ["time", "latitude", "longitude"], {"time": tindex, "latitude": lat, "longitude": lon}), lon_is_360=True)


def store_bytes(path):
    return sum(os.path.getsize(os.path.join(r, f)) for r, _, fs in os.walk(path) for f in fs)


def read(store, mode):
    os.environ["AGGFLY_HIP_GPU_DECODE"] = mode
    t0 = time.perf_counter()
    ds = af.dataset_from_path(store, "t2m", lon_is_360=True, preprocess=lambda x: x - 273.15, device="cuda")
    torch.cuda.synchronize()
    return ds, time.perf_counter() - t0


def job(store, mode, gr, tab, spec):
    t0 = time.perf_counter()
    ds, _ = read(store, mode)
    w = af.weights_from_objects(ds, gr, table=tab)
    df = af.aggregate_dataset(dataset=ds, weights=w, **spec)
    torch.cuda.synchronize()
    return df, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="730,2190,4380")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=base) as d:
        if a.profile:
            zs = os.path.join(d, "zstd.zarr")
            af.dataset_to_zarr(dataset(8760), zs, var="t2m", compress="zstd", zarr_format=3)
            read(zs, "1")                                 # warm
            os.environ["AGGFLY_HIP_INGEST_TRACE"] = "1"   # prints the pointer-jump rounds
            _, s = read(zs, "1")
            print(json.dumps({"profile_read_ms": round(s * 1e3, 2)}), flush=True)
            return
        ds0 = dataset(8760)
        zs, bs = os.path.join(d, "zstd.zarr"), os.path.join(d, "blosc.zarr")
        af.dataset_to_zarr(ds0, zs, var="t2m", compress="zstd", zarr_format=3)
        af.dataset_to_zarr(ds0, bs, var="t2m", chunks={"time": 24, "latitude": NY, "longitude": NX}, compress="blosc")
        cube_bytes = 8760 * NY * NX * 4
        tab = synth.weights_table(NY, NX, R, seed=2)
        gr = af.GeoRegions(pd.DataFrame({"geoid": [f"r{i:05d}" for i in range(int(tab.index_right.max()) + 1)]}))
        spec = dict(tavg=[("aggregate", {"calc": "mean", "groupby": "date"}), ("transform", {"transform": "power", "exp": np.arange(1, 3)}),
                          ("aggregate", {"calc": "sum", "groupby": "year"})])
        routes = [("zstd", zs, "1"), ("zstd", zs, "0"), ("blosc-lz4", bs, "auto")]
        ref = None
        for name, st, mode in routes:                     # warm-up; the three cubes agree
            ds, _ = read(st, mode)
            c = ds.cube().cpu().numpy()
            if ref is None:
                ref = c
            assert np.array_equal(c, ref, equal_nan=True), (name, mode)
            job(st, mode, gr, tab, spec)
        del ref
        reads = {r: [] for r in routes}
        jobs = {r: [] for r in routes}
        panels = {}
        for _ in range(a.reps):                          # alternating
            for r in routes:
                reads[r].append(read(r[1], r[2])[1])
            for r in routes:
                df, s = job(r[1], r[2], gr, tab, spec)
                jobs[r].append(s)
                panels[r] = df
        p0 = panels[routes[0]]
        for r in routes:
            pd.testing.assert_frame_equal(panels[r], p0)
            ms = statistics.median(reads[r]) * 1e3
            print(json.dumps({"store": r[0], "AGGFLY_HIP_GPU_DECODE": r[2], "store_bytes": store_bytes(r[1]), "cube_bytes": cube_bytes,
                              "read_ms_median": round(ms, 2), "read_ms_min": round(min(reads[r]) * 1e3, 2),
                              "decoded_GB_per_s": round(cube_bytes / ms / 1e6, 2),
                              "job_ms_median": round(statistics.median(jobs[r]) * 1e3, 2), "job_ms_min": round(min(jobs[r]) * 1e3, 2),
                              "reps": a.reps}), flush=True)
        # smaller requests of the same layout: where the GPU route starts to be ahead
        for T in [int(x) for x in a.sizes.split(",") if x]:
            p = os.path.join(d, f"zstd_{T}.zarr")
            af.dataset_to_zarr(dataset(T), p, var="t2m", compress="zstd", zarr_format=3)
            for mode in ("1", "0"):
                read(p, mode)
            t = {"1": [], "0": []}
            for _ in range(a.reps):
                for mode in ("1", "0"):
                    t[mode].append(read(p, mode)[1])
            print(json.dumps({"store": "zstd", "T": T, "request_bytes": T * NY * NX * 4,
                              "read_ms_median_gpu": round(statistics.median(t["1"]) * 1e3, 2),
                              "read_ms_median_host": round(statistics.median(t["0"]) * 1e3, 2)}), flush=True)


if __name__ == "__main__":
    main()
