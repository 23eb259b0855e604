#!/usr/bin/env python3
"""Time-last Zarr stores into HBM: the route that transposes every chunk into the time-major cube (`afhip_place_box_tlast`) against
the time-major store of the same chunk extents, against what the parent commit did with a time-last store, and the kernel alone.

Workload: the BASELINE configs[0] cube (8760 x 104 x 236 float32, synth.temperature_cube) written into /dev/shm

  (a) as the reference's converter writes it — (latitude, longitude, time), format 3, zstd, `_auto_chunks` (87 x 87 tiles with the whole
      series) — and read by `dataset_from_path(device="cuda")` + `cube()` with AGGFLY_HIP_GPU_DECODE=1 and =0;
  (b) as a time-major store of the same chunk extents and codec, on the route that existed before: the yardstick;
  (c) the time-last store the way the parent commit read it: the array streamed as stored (`zarr_to_device`, generic 3-D) and the
      permuted copy every `Dataset.cube()` call then made;

each with the time to the cube (median and minimum of --reps, after a warm-up, alternating) and `torch.cuda.max_memory_allocated`; then

  (d) with device events, the kernel alone on one chunk of that layout for 2-, 4- and 8-byte elements, against `k_place_box` moving the
      same number of bytes out of a time-major chunk and against a bare device-to-device copy of them.

One JSON line per result.

    python scripts/time_last_ingest_bench.py [--reps 5] [--steps 8760]
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
from aggfly_amd import hip, io as afio, synth  # noqa: E402

NY, NX = 104, 236


def timed(fn, reps):
    """-> (median ms, min ms, peak bytes allocated during the last call, what the last call returned a shape of)."""
    ms, peak, shape = [], 0, None
    for _ in range(reps):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        peak, shape = torch.cuda.max_memory_allocated(), tuple(out.shape)
        del out
    return round(statistics.median(ms), 2), round(min(ms), 2), peak, shape


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8760)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    args = ap.parse_args()
    hip.require_gpu()
    T = args.steps
    cube = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=11)
    ds = af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                 {"time": pd.date_range("2010-01-01", periods=T, freq="h"), "latitude": 30 + 0.25 * np.arange(NY),
                                  "longitude": 230 + 0.25 * np.arange(NX)}), lon_is_360=True)
    print(json.dumps({"device": hip.device_info(0)["name"], "cube": [T, NY, NX], "dtype": "float32", "bytes": int(cube.nbytes), "reps": args.reps}))
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        last, major = os.path.join(tmp, "last.zarr"), os.path.join(tmp, "major.zarr")
        af.dataset_to_zarr(ds, last, var="t2m", compress="zstd", zarr_format=3, layout="time-last")
        zl = afio.ZarrArray(os.path.join(last, "t2m"))
        yc, xc, tc = zl.chunks
        af.dataset_to_zarr(ds, major, var="t2m", chunks={"time": tc, "latitude": yc, "longitude": xc}, compress="zstd", zarr_format=3)
        zm = afio.ZarrArray(os.path.join(major, "t2m"))
        for name, z in (("time-last", zl), ("time-major", zm)):     # (the two hold different byte streams: their compressed sizes differ)
            stored = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(z.path) for f in fs)
            print(json.dumps({"store": name, "dims": z.dims, "shape": z.shape, "chunks": z.chunks, "codec": z.native_kind, "stored_bytes": stored}))

        def route_a():
            return af.dataset_from_path(last, "t2m", device="cuda").cube()

        def route_b():
            return af.dataset_from_path(major, "t2m", device="cuda").cube()

        def route_c():
            stored, _ = afio.zarr_to_device(last, "t2m", device="cuda")           # (latitude, longitude, time) in HBM, as the parent left it
            return stored.permute(2, 0, 1).contiguous()                           # what every cube() / packed_cube() call then made

        check = route_a()
        assert check.is_contiguous() and np.array_equal(check.cpu().numpy(), cube, equal_nan=True)
        del check
        results = {}
        for mode in ("1", "0"):
            os.environ["AGGFLY_HIP_GPU_DECODE"] = mode
            for fn in (route_a, route_b, route_c):                                # warm-up: page-locked buffers, kernels, page cache
                fn()
            for name, what, fn in (("a", "time-last store, transposing placement", route_a), ("b", "time-major store, same chunk extents (yardstick)", route_b),
                                   ("c", "time-last store as the parent commit read it: as stored + the cube() copy", route_c)):
                med, lo, peak, shape = timed(fn, args.reps)
                results[(name, mode)] = med
                print(json.dumps({"route": name, "what": what, "gpu_decode": mode, "ms_median": med, "ms_min": lo,
                                  "GB_per_s": round(cube.nbytes / med / 1e6, 2), "peak_allocated_MB": round(peak / 1e6, 1), "cube_shape": shape}))
            print(json.dumps({"gpu_decode": mode, "a_over_b": round(results[("a", mode)] / results[("b", mode)], 3),
                              "c_over_a": round(results[("c", mode)] / results[("a", mode)], 3)}))
        os.environ.pop("AGGFLY_HIP_GPU_DECODE", None)

    # (d) the kernel alone: one chunk [yc][xc][tc] into a cube [tc][yc][xc + 17] (rows of the cube longer than the box, as in a store)
    for es, dt in ((2, torch.int16), (4, torch.int32), (8, torch.int64)):
        n = yc * xc * tc
        src_last = torch.randint(-30000, 30000, (yc, xc, tc), dtype=dt, device="cuda")
        src_major = src_last.permute(2, 0, 1).contiguous()
        out = torch.empty((tc, yc, xc + 17), dtype=dt, device="cuda")
        flat = torch.empty(n, dtype=dt, device="cuda")
        hip.place_box_tlast(src_last, out, (0, 0, 0, yc, xc, tc), (0, 0, 9))
        assert torch.equal(out[:, :, 9:9 + xc], src_major)
        for name, fn in (("k_place_box_tlast", lambda: hip.place_box_tlast(src_last, out, (0, 0, 0, yc, xc, tc), (0, 0, 9))),
                         ("k_place_box", lambda: hip.place_box(src_major, out, (0, 0, 0, tc, yc, xc), (0, 0, 9))),
                         ("device copy", lambda: flat.copy_(src_last.view(-1)))):
            med, lo = events(fn, max(args.reps, 9))
            print(json.dumps({"kernel": name, "elem_size": es, "chunk": [yc, xc, tc], "bytes": n * es, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                              "moved_GB_per_s": round(2 * n * es / med / 1e6, 1)}))
        del src_last, src_major, out, flat


if __name__ == "__main__":
    main()
