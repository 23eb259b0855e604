#!/usr/bin/env python3
"""Zarr stores written with numcodecs element filters into HBM: the stored int16 elements cross PCIe, `afhip_delta_decode` and
`afhip_fso_decode` make float32 values of them there — against the same integers as a CF-packed int16 store, and the kernels alone.

Workload: the BASELINE configs[0] cube (8760 x 104 x 236 float32, synth.temperature_cube) written into /dev/shm, format 2, Blosc-LZ4 with
the byte shuffle, the converter's `_auto_chunks` (six chunks of 8760 x 87 x 87: 66 million elements each)

  (a) with ``fixedscaleoffset`` (scale 10, offset 273.15) to int16;
  (b) the same with ``delta`` behind it;
  (c) the yardstick: the same integers as a CF-packed int16 store (``scale_factor`` 0.1, ``add_offset`` 273.15) of the same chunks and
      compressor — today's fastest equivalent, unpacked to float32 in HBM by the existing route;

each read by `dataset_from_path(device="cuda")` + `cube()` with AGGFLY_HIP_GPU_DECODE=1 (decode in HBM) and =0 (decode on the host
team), the three routes taking turns, and (a), (b) also by the host route — `dataset_from_path` without ``device=``, un-filtered by `ZarrArray._chunk`, then `to_device()`
—: the time to the cube (median and minimum of --reps, after a warm-up) and `torch.cuda.max_memory_allocated`; then

  (d) with device events, the two kernels alone — the running sum over six chunks of that size (and of one element fewer each: the element-wise path of
      chunks that do not all begin on a 16-byte boundary) and the conversion of the whole cube, in
      bytes moved per second (read + written) — beside `k_place_box` moving one chunk and a bare device-to-device copy.

One JSON line per result.

    python scripts/zarr_filters_ingest_bench.py [--reps 5] [--steps 8760]
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
FSO = {"id": "fixedscaleoffset", "scale": 10.0, "offset": 273.15, "dtype": "<f4", "astype": "<i2"}
DELTA = {"id": "delta", "dtype": "<i2", "astype": "<i2"}
BLOSC = {"id": "blosc", "cname": "lz4", "clevel": 5, "shuffle": 1, "blocksize": 0}


def timed(fns, reps):
    """The routes ``fns`` timed in turn, ``reps`` rounds (alternating: what else the host does hits all of them alike)
    -> per route (median ms, min ms, peak bytes allocated during the last call, the shape the last call returned)."""
    ms, peak, shape = [[] for _ in fns], [0] * len(fns), [None] * len(fns)
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms[i].append((time.perf_counter() - t0) * 1e3)
            peak[i], shape[i] = torch.cuda.max_memory_allocated(), tuple(out.shape)
            del out
    return [(round(statistics.median(m), 2), round(min(m), 2), p, s) for m, p, s in zip(ms, peak, shape)]


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
    cube = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=11) + np.float32(273.15)          # kelvin, as ERA5 stores t2m
    time_ = pd.date_range("2010-01-01", periods=T, freq="h")
    lat, lon = 30 + 0.25 * np.arange(NY), 230 + 0.25 * np.arange(NX)
    ds = af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"], {"time": time_, "latitude": lat, "longitude": lon}), lon_is_360=True)
    auto = afio._auto_chunks({"time": T, "latitude": NY, "longitude": NX}, 4)
    chunks = {d: (n if auto[d] == -1 else auto[d]) for d, n in (("time", T), ("latitude", NY), ("longitude", NX))}
    print(json.dumps({"device": hip.device_info(0)["name"], "cube": [T, NY, NX], "dtype": "float32", "bytes": int(cube.nbytes), "reps": args.reps,
                      "chunks": chunks}))
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        pa, pb, pc = (os.path.join(tmp, n) for n in ("fso.zarr", "fso_delta.zarr", "cf.zarr"))
        af.dataset_to_zarr(ds, pa, var="t2m", chunks=chunks, filters=[FSO])
        af.dataset_to_zarr(ds, pb, var="t2m", chunks=chunks, filters=[FSO, DELTA])
        stored = afio.filter_elements(cube, afio._parse_elem_filters([FSO], cube.dtype)[0]).reshape(cube.shape)      # the same integers
        af.dataset_to_zarr(ds, pc, var="t2m", chunks=chunks)                                                       # (coordinates, group)
        afio._write_array(pc, "t2m", stored, ("time", "latitude", "longitude"), tuple(chunks[d] for d in ("time", "latitude", "longitude")),
                          {"scale_factor": 0.1, "add_offset": 273.15}, BLOSC)
        for name, p in (("a fso", pa), ("b fso+delta", pb), ("c cf-packed", pc)):
            z = afio.ZarrArray(os.path.join(p, "t2m"))
            size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(z.path) for f in fs)
            print(json.dumps({"store": name, "dtype": z.dtype.name, "stored_dtype": z.stored_dtype.name, "chunks": z.chunks, "codec": z.native_kind,
                              "filters": [f["id"] for f in z.elem_filters], "stored_bytes": size}))

        dev = lambda p: (lambda: af.dataset_from_path(p, "t2m", device="cuda").cube())
        host = lambda p: (lambda: af.dataset_from_path(p, "t2m").to_device().cube())
        want = afio.unfilter_elements(stored, afio._parse_elem_filters([FSO], cube.dtype)[0]).reshape(cube.shape)
        for p in (pa, pb):
            got = dev(p)()
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
            del got
        results = {}
        for mode in ("1", "0"):
            os.environ["AGGFLY_HIP_GPU_DECODE"] = mode
            routes = [("a", "fixedscaleoffset -> int16", dev(pa)), ("b", "fixedscaleoffset + delta", dev(pb)),
                      ("c", "CF-packed int16, the same integers (yardstick)", dev(pc))]
            for _, _, fn in routes:                                 # warm-up: page-locked buffers, kernels, page cache
                fn()
            for (name, what, _), (med, lo, peak, shape) in zip(routes, timed([fn for _, _, fn in routes], args.reps)):
                results[(name, mode)] = med
                print(json.dumps({"route": name, "what": what, "gpu_decode": mode, "ms_median": med, "ms_min": lo,
                                  "GB_per_s": round(cube.nbytes / med / 1e6, 2), "peak_allocated_MB": round(peak / 1e6, 1), "cube_shape": shape}))
            print(json.dumps({"gpu_decode": mode, "a_over_c": round(results[("a", mode)] / results[("c", mode)], 3),
                              "b_over_c": round(results[("b", mode)] / results[("c", mode)], 3)}))
        os.environ.pop("AGGFLY_HIP_GPU_DECODE", None)
        hosts = (("a", "fixedscaleoffset -> int16", host(pa)), ("b", "fixedscaleoffset + delta", host(pb)))
        for _, _, fn in hosts:
            fn()
        for (name, what, _), (med, lo, peak, shape) in zip(hosts, timed([fn for _, _, fn in hosts], max(2, args.reps // 2))):
            print(json.dumps({"route": name, "what": what + ", host route (ZarrArray._chunk, then to_device)", "ms_median": med, "ms_min": lo,
                              "GB_per_s": round(cube.nbytes / med / 1e6, 2), "cube_shape": shape,
                              "over_device_1": round(med / results[(name, "1")], 2), "over_device_0": round(med / results[(name, "0")], 2)}))

    # (d) the kernels alone
    tc, yc, xc = (chunks[d] for d in ("time", "latitude", "longitude"))
    n_chunks, ce = 6, tc * yc * xc
    reps = max(args.reps, 9)
    stage = torch.randint(-30000, 30000, (n_chunks * ce,), dtype=torch.int16, device="cuda")
    scratch = torch.empty(hip.delta_scratch_bytes(n_chunks, ce, 2), dtype=torch.uint8, device="cuda")
    med, lo = events(lambda: hip.delta_decode(stage, n_chunks, ce, 2, scratch), reps)
    print(json.dumps({"kernel": "afhip_delta_decode (3 launches)", "elem_size": 2, "chunks": n_chunks, "chunk_elems": ce, "bytes": n_chunks * ce * 2,
                      "ms_median": round(med, 4), "ms_min": round(lo, 4), "moved_GB_per_s": round(3 * n_chunks * ce * 2 / med / 1e6, 1),
                      "note": "moved = two reads and one write of the data"}))
    # chunks whose byte count is no multiple of 16 do not all begin on a 16-byte boundary: the kernels then take elements one by one
    odd = ce - 1
    med, lo = events(lambda: hip.delta_decode(stage, n_chunks, odd, 2, scratch), reps)
    print(json.dumps({"kernel": "afhip_delta_decode (3 launches), element-wise: chunk bytes % 16 != 0", "elem_size": 2, "chunks": n_chunks,
                      "chunk_elems": odd, "bytes": n_chunks * odd * 2, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                      "moved_GB_per_s": round(3 * n_chunks * odd * 2 / med / 1e6, 1)}))
    n = T * NY * NX
    src = stage[:n]
    dst = torch.empty(n, dtype=torch.float32, device="cuda")
    med, lo = events(lambda: hip.fso_decode(src, dst, n, "int16", 10.0, 273.15), reps)
    print(json.dumps({"kernel": "k_fso_decode int16 -> float32", "elements": n, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                      "moved_GB_per_s": round(6 * n / med / 1e6, 1)}))
    chunk = stage[:ce].view(tc, yc, xc)
    out = torch.empty((tc, yc, xc + 17), dtype=torch.int16, device="cuda")
    med, lo = events(lambda: hip.place_box(chunk, out, (0, 0, 0, tc, yc, xc), (0, 0, 9)), reps)
    print(json.dumps({"kernel": "k_place_box", "elem_size": 2, "chunk": [tc, yc, xc], "ms_median": round(med, 4), "ms_min": round(lo, 4),
                      "moved_GB_per_s": round(4 * ce / med / 1e6, 1)}))
    flat = torch.empty(n_chunks * ce, dtype=torch.int16, device="cuda")
    med, lo = events(lambda: flat.copy_(stage), reps)
    print(json.dumps({"kernel": "device copy", "bytes": n_chunks * ce * 2, "ms_median": round(med, 4), "ms_min": round(lo, 4),
                      "moved_GB_per_s": round(4 * n_chunks * ce / med / 1e6, 1)}))


if __name__ == "__main__":
    main()
