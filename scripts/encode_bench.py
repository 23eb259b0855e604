#!/usr/bin/env python3
"""Writing Zarr stores from a device-resident cube: `dataset_to_zarr` with the chunks cut, shuffled and LZ4-encoded in HBM
(`encode="gpu"`: `io._write_chunks_gpu` — `afhip_take_box`, `afhip_shuffle_blocks`, `afhip_lz4_encode_streams`, `afhip_copy_ranges`)
against the host route (`encode="host"`: the cube downloaded, chunks cut in Python, blosc1.c + liblz4 on up to 16 host threads).

Workload: the BASELINE configs[0] cube (8760 x 104 x 236 f32, synth.temperature_cube + 273.15) in HBM, written as Zarr v2 stores under
/dev/shm in the three layouts the decode benches use — (1, ny, nx), (24, ny, nx) and the converter's whole-series tiles
(`io._auto_chunks`) — at 64 MiB ... the whole cube (the first T steps).  In one process, after a warm-up of both routes and alternating
between them: wall time of `dataset_to_zarr` as min / median / max of --reps runs, the bytes of the data variable's files on both
routes, one JSON line per (layout, size).  Then per layout the kernel times of one batch, pass by pass (HIP events), and last the size
`io.GPU_ENCODE_AUTO_BYTES` follows from: the smallest from which, on every layout and for every larger size, the GPU route's median is
<= 0.9 x the host route's minimum AND the GPU-written store is at most 1.10 x the host-written one; null when there is none, with the
condition that fails.

--compress blosc-zstd is the same bench for Zstandard streams (`afhip_zstd_encode_blocks` in place of the LZ4 kernel; the host route:
libzstd level 3 through `afcodec_blosc_encode`); its last line names `io.GPU_ENCODE_AUTO_BYTES_BLOSC_ZSTD`.

    python scripts/encode_bench.py [--reps 3] [--sizes 64,821] [--compress blosc|blosc-zstd]      # (MiB; default: 64 ... the whole cube)
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
from aggfly_amd import codec, hip, io as afio, synth  # noqa: E402

T, NY, NX = 8760, 104, 236


def layouts():
    auto = afio._auto_chunks({"time": T, "latitude": NY, "longitude": NX}, 4)
    return [{"time": 1, "latitude": NY, "longitude": NX}, {"time": 24, "latitude": NY, "longitude": NX},
            {k: (-1 if v == -1 else v) for k, v in auto.items()}]


def dataset(cube):
    steps = cube.shape[0]
    return af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                   {"time": pd.date_range("2001-01-01", periods=steps, freq="h"), "latitude": 30 + 0.25 * np.arange(NY),
                                    "longitude": 230 + 0.25 * np.arange(NX)}), lon_is_360=True)


COMPRESS = "blosc"


def write(ds, base, chunks, route):
    with tempfile.TemporaryDirectory(dir=base) as d:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        af.dataset_to_zarr(ds, d, var="t2m", chunks=chunks, encode=route, compress=COMPRESS)
        torch.cuda.synchronize()
        s = time.perf_counter() - t0
        var = os.path.join(d, "t2m")
        stored = sum(os.path.getsize(os.path.join(var, f)) for f in os.listdir(var) if not f.startswith("."))
    return s, stored


def kernel_times(cube_dev, chunks, reps):
    """One batch of the route's kernels (`io._write_chunks_gpu`), each pass between HIP events: min ms of `reps` runs."""
    shape = tuple(cube_dev.shape)
    ct = tuple(shape[i] if chunks[k] == -1 else min(chunks[k], shape[i]) for i, k in enumerate(("time", "latitude", "longitude")))
    cb = int(np.prod(ct)) * 4
    grid = [-(-s // c) for s, c in zip(shape, ct)]
    idxs = list(np.ndindex(*grid))[:max(1, afio.GPU_ENCODE_BATCH_BYTES // cb)]
    n = len(idxs)
    zstd = COMPRESS == "blosc-zstd"
    pl = (codec.BloscZstdEncodePlan if zstd else codec.BloscEncodePlan)(n, cb, 4)
    rec = torch.from_numpy(np.concatenate([pl.streams.view(np.uint8), pl.blocks.view(np.uint8)])).cuda()
    if zstd:                                                                   # (the route's buffers: the shuffled input and the slots in one)
        chunk_dev = torch.empty(n * cb, dtype=torch.uint8, device="cuda")
        tmp_dev = slots_dev = torch.empty(pl.work_bytes, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(pl.scratch_bytes, dtype=torch.uint8, device="cuda")
    else:
        chunk_dev, tmp_dev, slots_dev = (torch.empty(n * cb, dtype=torch.uint8, device="cuda") for _ in range(3))
    packed = torch.empty(n * (cb + pl.header_bytes + 4 * pl.per_chunk), dtype=torch.uint8, device="cuda")
    csize = torch.empty(len(pl.streams), dtype=torch.int32, device="cuda")
    fill = int(np.array([np.nan], dtype=np.float32).view(np.uint32)[0])
    cview = chunk_dev.view(torch.float32)
    best = {}

    def timed(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        best[name] = min(best.get(name, 1e30), e0.elapsed_time(e1))

    def take():
        j = 0
        while j < n:                                                           # (chunks that follow one another in time: one launch, as the route does)
            idx, m = idxs[j], 1
            while j + m < n and idxs[j + m] == (idx[0] + m,) + tuple(idx[1:]):
                m += 1
            at = tuple(i * c for i, c in zip(idx, ct))
            run = (m * ct[0],) + ct[1:]
            box = tuple(min(c, s - a) for c, s, a in zip(run, shape, at))
            hip.take_box(cube_dev, cview[j * (cb // 4):(j + m) * (cb // 4)].view(run), at, box, fill)
            j += m

    def shuffle():
        nb = len(pl.blocks)
        for b0 in range(0, nb, 65535):
            hip.shuffle_blocks(chunk_dev, tmp_dev, rec[pl.streams.nbytes + b0 * codec.SHUFFLE_BLOCK.itemsize:], min(65535, nb - b0), pl.max_bsize)

    for _ in range(reps + 1):
        timed("take_box", take)
        timed("shuffle_blocks", shuffle)
        if zstd:
            timed("zstd_encode_blocks", lambda: hip.zstd_encode_blocks(tmp_dev, rec, len(pl.streams), scratch, tmp_dev[pl.slot_base:], csize))
        else:
            timed("lz4_encode_streams", lambda: hip.lz4_encode_streams(tmp_dev, rec, len(pl.streams), slots_dev, csize))
        cs = csize.cpu().numpy()
        ranges, off, size = pl.place(cs)
        rdev = torch.from_numpy(ranges.view(np.uint8)).cuda()
        timed("copy_ranges", lambda: hip.copy_ranges(slots_dev, packed, rdev, len(ranges)))
    stored = pl.stored_frames if zstd else int((cs == pl.streams["dsize"]).sum())
    return {"chunks": n, "batch_bytes": n * cb, "streams": len(pl.streams), "stored_streams": stored, "packed_bytes": int(size.sum()),
            "ms": {k: round(v, 3) for k, v in best.items()},
            "GB_per_s": {k: round(n * cb / v / 1e6, 1) for k, v in best.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="")
    ap.add_argument("--compress", default="blosc", choices=("blosc", "blosc-zstd"))
    a = ap.parse_args()
    global COMPRESS
    COMPRESS = a.compress
    cube = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1) + np.float32(273.15)
    step = NY * NX * 4
    sizes = [s for s in (64 << 20, 128 << 20, 256 << 20, 512 << 20) if s < T * step] + [T * step]
    if a.sizes:
        sizes = [min(int(x) << 20, T * step) for x in a.sizes.split(",")]
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    ok_time, ok_size, worst = {s: True for s in sizes}, {s: True for s in sizes}, {s: [0.0, 0.0] for s in sizes}
    for chunks in layouts():
        lay = [chunks[k] for k in ("time", "latitude", "longitude")]
        for nbytes in sizes:
            steps = min(T, nbytes // step)
            ds = dataset(cube[:steps]).to_device()
            for route in ("gpu", "host"):                                      # warm-up
                write(ds, base, chunks, route)
            t, stored = {"gpu": [], "host": []}, {}
            for _ in range(a.reps):                                            # alternating
                for route in ("gpu", "host"):
                    s, stored[route] = write(ds, base, chunks, route)
                    t[route].append(s * 1e3)
            gpu_med, host_min = statistics.median(t["gpu"]), min(t["host"])
            ratio = stored["gpu"] / stored["host"]
            ok_time[nbytes] = ok_time[nbytes] and gpu_med <= 0.9 * host_min
            ok_size[nbytes] = ok_size[nbytes] and ratio <= 1.10
            worst[nbytes] = [max(worst[nbytes][0], gpu_med / host_min), max(worst[nbytes][1], ratio)]
            print(json.dumps({"layout": lay, "steps": steps, "cube_bytes": steps * step, "reps": a.reps,
                              "gpu_ms_min_median_max": [round(min(t["gpu"]), 1), round(gpu_med, 1), round(max(t["gpu"]), 1)],
                              "host_ms_min_median_max": [round(host_min, 1), round(statistics.median(t["host"]), 1), round(max(t["host"]), 1)],
                              "gpu_median_over_host_min": round(gpu_med / host_min, 3), "raw_GB_per_s_gpu": round(steps * step / gpu_med / 1e6, 2),
                              "raw_GB_per_s_host": round(steps * step / host_min / 1e6, 2), "stored_bytes_gpu": stored["gpu"],
                              "stored_bytes_host": stored["host"], "gpu_store_over_host_store": round(ratio, 4)}), flush=True)
            del ds
        print(json.dumps({"layout": lay, "kernels_of_one_batch": kernel_times(torch.from_numpy(cube).cuda(), chunks, a.reps)}), flush=True)
    from_size = None
    for s in reversed(sizes):                                                  # the smallest size from which every larger one holds too
        if not (ok_time[s] and ok_size[s]):
            break
        from_size = s
    print(json.dumps({"GPU_ENCODE_AUTO_BYTES_BLOSC_ZSTD" if COMPRESS == "blosc-zstd" else "GPU_ENCODE_AUTO_BYTES": from_size,
                      "time_rule_holds_at_bytes": [s for s in sizes if ok_time[s]], "size_rule_holds_at_bytes": [s for s in sizes if ok_size[s]],
                      "worst_gpu_median_over_host_min_by_size": {str(s): round(worst[s][0], 3) for s in sizes},
                      "worst_gpu_store_over_host_store_by_size": {str(s): round(worst[s][1], 4) for s in sizes}}), flush=True)


if __name__ == "__main__":
    main()
