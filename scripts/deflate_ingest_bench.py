#!/usr/bin/env python3
"""netCDF-4-style chunks (byte shuffle + deflate) into HBM: the decode-in-HBM route (`afhip_inflate_decode`) against the host route
(zlib's inflate + unshuffle, a chunk per host thread).

Workload: the BASELINE configs[0] cube (8760 x 104 x 236 f32, synth.temperature_cube + 273.15) written as shuffle + deflate level 4
chunks into plain chunk files under /dev/shm, in three layouts — (1, ny, nx), netCDF4-python's default for a record dimension;
(24, ny, nx); and space-tiled (730, 52, 59) — and presented through a minimal duck-typed source (`ChunkFiles`: what `io.array_to_device`
asks of an `hdf5.ChunkSource`; there is no HDF5 writer here).  In one process, after a warm-up and alternating between the routes, it
times `io.array_to_device` on requests of 64 MiB ... the whole cube (powers of two, the first T steps) with AGGFLY_HIP_GPU_DECODE=0
(16 host threads) and =1; medians of --reps runs, one JSON line per (layout, size), then the size from which the GPU route takes
<= 0.9 x the host route's time on all three layouts (`io.GPU_DECODE_AUTO_BYTES_DEFLATE`; null when there is none).

    python scripts/deflate_ingest_bench.py [--reps 5] [--sizes 256,821]     # (MiB; default: 64 ... the whole cube)
    python scripts/deflate_ingest_bench.py --profile     # GPU-route reads of the whole cube only (AGGFLY_HIP_INGEST_TRACE=1): run it
                                                         # under rocprofv3 --kernel-trace --stats for the per-pass shares
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from aggfly_amd import io as afio, synth  # noqa: E402

T, NY, NX = 8760, 104, 236
LAYOUTS = [(1, NY, NX), (24, NY, NX), (730, 52, 59)]


class ChunkFiles:
    """Chunk files ``t.y.x`` of one array, each a zlib stream of the byte-shuffled chunk."""

    def __init__(self, root, shape, chunks, dtype):
        self.path, self.shape, self.chunks = root, tuple(shape), tuple(chunks)
        self.dtype = self.disk_dtype = np.dtype(dtype)
        self.native_kind = ("zlib", self.dtype.itemsize)
        self.chunk_nbytes = int(np.prod(chunks)) * self.dtype.itemsize
        self.attrs = {}

    def chunk_locator(self, idx, probe=True):
        return os.path.join(self.path, "%d.%d.%d" % tuple(idx)), 0, -1

    def _fill(self):
        return np.nan


def write(root, cube, chunks, level=4):
    os.makedirs(root)
    tc, yc, xc = chunks
    ts = cube.dtype.itemsize

    def one(idx):
        it, iy, ix = idx
        blk = np.ascontiguousarray(cube[it * tc:(it + 1) * tc, iy * yc:(iy + 1) * yc, ix * xc:(ix + 1) * xc])
        planes = blk.view(np.uint8).reshape(-1, ts).T.tobytes()
        with open(os.path.join(root, "%d.%d.%d" % idx), "wb") as f:
            f.write(zlib.compress(planes, level))

    grid = [(it, iy, ix) for it in range(cube.shape[0] // tc) for iy in range(cube.shape[1] // yc) for ix in range(cube.shape[2] // xc)]
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(one, grid))
    return ChunkFiles(root, cube.shape, chunks, cube.dtype)


def read(src, mode, steps):
    os.environ["AGGFLY_HIP_GPU_DECODE"] = mode
    t0 = time.perf_counter()
    data, _ = afio.array_to_device(src, device="cuda", t_range=(0, steps))
    torch.cuda.synchronize()
    return data, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    cube = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1) + np.float32(273.15)
    step = NY * NX * 4
    sizes = [s for s in (64 << 20, 128 << 20, 256 << 20, 512 << 20) if s < T * step] + [T * step]
    if a.sizes:
        sizes = [min(int(x) << 20, T * step) for x in a.sizes.split(",")]
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=base) as d:
        srcs = [write(os.path.join(d, "c%d" % i), cube, ch) for i, ch in enumerate(LAYOUTS)]
        for src in srcs:
            stored = sum(os.path.getsize(os.path.join(src.path, f)) for f in os.listdir(src.path))
            print(json.dumps({"layout": src.chunks, "chunks": len(os.listdir(src.path)), "stored_bytes": stored, "cube_bytes": T * step}), flush=True)
        if a.profile:
            os.environ["AGGFLY_HIP_INGEST_TRACE"] = "1"       # prints the batches and the pointer-jump rounds
            for src in srcs:
                read(src, "1", T)
                _, s = read(src, "1", T)
                print(json.dumps({"layout": src.chunks, "profile_read_ms": round(s * 1e3, 2)}), flush=True)
            return
        ahead = {s: True for s in sizes}
        for src in srcs:
            for nbytes in sizes:
                steps = min(T, nbytes // step)
                got = {m: read(src, m, steps)[0] for m in ("1", "0")}      # warm-up; the routes agree with the source
                for m in ("1", "0"):
                    assert np.array_equal(got[m].cpu().numpy(), cube[:steps]), (src.chunks, m)
                del got
                t = {"1": [], "0": []}
                for _ in range(a.reps):                                     # alternating
                    for m in ("1", "0"):
                        t[m].append(read(src, m, steps)[1])
                gpu, host = statistics.median(t["1"]) * 1e3, statistics.median(t["0"]) * 1e3
                ahead[nbytes] = ahead[nbytes] and gpu <= 0.9 * host
                print(json.dumps({"layout": src.chunks, "steps": steps, "request_bytes": steps * step, "read_ms_median_gpu": round(gpu, 2),
                                  "read_ms_median_host": round(host, 2), "gpu_over_host": round(gpu / host, 3),
                                  "decoded_GB_per_s_gpu": round(steps * step / gpu / 1e6, 2),
                                  "decoded_GB_per_s_host": round(steps * step / host / 1e6, 2), "reps": a.reps}), flush=True)
        from_size = None
        for s in reversed(sizes):                                           # the smallest size from which every larger one is ahead too
            if not ahead[s]:
                break
            from_size = s
        print(json.dumps({"GPU_DECODE_AUTO_BYTES_DEFLATE": from_size}), flush=True)


if __name__ == "__main__":
    main()
