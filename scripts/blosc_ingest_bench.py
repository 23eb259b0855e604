#!/usr/bin/env python3
"""Blosc-1 chunks beyond LZ4 + byte shuffle into HBM: the decode-in-HBM route (`io._BloscRoute`: `afhip_lz4_decode_streams`,
`afhip_zstd_decode`, `afhip_unshuffle_blocks`, `afhip_bitunshuffle_blocks`) against the host route (blosc1.c on 16 host threads —
code this route does not touch, so it is the yardstick of the commit before it too).

Workload: the BASELINE configs[0] cube (8760 x 104 x 236 f32, synth.temperature_cube + 273.15) written by `dataset_to_zarr` as Zarr v2
stores under /dev/shm in three flavours — LZ4 + bit shuffle, Zstandard + byte shuffle, Zstandard + bit shuffle — and three layouts:
(24, ny, nx), space-tiled (730, 52, 59), and the converter's whole-series tiles (`io._auto_chunks`).  In one process, after a warm-up
and alternating between the routes, it times `io.array_to_device` on requests of 64 MiB ... the whole cube (powers of two, the first T
steps) with AGGFLY_HIP_GPU_DECODE=0 and =1; medians of --reps runs, one JSON line per (flavour, layout, size), then per flavour the
size from which the GPU route takes <= 0.9 x the host route's time on all three layouts (`io.GPU_DECODE_AUTO_BYTES_BLOSC_BITSHUFFLE`,
`io.GPU_DECODE_AUTO_BYTES_BLOSC_ZSTD`: the larger of its two flavours' sizes; null when there is none).

    python scripts/blosc_ingest_bench.py [--reps 5] [--sizes 256,821] [--flavours blosc-zstd]     # (MiB; default: 64 ... the whole cube)
    python scripts/blosc_ingest_bench.py --profile     # GPU-route reads of the whole cube only (AGGFLY_HIP_INGEST_TRACE=1): run it
                                                       # under rocprofv3 --kernel-trace --stats for the per-kernel shares
    python scripts/blosc_ingest_bench.py --kernels     # k_unshuffle_blocks and k_bitunshuffle_blocks on the cube's block list (256 KiB
                                                       # blocks of 4-byte elements), for a rocprofv3 --kernel-trace --stats run of its own
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
FLAVOURS = ["blosc-bitshuffle", "blosc-zstd", "blosc-zstd-bitshuffle"]


def layouts():
    auto = afio._auto_chunks({"time": T, "latitude": NY, "longitude": NX}, 4)
    return [{"time": 24, "latitude": NY, "longitude": NX}, {"time": 730, "latitude": 52, "longitude": 59},
            {k: (T if v == -1 else v) for k, v in auto.items()}]


def read(za, mode, steps):
    os.environ["AGGFLY_HIP_GPU_DECODE"] = mode
    t0 = time.perf_counter()
    data, _ = afio.array_to_device(za, device="cuda", t_range=(0, steps))
    torch.cuda.synchronize()
    return data, time.perf_counter() - t0


def kernels(reps):
    """Both unshuffle kernels on the block list of the cube: every byte once in, once out."""
    bsize, ts = 256 << 10, 4
    nbytes = T * NY * NX * 4
    nb = -(-nbytes // bsize)
    rec = np.zeros(nb, dtype=codec.SHUFFLE_BLOCK)
    rec["tmp_off"] = rec["out_off"] = np.arange(nb, dtype=np.int64) * bsize
    rec["bsize"] = np.minimum(bsize, nbytes - rec["out_off"])
    rec["typesize"] = ts
    tmp = torch.randint(0, 256, (nb * bsize,), dtype=torch.uint8, device="cuda")
    out = torch.empty(nb * bsize, dtype=torch.uint8, device="cuda")
    dev = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    for _ in range(reps + 1):                                               # (the first launch of each is the warm-up)
        hip.unshuffle_blocks(tmp, out, dev, nb, bsize)
        hip.bitunshuffle_blocks(tmp, out, dev, nb, bsize)
    torch.cuda.synchronize()
    print(json.dumps({"kernels": ["k_unshuffle_blocks", "k_bitunshuffle_blocks"], "blocks": nb, "bsize": bsize, "typesize": ts,
                      "bytes_in_plus_out": 2 * nbytes, "launches_each": reps + 1}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="")
    ap.add_argument("--flavours", default=",".join(FLAVOURS))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.kernels:
        return kernels(a.reps)
    cube = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1) + np.float32(273.15)
    ds = af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                 {"time": pd.date_range("2001-01-01", periods=T, freq="h"), "latitude": 30 + 0.25 * np.arange(NY),
                                  "longitude": 230 + 0.25 * np.arange(NX)}), lon_is_360=True)
    step = NY * NX * 4
    sizes = [s for s in (64 << 20, 128 << 20, 256 << 20, 512 << 20) if s < T * step] + [T * step]
    if a.sizes:
        sizes = [min(int(x) << 20, T * step) for x in a.sizes.split(",")]
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    from_size = {}
    for flavour in a.flavours.split(","):
        ahead = {s: True for s in sizes}
        for chunks in layouts():
            with tempfile.TemporaryDirectory(dir=base) as d:
                af.dataset_to_zarr(ds, d, var="t2m", chunks=chunks, compress=flavour)
                za = afio.ZarrArray(os.path.join(d, "t2m"))
                files = [os.path.join(za.path, f) for f in os.listdir(za.path) if not f.startswith(".")]
                lay = [chunks[k] for k in ("time", "latitude", "longitude")]
                print(json.dumps({"flavour": flavour, "layout": lay, "chunks": len(files), "stored_bytes": sum(os.path.getsize(f) for f in files),
                                  "cube_bytes": T * step, "blosc": codec.blosc_info(open(files[0], "rb").read(16))}), flush=True)
                if a.profile:
                    os.environ["AGGFLY_HIP_INGEST_TRACE"] = "1"       # prints the batches and the pointer-jump rounds
                    read(za, "1", T)
                    _, s = read(za, "1", T)
                    print(json.dumps({"flavour": flavour, "layout": lay, "profile_read_ms": round(s * 1e3, 2)}), flush=True)
                    continue
                for nbytes in sizes:
                    steps = min(T, nbytes // step)
                    got = {m: read(za, m, steps)[0] for m in ("1", "0")}      # warm-up; the routes agree with the source
                    for m in ("1", "0"):
                        assert np.array_equal(got[m].cpu().numpy(), cube[:steps]), (flavour, lay, m)
                    del got
                    t = {"1": [], "0": []}
                    for _ in range(a.reps):                                     # alternating
                        for m in ("1", "0"):
                            t[m].append(read(za, m, steps)[1])
                    gpu, host = statistics.median(t["1"]) * 1e3, statistics.median(t["0"]) * 1e3
                    ahead[nbytes] = ahead[nbytes] and gpu <= 0.9 * host
                    print(json.dumps({"flavour": flavour, "layout": lay, "steps": steps, "request_bytes": steps * step,
                                      "read_ms_median_gpu": round(gpu, 2), "read_ms_median_host": round(host, 2),
                                      "gpu_over_host": round(gpu / host, 3), "decoded_GB_per_s_gpu": round(steps * step / gpu / 1e6, 2),
                                      "decoded_GB_per_s_host": round(steps * step / host / 1e6, 2), "reps": a.reps}), flush=True)
        if a.profile:
            continue
        from_size[flavour] = None
        for s in reversed(sizes):                                           # the smallest size from which every larger one is ahead too
            if not ahead[s]:
                break
            from_size[flavour] = s
        print(json.dumps({"flavour": flavour, "gpu_route_ahead_from_bytes": from_size[flavour]}), flush=True)
    if not a.profile:
        z = [from_size.get(f, None) for f in ("blosc-zstd", "blosc-zstd-bitshuffle") if f in from_size]
        print(json.dumps({"GPU_DECODE_AUTO_BYTES_BLOSC_BITSHUFFLE": from_size.get("blosc-bitshuffle"),
                          "GPU_DECODE_AUTO_BYTES_BLOSC_ZSTD": None if not z or None in z else max(z)}), flush=True)


if __name__ == "__main__":
    main()
