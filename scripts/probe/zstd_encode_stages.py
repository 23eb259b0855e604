#!/usr/bin/env python3
"""The three stages of k_zstd_encode_blocks — matches, sequences, literals — as shares of the kernel's time on one batch of the
production route (the configs[0] cube, up to 256 MiB of chunks, taken and shuffled by the route's own kernels): the kernel built three
times from scripts/probe/zstd_encode_stages.hip, stopping after the first stage, after the second, and whole; HIP events, the minimum of
--reps runs; one JSON line per layout of scripts/encode_bench.py.

    python scripts/probe/zstd_encode_stages.py --build          # compile the three libraries into scripts/probe/_build (no GPU needed)
    python scripts/probe/zstd_encode_stages.py [--reps 5]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
BUILD = os.path.join(HERE, "_build")
ARMS = {"matches": "1", "matches+sequences": "2", "whole": None}


def lib_path(arm):
    return os.path.join(BUILD, f"zstd_encode_stages_{ARMS[arm] or 'all'}.so")


def build():
    os.makedirs(BUILD, exist_ok=True)
    for arm, stop in ARMS.items():
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off",
               "-I", os.path.join(ROOT, "aggfly_amd", "csrc"), os.path.join(HERE, "zstd_encode_stages.hip"), "-o", lib_path(arm)]
        subprocess.check_call(cmd + ([f"-DAFZE_STOP_AFTER={stop}"] if stop else []))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.build:
        return build()
    import numpy as np
    import torch
    import encode_bench as eb
    from aggfly_amd import codec, hip, io as afio, synth
    libs = {arm: C.CDLL(lib_path(arm)) for arm in ARMS}
    cube = torch.from_numpy(synth.temperature_cube(eb.T, eb.NY, eb.NX, dtype=np.float32, seed=1) + np.float32(273.15)).cuda()
    shape = tuple(cube.shape)
    fill = int(np.array([np.nan], dtype=np.float32).view(np.uint32)[0])
    for chunks in eb.layouts():
        ct = tuple(shape[i] if chunks[k] == -1 else min(chunks[k], shape[i]) for i, k in enumerate(("time", "latitude", "longitude")))
        cb = int(np.prod(ct)) * 4
        idxs = list(np.ndindex(*[-(-s // c) for s, c in zip(shape, ct)]))[:max(1, afio.GPU_ENCODE_BATCH_BYTES // cb)]
        n = len(idxs)
        pl = codec.BloscZstdEncodePlan(n, cb, 4)
        rec = torch.from_numpy(np.concatenate([pl.streams.view(np.uint8), pl.blocks.view(np.uint8)])).cuda()
        chunk_dev = torch.empty(n * cb, dtype=torch.uint8, device="cuda")
        work = torch.empty(pl.work_bytes, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(pl.scratch_bytes, dtype=torch.uint8, device="cuda")
        csize = torch.empty(len(pl.streams), dtype=torch.int32, device="cuda")
        cview = chunk_dev.view(torch.float32)
        for j, idx in enumerate(idxs):
            at = tuple(i * c for i, c in zip(idx, ct))
            box = tuple(min(c, s - o) for c, s, o in zip(ct, shape, at))
            hip.take_box(cube, cview[j * (cb // 4):(j + 1) * (cb // 4)].view(ct), at, box, fill)
        for b0 in range(0, len(pl.blocks), 65535):
            hip.shuffle_blocks(chunk_dev, work, rec[pl.streams.nbytes + b0 * codec.SHUFFLE_BLOCK.itemsize:], min(65535, len(pl.blocks) - b0), pl.max_bsize)
        torch.cuda.synchronize()
        ms = {}
        for arm, lib in libs.items():
            for _ in range(a.reps + 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = lib.probe_zstd_encode_blocks(C.c_void_p(work.data_ptr()), C.c_void_p(rec.data_ptr()), C.c_longlong(len(pl.streams)),
                                                  C.c_void_p(scratch.data_ptr()), C.c_void_p(work[pl.slot_base:].data_ptr()),
                                                  C.c_void_p(csize.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                e1.record()
                e1.synchronize()
                assert rc == 0, rc
                ms[arm] = min(ms.get(arm, 1e30), e0.elapsed_time(e1))
        whole = ms["whole"]
        print(json.dumps({"layout": [chunks[k] for k in ("time", "latitude", "longitude")], "chunks": n, "batch_bytes": n * cb,
                          "blocks": len(pl.streams), "ms": {k: round(v, 3) for k, v in ms.items()},
                          "share": {"matches": round(ms["matches"] / whole, 3),
                                    "sequences": round((ms["matches+sequences"] - ms["matches"]) / whole, 3),
                                    "literals": round((whole - ms["matches+sequences"]) / whole, 3)},
                          "raw_GB_per_s": round(n * cb / whole / 1e6, 2)}), flush=True)


if __name__ == "__main__":
    main()
