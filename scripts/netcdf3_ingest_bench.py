#!/usr/bin/env python3
"""NetCDF classic files into HBM: the streaming route (`pread` into page-locked slabs, the bytes over PCIe as stored, one
kernel that swaps and places them: `afhip_place_box_swapped`) against the host route it replaces (`scipy.io.netcdf_file`, byte swap
and CF unpack on one host thread, then `Dataset.to_device()`) and against a bare page-locked upload of the same bytes.

Workload: the BASELINE configs[0] cube (8760 x 104 x 236, synth.temperature_cube) written into /dev/shm as a CDF-2 file the way
ERA5 is served — a record dimension `time`, its int32 coordinate and one data variable, so every step is one run of the file —
in two storages (int16 with scale_factor / add_offset / _FillValue; float32) and two layouts (the grid itself; the same box
clipped by `georegions=` out of a grid four times as large, 208 x 472).  Requests of about 1 MB, 64 MB and the whole cube
(`time_window=`).  In one process, after a warm-up and alternating between them, it times

  (a) `dataset_from_path(device="cuda")`, the streaming route;
  (b) the same call with the header reader switched off, i.e. the route the parent commit took, its `to_device()` included
      (big-endian float storage cannot be uploaded by it as it is: there the byte order is converted on the host first, and the
      line says so);
  (c) one `copy_` of the request's stored bytes from a page-locked buffer;

then, for the whole cube, the host side of (a) alone — header and coordinates; the `pread`s into the page-locked slabs with nothing
uploaded — and, with device events, the placement kernel alone on one slab of each layout.  One JSON line per result.

    python scripts/netcdf3_ingest_bench.py [--reps 5] [--steps 8760]
"""
import argparse
import json
import os
import statistics
import struct
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
SF, AO, FILL = 0.0018311105046321, 283.64, -32767


def write_classic(path, hours, lat, lon, data, attrs):
    """A CDF-2 file: dimensions time (record), latitude, longitude; float32 coordinates, int32 hours, the variable t2m."""
    def pad(b):
        return b + b"\0" * (-len(b) % 4)

    def name(s):
        return struct.pack(">I", len(s)) + pad(s.encode())

    def att(a):
        out = struct.pack(">II", 0x0C, len(a)) if a else struct.pack(">II", 0, 0)
        for k, v in a.items():
            if isinstance(v, str):
                out += name(k) + struct.pack(">II", 2, len(v)) + pad(v.encode())
            elif isinstance(v, float):
                out += name(k) + struct.pack(">II", 6, 1) + struct.pack(">d", v)
            else:
                out += name(k) + struct.pack(">II", 3, 1) + pad(struct.pack(">h", v))
        return out

    T, ny, nx = data.shape
    code = {"i2": 3, "f4": 5}[data.dtype.str[1:]]
    plane = ny * nx * data.dtype.itemsize
    variables = [("latitude", [1], {"units": "degrees_north"}, 5, ny * 4), ("longitude", [2], {"units": "degrees_east"}, 5, nx * 4),
                 ("time", [0], {"units": "hours since 1900-01-01 00:00:00.0", "calendar": "gregorian"}, 4, 4), ("t2m", [0, 1, 2], attrs, code, plane)]

    def header(begins):
        h = b"CDF\x02" + struct.pack(">I", T) + struct.pack(">II", 0x0A, 3) + name("time") + struct.pack(">I", 0)
        h += name("latitude") + struct.pack(">I", ny) + name("longitude") + struct.pack(">I", nx) + struct.pack(">II", 0, 0)
        h += struct.pack(">II", 0x0B, len(variables))
        for (nm, ids, a, c, size), b in zip(variables, begins):
            h += name(nm) + struct.pack(">I", len(ids)) + b"".join(struct.pack(">I", i) for i in ids) + att(a)
            h += struct.pack(">II", c, min(size + (-size % 4), 0xFFFFFFFF)) + struct.pack(">Q", b)
        return h

    h0 = len(header([0] * 4))
    begins = [h0, h0 + ny * 4, h0 + ny * 4 + nx * 4, h0 + ny * 4 + nx * 4 + 4]
    hours_be, be = hours.astype(">i4"), data.dtype.newbyteorder(">")
    tail = b"\0" * (-plane % 4)
    with open(path, "wb") as f:
        f.write(header(begins) + lat.astype(">f4").tobytes() + lon.astype(">f4").tobytes())
        for t in range(T):
            f.write(hours_be[t:t + 1].tobytes())
            f.write(data[t].astype(be).tobytes())
            f.write(tail)


def cubes(T):
    """The cube as float32 kelvin with NaN over the ocean, and as the int16 a packer would store."""
    f32 = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1, ocean_frac=0.1) + np.float32(273.15)
    i16 = np.where(np.isnan(f32), FILL, np.clip(np.round((f32.astype(np.float64) - AO) / SF), -32766, 32767)).astype(np.int16)
    return f32, i16


def embed(a, fill):
    """``a`` as the middle box of a grid four times as large."""
    out = np.full((a.shape[0], 2 * NY, 2 * NX), fill, dtype=a.dtype)
    out[:, NY // 2:NY // 2 + NY, NX // 2:NX // 2 + NX] = a
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8760)
    a = ap.parse_args()
    hip.require_gpu()
    T = a.steps
    hours = (876576 + np.arange(T)).astype(np.int32)
    lat, lon = (60 - 0.25 * np.arange(NY)).astype(np.float32), (235 + 0.25 * np.arange(NX)).astype(np.float32)
    lat4 = (60 + 0.25 * (NY // 2) - 0.25 * np.arange(2 * NY)).astype(np.float32)
    lon4 = (235 - 0.25 * (NX // 2) + 0.25 * np.arange(2 * NX)).astype(np.float32)
    box = af.GeoRegions(pd.DataFrame({"geoid": ["box"], "minx": [float(lon[0]) - 360], "maxx": [float(lon[-1]) - 360],
                                      "miny": [float(lat[-1])], "maxy": [float(lat[0])]}))
    packed_attrs = {"scale_factor": SF, "add_offset": AO, "_FillValue": FILL, "units": "K"}
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=base) as d:
        f32, i16 = cubes(T)
        files = {}
        for storage, arr, attrs, fill in (("int16", i16, packed_attrs, FILL), ("float32", f32, {"units": "K"}, np.float32("nan"))):
            files[storage, "grid"] = os.path.join(d, f"{storage}_grid.nc")
            write_classic(files[storage, "grid"], hours, lat, lon, arr, attrs)
            files[storage, "box_of_4x"] = os.path.join(d, f"{storage}_4x.nc")
            write_classic(files[storage, "box_of_4x"], hours, lat4, lon4, embed(arr, fill), attrs)
        del f32, i16

        real_source = afio._netcdf3_source

        def new_route(path, kw):
            ds = af.dataset_from_path(path, "t2m", device="cuda", **kw)
            assert ds.cube().is_cuda
            return ds

        def old_route(path, kw, note):
            afio._netcdf3_source = lambda *a_, **k_: None            # the header reader declines: the parent commit's code path
            try:
                try:
                    return af.dataset_from_path(path, "t2m", device="cuda", **kw)
                except (ValueError, TypeError) as e:                 # big-endian floats: torch takes native byte order only
                    note.append(f"to_device() raises ({type(e).__name__}): byte order converted on the host")
                    ds = af.dataset_from_path(path, "t2m", **kw)
                    c = ds.cube()
                    return torch.from_numpy(c.astype(c.dtype.newbyteorder("="))).to("cuda")
            finally:
                afio._netcdf3_source = real_source

        for (storage, layout), path in files.items():
            isz = 2 if storage == "int16" else 4
            step = NY * NX * isz                                      # stored bytes of the request per step
            geo = {"georegions": box} if layout == "box_of_4x" else {}
            for label, n in (("1MB", max(1, round((1 << 20) / step))), ("64MB", min(T, round((64 << 20) / step))), ("whole", T)):
                kw = dict(geo, time_window=(0, n))
                nbytes = n * step
                pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
                dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
                note = []
                want = new_route(path, kw).cube()                     # warm-up, and the two routes agree
                got = old_route(path, kw, note)
                got = got.cube() if hasattr(got, "cube") else got
                got = got if torch.is_tensor(got) else torch.from_numpy(np.ascontiguousarray(got)).cuda()
                assert got.shape == want.shape and torch.equal(torch.nan_to_num(got, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), (storage, layout, label)
                assert bool((torch.isnan(got) == torch.isnan(want)).all())
                del got, want
                dev.copy_(pinned, non_blocking=True)
                t = {"a": [], "b": [], "c": []}
                for _ in range(a.reps):                               # alternating
                    t["a"].append(timed(lambda: new_route(path, kw))[1])
                    t["b"].append(timed(lambda: old_route(path, kw, []))[1])
                    t["c"].append(timed(lambda: dev.copy_(pinned, non_blocking=True))[1])
                med = {k: statistics.median(v) for k, v in t.items()}
                print(json.dumps({"storage": storage, "layout": layout, "request": label, "steps": n, "stored_bytes": nbytes,
                                  "new_ms_median": round(med["a"] * 1e3, 3), "new_ms_min": round(min(t["a"]) * 1e3, 3),
                                  "host_ms_median": round(med["b"] * 1e3, 3), "host_ms_min": round(min(t["b"]) * 1e3, 3),
                                  "h2d_ms_median": round(med["c"] * 1e3, 3), "new_GB_per_s": round(nbytes / med["a"] / 1e9, 2),
                                  "h2d_GB_per_s": round(nbytes / med["c"] / 1e9, 2), "new_over_host": round(med["a"] / med["b"], 4),
                                  "new_over_h2d": round(med["a"] / med["c"], 3), "reps": a.reps, "note": "; ".join(note[:1])}), flush=True)
                del pinned, dev

        # where the route's time goes on the host: header + coordinates, and the reads into the page-locked slabs with nothing uploaded
        real_stream = afio.stream_to_device

        def reads_only(T_, spatial, np_dtype, read_slab, slab_steps, device="cuda", post=None, out_dtype=None, wire_dtype=None, place=None,
                       stage_step_bytes=None):
            slab_steps = max(1, min(slab_steps, T_))
            buf = afio._pinned_stage(slab_steps * stage_step_bytes, 1, device)[0].numpy()
            for k0 in range(0, T_, slab_steps):
                k1 = min(T_, k0 + slab_steps)
                read_slab(k0, k1, buf[:(k1 - k0) * stage_step_bytes])
            return torch.empty((0,) + tuple(spatial), device=device)

        def head_of(path):
            src = afio._netcdf3_source(path, "t2m")
            return src, src.coords()

        for (storage, layout), path in files.items():
            geo = box if layout == "box_of_4x" else None
            head, reads = [], []
            for i in range(a.reps + 1):
                (src, _), s0 = timed(lambda: head_of(path))
                afio.stream_to_device = reads_only
                try:
                    _, s1 = timed(lambda: afio._part_to_device(src, "cuda", ("longitude", "latitude"), "time", georegions=geo))
                finally:
                    afio.stream_to_device = real_stream
                if i:
                    head.append(s0)
                    reads.append(s1 - s0)                             # (the part reads the coordinates once more)
            nbytes = T * NY * NX * (2 if storage == "int16" else 4)
            print(json.dumps({"parts": "host side", "storage": storage, "layout": layout, "request": "whole",
                              "header_and_coordinates_ms_median": round(statistics.median(head) * 1e3, 3),
                              "preads_into_pinned_slabs_ms_median": round(statistics.median(reads) * 1e3, 3),
                              "preads_GB_per_s": round(nbytes / statistics.median(reads) / 1e9, 2)}), flush=True)

        # the kernel alone, one slab (128 MB of the file's rows) of each layout and element size
        for es, tdt in ((2, torch.int16), (4, torch.float32), (8, torch.float64)):
            for layout, (by, bx, sx) in (("grid", (NY, NX, 0)), ("box_of_4x", (NY, 2 * NX, NX // 2))):
                m = max(1, (128 << 20) // (by * bx * es))
                blk = torch.randint(-30000, 30000, (m, by, bx), dtype=torch.int16, device="cuda").to(tdt)
                out = torch.empty((m, NY, NX), dtype=tdt, device="cuda")
                ms = []
                for i in range(25):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    hip.place_box_swapped(blk, out, (0, 0, sx, m, NY, NX), (0, 0, 0))
                    e1.record()
                    e1.synchronize()
                    if i >= 5:
                        ms.append(e0.elapsed_time(e1))
                moved = 2 * m * NY * NX * es                          # read once, written once
                print(json.dumps({"kernel": "k_place_box_swapped", "elem_size": es, "layout": layout, "slab_steps": m,
                                  "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                                  "moved_GB_per_s": round(moved / statistics.median(ms) / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
