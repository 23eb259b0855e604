#!/usr/bin/env python3
"""GRIB files into HBM: the device route (`pread` of the packed bits into page-locked slabs, the bytes over PCIe as stored, one
kernel that extracts, scales and places them: `afhip_grib_unpack`) against the host route (`grib.GribFile.read`, vectorised numpy,
then one upload), a bare page-locked upload of the same packed bytes, and the NetCDF classic route on the same integers stored as
int16 in a CDF-2 file — the yardstick: the same bytes per value, the same reader team, a kernel that does strictly less.

Workload: the BASELINE configs[0] cube (8760 x 104 x 236, synth.temperature_cube) written into /dev/shm as 16-bit edition-1
messages, one per hour, three times: the grid itself; the same box clipped by `georegions=` out of a grid four times as large
(208 x 472); and the grid with a bitmap that leaves out a third of the points.  In one process, after a warm-up and alternating
between them, it times the four — the device route twice: the first open of a file, which walks its headers, and a later one, which finds
the index kept by `grib.open_index` — and prints min / median / max; then, with device events, the kernel alone on one slab: GB/s of staged
bytes for 16-bit and 12-bit fields, with and without a bitmap.  One JSON line per result.

    python scripts/grib_ingest_bench.py [--reps 5] [--steps 8760]
"""
import argparse
import datetime as dt
import json
import math
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import grib, hip, synth  # noqa: E402
from netcdf3_ingest_bench import write_classic  # noqa: E402

NY, NX = 104, 236
E, R = -9, 200.0                      # 16 bits of 2^-9 K from 200 K: 200 .. 328 K
START = dt.datetime(2000, 1, 1)


def _sm(v, nbytes):
    return (abs(v) | ((1 << (8 * nbytes - 1)) if v < 0 else 0)).to_bytes(nbytes, "big")


def _ibm(x):
    if x == 0:
        return bytes(4)
    a = max(0, min(127, math.floor(math.log(abs(x), 16)) + 65))
    b = round(abs(x) / 16.0 ** (a - 64) * 2 ** 24)
    assert 0 < b < (1 << 24) and math.ldexp(b, 4 * (a - 64) - 24) == abs(x), x
    return ((((0x80 | a) if x < 0 else a) << 24) | b).to_bytes(4, "big")


def write_grib1(path, X, lat, lon, have=None):
    """One edition-1 message per step of the uint16 integers ``X`` (T, ny, nx), parameter 167 of table 128, hourly from START;
    ``have`` (T, ny, nx) bool: a bitmap, and only the values of its points are packed."""
    T, ny, nx = X.shape
    md = lambda deg: int(round(float(deg) * 1000))
    gds = (b"\x00\x00\x20\x00\xff\x00" + nx.to_bytes(2, "big") + ny.to_bytes(2, "big") + _sm(md(lat[0]), 3) + _sm(md(lon[0]), 3) + b"\x80"
           + _sm(md(lat[-1]), 3) + _sm(md(lon[-1]), 3) + (250).to_bytes(2, "big") * 2 + b"\x00" + bytes(4))
    with open(path, "wb") as f:
        for t in range(T):
            when = START + dt.timedelta(hours=t)
            pds = (b"\x00\x00\x1c\x80\x62\x91\xff" + bytes([0xC0 if have is not None else 0x80]) + b"\xa7\x01\x00\x00"
                   + bytes([(when.year - 1) % 100 + 1, when.month, when.day, when.hour, 0, 1, 0, 0, 0, 0, 0, 0, (when.year - 1) // 100 + 1, 0]) + _sm(0, 2))
            bms = b""
            if have is not None:
                bits = np.packbits(have[t].ravel()).tobytes()
                bits += b"\x00" * (len(bits) % 2)
                bms = (6 + len(bits)).to_bytes(3, "big") + bytes([len(bits) * 8 - ny * nx]) + b"\x00\x00" + bits
            vals = X[t].ravel() if have is None else X[t].ravel()[have[t].ravel()]
            data = vals.astype(">u2").tobytes()
            data += b"\x00" * ((11 + len(data)) % 2)
            bds = (11 + len(data)).to_bytes(3, "big") + bytes([len(data) * 8 - vals.size * 16]) + _sm(E, 2) + _ibm(R) + b"\x10" + data
            body = pds + gds + bms + bds + b"7777"
            f.write(b"GRIB" + (8 + len(body)).to_bytes(3, "big") + b"\x01" + body)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stats(v):
    return {"ms_min": round(min(v) * 1e3, 3), "ms_median": round(statistics.median(v) * 1e3, 3), "ms_max": round(max(v) * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8760)
    a = ap.parse_args()
    hip.require_gpu()
    T = a.steps
    lat, lon = 60 - 0.25 * np.arange(NY), 235 + 0.25 * np.arange(NX)
    lat4, lon4 = 60 + 0.25 * (NY // 2) - 0.25 * np.arange(2 * NY), 235 - 0.25 * (NX // 2) + 0.25 * np.arange(2 * NX)
    box = af.GeoRegions(pd.DataFrame({"geoid": ["box"], "minx": [float(lon[0]) - 360], "maxx": [float(lon[-1]) - 360],
                                      "miny": [float(lat[-1])], "maxy": [float(lat[0])]}))
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    with tempfile.TemporaryDirectory(dir=base) as d:
        f32 = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1, ocean_frac=0.33) + np.float32(273.15)
        have = ~np.isnan(f32)
        X = np.clip(np.round((np.nan_to_num(f32, nan=280.0).astype(np.float64) - R) / 2.0 ** E), 0, 65535).astype(np.uint16)
        del f32
        X4 = np.zeros((T, 2 * NY, 2 * NX), dtype=np.uint16)
        X4[:, NY // 2:NY // 2 + NY, NX // 2:NX // 2 + NX] = X
        files = {"grid": (os.path.join(d, "grid.grib"), {}), "box_of_4x": (os.path.join(d, "4x.grib"), {"georegions": box}),
                 "bitmap_third_missing": (os.path.join(d, "bitmap.grib"), {})}
        write_grib1(files["grid"][0], X, lat, lon)
        write_grib1(files["box_of_4x"][0], X4, lat4, lon4)
        write_grib1(files["bitmap_third_missing"][0], X, lat, lon, have)
        # the yardstick: the same integers as int16 in CDF-2 files (X - 32768, the offset folded into add_offset)
        hours = (876576 + np.arange(T)).astype(np.int32)
        attrs = {"scale_factor": 2.0 ** E, "add_offset": R + 32768 * 2.0 ** E, "units": "K"}
        classic = {"grid": os.path.join(d, "grid.nc"), "box_of_4x": os.path.join(d, "4x.nc")}
        write_classic(classic["grid"], hours, lat.astype(np.float32), lon.astype(np.float32), (X.astype(np.int32) - 32768).astype(np.int16), attrs)
        write_classic(classic["box_of_4x"], hours, lat4.astype(np.float32), lon4.astype(np.float32), (X4.astype(np.int32) - 32768).astype(np.int16), attrs)
        missing = 1.0 - float(have.mean())
        del X4

        def device_route(path, kw):
            ds = af.dataset_from_path(path, "t2m", device="cuda", **kw)
            assert ds.cube().is_cuda
            return ds.cube()

        def host_route(path, kw):
            return torch.from_numpy(np.ascontiguousarray(af.dataset_from_path(path, "t2m", **kw).cube())).to("cuda")

        for layout, (path, kw) in files.items():
            packed = int((have.sum() if layout == "bitmap_third_missing" else T * NY * NX)) * 2       # the packed bytes of the request
            pinned = torch.empty(packed, dtype=torch.uint8, pin_memory=True)
            dev = torch.empty(packed, dtype=torch.uint8, device="cuda")
            want, got = device_route(path, kw), host_route(path, kw)                     # warm-up, and the two routes agree bit for bit
            assert got.shape == want.shape == (T, NY, NX) and torch.equal(got.view(torch.int32), want.view(torch.int32)), layout
            if layout in classic:                                                        # ... and the classic file holds the same field
                ref = device_route(classic[layout], kw)
                assert float((ref - want).abs().max()) < 1e-3, layout
                del ref
            del want, got
            dev.copy_(pinned, non_blocking=True)
            t = {"device": [], "device_first": [], "host": [], "h2d": [], "classic": []}
            for _ in range(a.reps):                                                      # alternating
                grib._INDEX_CACHE.clear()                                                # the first open of a file walks its headers ...
                t["device_first"].append(timed(lambda: device_route(path, kw))[1])
                t["device"].append(timed(lambda: device_route(path, kw))[1])            # ... every later one finds the index (`grib.open_index`)
                t["host"].append(timed(lambda: host_route(path, kw))[1])
                t["h2d"].append(timed(lambda: dev.copy_(pinned, non_blocking=True))[1])
                if layout in classic:
                    t["classic"].append(timed(lambda: device_route(classic[layout], kw))[1])
            med = {k: statistics.median(v) for k, v in t.items() if v}
            line = {"layout": layout, "steps": T, "packed_bytes": packed, "missing_fraction": round(missing, 3) if "bitmap" in layout else 0.0,
                    "device_route": stats(t["device"]), "device_route_first_open": stats(t["device_first"]), "host_route_plus_upload": stats(t["host"]), "bare_pinned_upload": stats(t["h2d"]),
                    "device_GB_per_s_of_packed_bytes": round(packed / med["device"] / 1e9, 2), "device_over_host": round(med["device"] / med["host"], 4),
                    "device_over_h2d": round(med["device"] / med["h2d"], 3), "reps": a.reps}
            if t["classic"]:
                line["classic_int16_route"] = stats(t["classic"])
                line["device_over_classic"] = round(med["device"] / med["classic"], 3)
            print(json.dumps(line), flush=True)
            del pinned, dev

        # where the device route's time goes on the host: the index (headers only) and the choice of the variable
        idx, sel = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            gf = grib.GribFile(files["grid"][0])
            t1 = time.perf_counter()
            gf.select("t2m").coords()
            idx.append(t1 - t0)
            sel.append(time.perf_counter() - t1)
        print(json.dumps({"parts": "host side", "layout": "grid", "messages": T, "index_headers": stats(idx), "select_and_coordinates": stats(sel)}), flush=True)

    # the kernel alone: one slab of fields of the grid, random bits, by device events; GB/s of STAGED bytes (the cube written is 4 bytes a value)
    rng = np.random.default_rng(0)
    npts = NY * NX
    for nbits in (16, 12):
        for with_map in (False, True):
            n_vals = npts if not with_map else int(round(npts * 2 / 3))
            map_bytes = ((npts + 7) // 8 + 3) // 4 * 4 if with_map else 0
            data_bytes = (n_vals * nbits + 7) // 8
            step = map_bytes + (data_bytes + 3) // 4 * 4
            m = max(1, (64 << 20) // step)
            stage = rng.integers(0, 256, size=m * step, dtype=np.uint8)
            if with_map:
                bits = np.zeros(npts, dtype=np.uint8)
                bits[rng.permutation(npts)[:n_vals]] = 1
                stage.reshape(m, step)[:, :(npts + 7) // 8] = np.packbits(bits)
            rec = np.zeros(m, dtype=hip.GRIB_STEP)
            rec["bitmap_off"] = np.arange(m) * step if with_map else -1
            rec["data_off"], rec["data_bytes"], rec["nbits"] = np.arange(m) * step + map_bytes, data_bytes, nbits
            rec["R"], rec["s"], rec["d"] = R, 2.0 ** E, 1.0
            stage_d, rec_d = torch.from_numpy(stage).cuda(), torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
            cube = torch.empty((m, NY, NX), dtype=torch.float32, device="cuda")
            rank = torch.empty(hip.grib_rank_bytes(m, npts), dtype=torch.uint8, device="cuda")
            errors = torch.zeros(1, dtype=torch.int32, device="cuda")
            ms = []
            for i in range(25):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hip.grib_unpack(stage_d, rec_d, m, (NY, NX), (0, 0, NY, NX), cube, (0, 0, 0), rank, errors)
                e1.record()
                e1.synchronize()
                if i >= 5:
                    ms.append(e0.elapsed_time(e1))
            assert int(errors.item()) == 0
            print(json.dumps({"kernel": "k_grib_rank + k_grib_unpack", "nbits": nbits, "bitmap": with_map, "slab_steps": m, "staged_bytes": m * step,
                              "ms_min": round(min(ms), 4), "ms_median": round(statistics.median(ms), 4), "ms_max": round(max(ms), 4),
                              "staged_GB_per_s": round(m * step / statistics.median(ms) / 1e6, 1),
                              "staged_plus_written_GB_per_s": round((m * step + cube.numel() * 4) / statistics.median(ms) / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
