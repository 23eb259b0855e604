#!/usr/bin/env python3
"""GeoTIFF stacks into HBM: the device route (`_TiffSource.to_device`: segments read or decoded by the host team, or LZW streams
decoded in HBM by `afhip_lzw_decode`, then `afhip_tiff_place`) against the NetCDF classic route on the same values in the same process
— the yardstick of DESIGN.md §8 —, against the host route (`TiffStack.read`, then one upload), and the LZW kernel against 16 host
threads at request sizes from 64 MiB up.

Workload: the BASELINE configs[0] cube (8760 x 104 x 236 float32, synth.temperature_cube, kelvin, no missing cells) written into /dev/shm
in five forms, one after the other:
    raw_daily      one uncompressed single-page file per step (strips of 8 rows), the independent writer of tests/tiff_cases.py
    raw_pages      one uncompressed multi-page file
    lzw_p3_strips  one file per step, LZW + predictor 3, strips of 8 rows, WRITTEN BY libtiff through Pillow
    lzw_p3_tiles   one multi-page file, LZW + predictor 3, one 256 x 256 tile per step: the tile's stream is what libtiff writes for a
                   256 x 256 image in one strip (Pillow), set into a tiled directory by this script
    deflate_p3     one file per step, Deflate + predictor 3, strips of 8 rows, libtiff through Pillow
A synthetic field: smooth in space, and nothing here says how a raster of an archive would time.  Without Pillow only the two raw forms
are measured.

After a warm-up in which the routes are compared bit for bit, it times each form's device route (AGGFLY_HIP_GPU_DECODE=0 and, for the
LZW forms, =1), its host route and the classic file, alternating, and prints min / median / max; the time `tiff.TiffStack` takes to read
the directories is part of every TIFF route and is printed on its own.  Then the LZW sweep: the first steps of the LZW forms up to
request sizes of 64, 128, 256, 512 MiB and the whole cube, decode in HBM against the host team — the rule of
`io.GPU_DECODE_AUTO_BYTES_DEFLATE`: the smallest size from which the GPU median is <= 0.9 x the host minimum on EVERY layout, else None.
One JSON line per result.

    python scripts/tiff_ingest_bench.py [--reps 3] [--steps 8760]
"""
import argparse
import io as pyio
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import hip, synth, tiff  # noqa: E402
from netcdf3_ingest_bench import NX, NY, write_classic  # noqa: E402
import tiff_cases as TC  # noqa: E402

LON0, LAT0, D = -125.0, 60.0, 0.25
DAY0 = pd.Timestamp("2000-01-01")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stats(v):
    return {"ms_min": round(min(v) * 1e3, 2), "ms_median": round(statistics.median(v) * 1e3, 2), "ms_max": round(max(v) * 1e3, 2)}


def name_of(d, t):
    return os.path.join(d, f"t2m_{(DAY0 + pd.Timedelta(days=t)).strftime('%Y%m%d')}.tif")


def pillow_tags(predictor, rows_per_strip):
    from PIL import TiffImagePlugin
    ifd = TiffImagePlugin.ImageFileDirectory_v2()
    ifd[33550] = (D, D, 0.0)
    ifd[33922] = (0.0, 0.0, 0.0, LON0, LAT0, 0.0)
    ifd[34735] = (1, 1, 0, 2, 1024, 0, 1, 2, 1025, 0, 1, 1)
    ifd[317] = predictor
    ifd[278] = rows_per_strip
    return ifd


def write_form(form, d, cube):
    """-> (paths, tiff_time or None)."""
    T = len(cube)
    geo = TC.geo_tags(lon0=LON0, lat0=LAT0, dx=D, dy=D)
    if form == "raw_daily":
        return [TC.write_tiff(name_of(d, t), [TC.page(cube[t], rows_per_strip=8, geo=geo)]) for t in range(T)], None
    if form == "raw_pages":
        # (the pages share one geo dictionary; the writer lays out segment data, then each directory)
        return [TC.write_tiff(os.path.join(d, "pages.tif"), [TC.page(cube[t], rows_per_strip=8, geo=geo) for t in range(T)], bigtiff=True)], \
            list(DAY0 + pd.to_timedelta(np.arange(T), unit="D"))
    from PIL import Image
    if form in ("lzw_p3_strips", "deflate_p3"):
        comp = "tiff_lzw" if form == "lzw_p3_strips" else "tiff_adobe_deflate"
        tags = pillow_tags(3, 8)
        paths = []
        for t in range(T):
            Image.fromarray(cube[t]).save(name_of(d, t), compression=comp, tiffinfo=tags)
            paths.append(name_of(d, t))
        return paths, None
    # lzw_p3_tiles: one 256 x 256 tile per step; libtiff compresses the padded tile as a one-strip image, the stream is lifted out of it
    tags = pillow_tags(3, 256)
    tile = np.zeros((256, 256), dtype=np.float32)
    path = os.path.join(d, "tiles.tif")
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HHHQ", 43, 8, 0, 0))
        streams = []
        for t in range(T):
            tile[:NY, :NX] = cube[t]
            mem = pyio.BytesIO()
            Image.fromarray(tile).save(mem, format="TIFF", compression="tiff_lzw", tiffinfo=tags)
            raw = mem.getvalue()                                      # (a little-endian classic file: where its one strip lies)
            first = struct.unpack("<I", raw[4:8])[0]
            n = struct.unpack("<H", raw[first:first + 2])[0]
            ent = {struct.unpack("<H", raw[first + 2 + 12 * i:first + 4 + 12 * i])[0]: struct.unpack("<II", raw[first + 6 + 12 * i:first + 14 + 12 * i]) for i in range(n)}
            assert raw[:4] == b"II*\0" and ent[273][0] == 1 and ent[279][0] == 1, "one strip was expected"
            ent = {k: v[1] for k, v in ent.items()}
            streams.append((f.tell(), ent[279]))
            f.write(raw[ent[273]:ent[273] + ent[279]])
            f.write(b"\0" * (-f.tell() % 8))
        gkeys = struct.pack("<12H", 1, 1, 0, 2, 1024, 0, 1, 2, 1025, 0, 1, 1)
        scale, tie = struct.pack("<3d", D, D, 0.0), struct.pack("<6d", 0.0, 0.0, 0.0, LON0, LAT0, 0.0)
        geo_at = f.tell()
        f.write(scale + tie + gkeys)
        prev = 8                                                      # where the offset of the next directory is written
        for t, (off, cnt) in enumerate(streams):
            here = f.tell()
            ents = [(256, 4, 1, NX), (257, 4, 1, NY), (258, 3, 1, 32), (259, 3, 1, 5), (262, 3, 1, 1), (277, 3, 1, 1), (284, 3, 1, 1), (317, 3, 1, 3),
                    (322, 4, 1, 256), (323, 4, 1, 256), (324, 16, 1, off), (325, 4, 1, cnt), (339, 3, 1, 3), (33550, 12, 3, geo_at),
                    (33922, 12, 6, geo_at + 24), (34735, 3, 12, geo_at + 72)]
            body = struct.pack("<Q", len(ents)) + b"".join(struct.pack("<HHQQ", tg, ty, c, v) for tg, ty, c, v in ents) + struct.pack("<Q", 0)
            f.write(body)
            f.seek(prev)
            f.write(struct.pack("<Q", here))
            f.seek(0, 2)
            prev = here + 8 + 20 * len(ents)
    return [path], list(DAY0 + pd.to_timedelta(np.arange(T), unit="D"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8760)
    ap.add_argument("--host-threads", type=int, default=16)
    a = ap.parse_args()
    hip.require_gpu()
    try:
        import PIL  # noqa: F401
        forms = ["raw_daily", "raw_pages", "lzw_p3_strips", "lzw_p3_tiles", "deflate_p3"]
    except ImportError:
        forms = ["raw_daily", "raw_pages"]
        print(json.dumps({"note": "Pillow is not installed: the LZW and Deflate forms are not written"}), flush=True)
    T = a.steps
    cube = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1, ocean_frac=0.0) + np.float32(273.15)
    lat, lon = (LAT0 - D * (np.arange(NY) + 0.5)), (LON0 + D * (np.arange(NX) + 0.5))
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    step_bytes = NY * NX * 4
    sweep, verdict = {}, {}
    with tempfile.TemporaryDirectory(dir=base) as top:
        classic = os.path.join(top, "cube.nc")
        write_classic(classic, (876576 + np.arange(T)).astype(np.int32), lat.astype(np.float32), lon.astype(np.float32), cube, {"units": "K"})
        classic_route = lambda: af.dataset_from_path(classic, "t2m", device="cuda", lon_is_360=False).cube()
        ref = classic_route()
        for form in forms:
            d = os.path.join(top, form)
            os.makedirs(d)
            t0 = time.perf_counter()
            paths, tt = write_form(form, d, cube)
            wrote = time.perf_counter() - t0
            size = sum(os.path.getsize(p) for p in paths)

            def device_route(n=T, mode="0"):
                os.environ["AGGFLY_HIP_GPU_DECODE"] = mode
                p, t_ = (paths[:n], tt) if len(paths) > 1 else (paths, tt)
                ds = af.dataset_from_path(p if len(p) > 1 else p[0], "t2m", device="cuda", lon_is_360=False, tiff_time=t_,
                                          **({"time_window": (0, n)} if n < T and len(paths) == 1 else {}))
                return ds.cube()

            def host_route():
                st = tiff.TiffStack(paths, tt)
                return torch.from_numpy(st.read(threads=a.host_threads)).to("cuda")

            lzw = form.startswith("lzw")
            got = device_route()
            assert got.shape == ref.shape and torch.equal(got.view(torch.int32), ref.view(torch.int32)), form       # bit for bit, every route
            assert torch.equal(host_route().view(torch.int32), ref.view(torch.int32)), form
            if lzw:
                assert torch.equal(device_route(mode="1").view(torch.int32), ref.view(torch.int32)), form
            del got
            t = {"device": [], "device_lzw_in_hbm": [], "host": [], "classic": [], "directories": []}
            for _ in range(a.reps):
                t["device"].append(timed(device_route)[1])
                if lzw:
                    t["device_lzw_in_hbm"].append(timed(lambda: device_route(mode="1"))[1])
                t["classic"].append(timed(classic_route)[1])
                t["host"].append(timed(host_route)[1])
                t["directories"].append(timed(lambda: tiff.TiffStack(paths, tt))[1])
            med = {k: statistics.median(v) for k, v in t.items() if v}
            print(json.dumps({"form": form, "files": len(paths), "bytes": size, "written_in_s": round(wrote, 1), "steps": T,
                              "device_route": stats(t["device"]), **({"device_route_lzw_in_hbm": stats(t["device_lzw_in_hbm"])} if lzw else {}),
                              "classic_route": stats(t["classic"]), f"host_route_{a.host_threads}_threads_plus_upload": stats(t["host"]),
                              "of_which_directories": stats(t["directories"]), "device_over_classic": round(med["device"] / med["classic"], 2),
                              "device_minus_directories_over_classic": round((med["device"] - med["directories"]) / med["classic"], 2),
                              "device_over_host": round(med["device"] / med["host"], 3), "reps": a.reps}), flush=True)
            if lzw:
                # the sweep: the LZW streams decoded in HBM against the host team, at request sizes from 64 MiB up
                rows = []
                for mib in (64, 128, 256, 512, None):
                    n = T if mib is None else min(T, (mib << 20) // step_bytes)
                    g, h = [], []
                    for _ in range(a.reps):
                        h.append(timed(lambda: device_route(n, "0"))[1])
                        g.append(timed(lambda: device_route(n, "1"))[1])
                    rows.append({"request_MiB": round(n * step_bytes / (1 << 20)), "steps": n, "host_team": stats(h), "in_hbm": stats(g),
                                 "gpu_median_over_host_min": round(statistics.median(g) / min(h), 2)})
                    if n == T:
                        break
                sweep[form] = rows
                print(json.dumps({"lzw_sweep": form, "rows": rows}), flush=True)
            shutil.rmtree(d)
    if sweep:
        sizes = sorted({r["request_MiB"] for rows in sweep.values() for r in rows})
        ok = [s for s in sizes if all(any(r["request_MiB"] >= s for r in rows) and all(r["gpu_median_over_host_min"] <= 0.9 for r in rows if r["request_MiB"] >= s)
                                      for rows in sweep.values())]
        verdict = {"GPU_DECODE_AUTO_BYTES_LZW": f"{ok[0]} MiB" if ok else None, "rule": "GPU median <= 0.9 x host minimum on every layout from that size on"}
        print(json.dumps(verdict), flush=True)


if __name__ == "__main__":
    main()
