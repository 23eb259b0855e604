#!/usr/bin/env python3
"""Multi-band GeoTIFF files into HBM: the device route on files with a band per time step (`_TiffSource.to_device`: chunky pages staged
once and placed by `afhip_tiff_place_bands`, planar pages band by band through `afhip_tiff_place`) against the same values stored as
single-band pages of one multi-page file on the same route — the yardstick —, in the same process, the routes alternating; and the new
kernel alone on one page's decoded bytes against `afhip_tiff_place` on the same values as single-band tiles.

Workload: the BASELINE configs[0] cube (8760 x 104 x 236 float32, synth.temperature_cube, kelvin, no missing cells) written into /dev/shm
as 24 files of 365 bands, by the independent writer of tests/tiff_band_cases.py, in three forms, one after the other:
    chunky_deflate_p3   PlanarConfiguration 1, one 256 x 256 tile, Deflate + predictor 3 (what GDAL and Earth Engine write by default)
    planar_deflate_p3   PlanarConfiguration 2, one 256 x 256 tile per band, Deflate + predictor 3
    chunky_raw          PlanarConfiguration 1, one 256 x 256 tile, uncompressed
and the yardstick `pages_deflate_p3`: one BigTIFF of 8760 single-band pages, one 256 x 256 tile each, Deflate + predictor 3.  Deflate at
zlib level 1 throughout, so that writing stays short.  A synthetic field: smooth in space, and nothing here says how a raster of an
archive would time; no GDAL-written file is among them.

After a warm-up in which every form is compared bit for bit with the yardstick, it times each form's device route and the yardstick,
alternating, and prints min / median / max; the time `tiff.TiffStack` takes to read the directories is part of every route and is
printed on its own.  One JSON line per result.

    python scripts/tiff_bands_ingest_bench.py [--reps 3] [--files 24] [--bands 365]
"""
import argparse
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import hip, synth, tiff  # noqa: E402
from netcdf3_ingest_bench import NX, NY  # noqa: E402
import tiff_band_cases as BC  # noqa: E402
import tiff_cases as TC  # noqa: E402

LON0, LAT0, D = -125.0, 60.0, 0.25
DAY0 = pd.Timestamp("2000-01-01")
TILE = 256


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def stats(v):
    return {"ms_min": round(min(v) * 1e3, 2), "ms_median": round(statistics.median(v) * 1e3, 2), "ms_max": round(max(v) * 1e3, 2)}


def write_pages(path, cube, pool):
    """One BigTIFF of single-band pages, a 256 x 256 tile each (zeros in the padding), Deflate + predictor 3."""
    def stream(t):
        tile = np.zeros((TILE, TILE), dtype=np.float32)
        tile[:NY, :NX] = cube[t]
        return zlib.compress(TC.apply_predictor(tile, 3, "<"), 1)
    streams = list(pool.map(stream, range(len(cube))))
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HHHQ", 43, 8, 0, 0))
        where = []
        for s in streams:
            where.append((f.tell(), len(s)))
            f.write(s)
            f.write(b"\0" * (-f.tell() % 8))
        geo_at = f.tell()
        f.write(struct.pack("<3d", D, D, 0.0) + struct.pack("<6d", 0.0, 0.0, 0.0, LON0, LAT0, 0.0) + struct.pack("<12H", 1, 1, 0, 2, 1024, 0, 1, 2, 1025, 0, 1, 1))
        prev = 8                                                      # where the offset of the next directory is written
        for off, cnt in where:
            here = f.tell()
            ents = [(256, 4, 1, NX), (257, 4, 1, NY), (258, 3, 1, 32), (259, 3, 1, 8), (262, 3, 1, 1), (277, 3, 1, 1), (284, 3, 1, 1), (317, 3, 1, 3),
                    (322, 4, 1, TILE), (323, 4, 1, TILE), (324, 16, 1, off), (325, 4, 1, cnt), (339, 3, 1, 3), (33550, 12, 3, geo_at),
                    (33922, 12, 6, geo_at + 24), (34735, 3, 12, geo_at + 72)]
            f.write(struct.pack("<Q", len(ents)) + b"".join(struct.pack("<HHQQ", tg, ty, c, v) for tg, ty, c, v in ents) + struct.pack("<Q", 0))
            f.seek(prev)
            f.write(struct.pack("<Q", here))
            f.seek(0, 2)
            prev = here + 8 + 20 * len(ents)
    return [path]


def write_form(form, d, cube, bands, pool):
    planar = 2 if form.startswith("planar") else 1
    comp, pred = (1, 1) if form.endswith("raw") else (8, 3)
    geo = TC.geo_tags(lon0=LON0, lat0=LAT0, dx=D, dy=D)

    def one(i):
        page = BC.band_page(cube[i * bands:(i + 1) * bands], planar=planar, compression=comp, predictor=pred, tile=(TILE, TILE), geo=geo, deflate_level=1)
        return BC.write_band_tiff(os.path.join(d, f"year_{i:02d}.tif"), [page], bigtiff=True)
    return list(pool.map(one, range(len(cube) // bands)))


def kernel_alone(cube, bands, reps):
    """`hip.tiff_place_bands` on one page's decoded bytes (one 256 x 256 tile of ``bands`` bands, predictor 3) against `hip.tiff_place` on
    the same values as ``bands`` single-band tiles: HIP events around each launch."""
    padded = np.zeros((bands, TILE, TILE), dtype=np.float32)
    padded[:, :NY, :NX] = cube[:bands]
    chunky = np.frombuffer(BC.apply_band_predictor(np.ascontiguousarray(padded.transpose(1, 2, 0)), 3, "<"), np.uint8)
    single = np.frombuffer(b"".join(TC.apply_predictor(p, 3, "<") for p in padded), np.uint8)
    rec1 = np.zeros(1, dtype=hip.TIFF_SEG)
    rec1["dec_bytes"], rec1["rows"], rec1["pitch"] = len(chunky), TILE, TILE
    recn = np.zeros(bands, dtype=hip.TIFF_SEG)
    recn["dec_bytes"], recn["rows"], recn["pitch"], recn["t"] = TILE * TILE * 4, TILE, TILE, np.arange(bands)
    recn["dec_off"] = np.arange(bands) * TILE * TILE * 4
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    d1, dn, r1, rn = dev(chunky), dev(single), dev(rec1.view(np.uint8)), dev(recn.view(np.uint8))
    out1, outn = torch.zeros((bands, NY, NX), dtype=torch.float32, device="cuda"), torch.zeros((bands, NY, NX), dtype=torch.float32, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    box = (0, 0, NY, NX)
    runs = {"tiff_place_bands": lambda: hip.tiff_place_bands(d1, r1, 1, TILE, bands, 3, False, out1, box, (0, 0, 0), errors),
            "tiff_place": lambda: hip.tiff_place(dn, rn, bands, TILE, 3, False, outn, box, (0, 0, 0), errors)}
    ms = {k: [] for k in runs}
    for i in range(reps + 2):
        for k, fn in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms[k].append(a.elapsed_time(b) / 1e3)
    assert int(errors.item()) == 0 and torch.equal(out1.view(torch.int32), outn.view(torch.int32))
    want = torch.from_numpy(cube[:bands]).cuda()
    assert torch.equal(out1.view(torch.int32), want.view(torch.int32))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"kernel_alone": f"one 256 x 256 tile of {bands} bands, predictor 3, box {NY} x {NX}", "decoded_MiB": round(len(chunky) / (1 << 20), 1),
                      "tiff_place_bands": stats(ms["tiff_place_bands"]), "tiff_place_on_single_band_tiles": stats(ms["tiff_place"]),
                      "bands_over_single": round(med["tiff_place_bands"] / med["tiff_place"], 2), "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--files", type=int, default=24)
    ap.add_argument("--bands", type=int, default=365)
    ap.add_argument("--write-threads", type=int, default=16)
    a = ap.parse_args()
    hip.require_gpu()
    T = a.files * a.bands
    cube = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1, ocean_frac=0.0) + np.float32(273.15)
    tt = list(DAY0 + pd.to_timedelta(np.arange(T), unit="D"))
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    kernel_alone(cube, a.bands, max(a.reps, 5))
    with tempfile.TemporaryDirectory(dir=base) as top, ThreadPoolExecutor(a.write_threads) as pool:
        t0 = time.perf_counter()
        yard = write_pages(os.path.join(top, "pages.tif"), cube, pool)
        print(json.dumps({"form": "pages_deflate_p3", "files": 1, "bytes": os.path.getsize(yard[0]), "written_in_s": round(time.perf_counter() - t0, 1)}), flush=True)
        route = lambda paths: af.dataset_from_path(paths if len(paths) > 1 else paths[0], "t2m", device="cuda", lon_is_360=False, tiff_time=tt).cube()
        ref = route(yard)
        assert torch.equal(ref.view(torch.int32), torch.from_numpy(cube).cuda().view(torch.int32))
        for form in ("chunky_deflate_p3", "planar_deflate_p3", "chunky_raw"):
            d = os.path.join(top, form)
            os.makedirs(d)
            t0 = time.perf_counter()
            paths = write_form(form, d, cube, a.bands, pool)
            wrote = time.perf_counter() - t0
            size = sum(os.path.getsize(p) for p in paths)
            got = route(paths)
            assert got.shape == ref.shape and torch.equal(got.view(torch.int32), ref.view(torch.int32)), form       # bit for bit
            del got
            t = {"bands": [], "pages": [], "directories": [], "pages_directories": []}
            for _ in range(a.reps):
                t["bands"].append(timed(lambda: route(paths))[1])
                t["pages"].append(timed(lambda: route(yard))[1])
                t["directories"].append(timed(lambda: tiff.TiffStack(paths, tt))[1])
                t["pages_directories"].append(timed(lambda: tiff.TiffStack(yard, tt))[1])
            med = {k: statistics.median(v) for k, v in t.items()}
            print(json.dumps({"form": form, "files": len(paths), "bands_per_file": a.bands, "bytes": size, "written_in_s": round(wrote, 1), "steps": T,
                              "device_route": stats(t["bands"]), "of_which_directories": stats(t["directories"]),
                              "single_band_pages_route": stats(t["pages"]), "of_which_its_directories": stats(t["pages_directories"]),
                              "bands_over_pages": round(med["bands"] / med["pages"], 2), "reps": a.reps}), flush=True)
            shutil.rmtree(d)


if __name__ == "__main__":
    main()
