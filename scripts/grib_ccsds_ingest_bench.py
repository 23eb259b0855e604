#!/usr/bin/env python3
"""CCSDS-packed GRIB2 files (template 5.42) into HBM: the device route (`afhip_grib_unpack_ccsds`: boundary walk, RSI decode, place pass)
against the same integers in 16-bit simple packing on the existing device route — the yardstick of DESIGN.md §8 —, against the host
route on 16 threads (`grib.GribFile.read` over 16 runs of steps, then one upload), and its kernels one by one.

Workload: the BASELINE configs[0] cube (8760 x 104 x 236, synth.temperature_cube) as 16-bit integers of 2^-9 K from 200 K, written into
/dev/shm twice: as edition-1 messages in simple packing (scripts/grib_ingest_bench.py's writer) and as edition-2 messages in template
5.42 at ecCodes' defaults (block size 32, rsi 128, flags 14: preprocessor on), section 7 ENCODED BY libaec through ctypes — the library
ecCodes calls.  A synthetic field: smooth along a row, and nothing here says how a field of an archive would time.

In one process, after a warm-up in which the routes are compared bit for bit, and alternating between them, it times the three routes
and prints min / median / max; then, on one slab with device events, the whole entry and the simple-packing kernel for scale, and with
the profiler of torch (kernel activities) the device time of every kernel of the entry by name.  One JSON line per result.

    python scripts/grib_ccsds_ingest_bench.py [--reps 5] [--steps 8760]
"""
import argparse
import concurrent.futures
import datetime as dt
import json
import os
import statistics
import struct
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import torch  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import grib, hip, synth  # noqa: E402
from grib_ingest_bench import E, NX, NY, R, START, _sm, stats, timed, write_grib1  # noqa: E402
from grib_complex_ingest_bench import event_ms  # noqa: E402
from grib_ccsds_cases import libaec_encode, load_libaec  # noqa: E402  (the ctypes binding of libaec)

J, RSI, FLAGS = 32, 128, 14


def write_grib2_ccsds(path, X, lat, lon):
    """One edition-2 message per step of the integers ``X`` (T, ny, nx): 2 m temperature, hourly from START, template 5.42.  -> the
    bodies of section 7."""
    T, ny, nx = X.shape
    ud = lambda deg: int(round(float(deg) * 1e6))
    s3 = ((72).to_bytes(4, "big") + b"\x03\x00" + (ny * nx).to_bytes(4, "big") + b"\x00\x00\x00\x00\x06" + (b"\xff" + b"\xff" * 4) * 3
          + nx.to_bytes(4, "big") + ny.to_bytes(4, "big") + bytes(4) + b"\xff" * 4 + _sm(ud(lat[0]), 4) + _sm(ud(lon[0]), 4) + b"\x30"
          + _sm(ud(lat[-1]), 4) + _sm(ud(lon[-1]), 4) + (250000).to_bytes(4, "big") * 2 + b"\x00")
    s4 = ((34).to_bytes(4, "big") + b"\x04" + bytes(4) + b"\x00\x00\x00\x00" + bytes([145]) + bytes(3) + b"\x01" + bytes(4) + bytes([103, 0])
          + (2).to_bytes(4, "big") + b"\xff\xff" + b"\xff" * 4)
    s5 = ((25).to_bytes(4, "big") + b"\x05" + (ny * nx).to_bytes(4, "big") + (42).to_bytes(2, "big") + struct.pack(">f", R) + _sm(E, 2) + _sm(0, 2)
          + bytes([16, 0, FLAGS, J]) + RSI.to_bytes(2, "big"))
    s6 = (6).to_bytes(4, "big") + b"\x06\xff"
    assert len(s3) == 72 and len(s4) == 34 and len(s5) == 25
    bodies = []
    with open(path, "wb") as f:
        for t in range(T):
            when = START + dt.timedelta(hours=t)
            s1 = ((21).to_bytes(4, "big") + b"\x01" + (98).to_bytes(2, "big") + bytes(2) + b"\x04\x00\x01" + when.year.to_bytes(2, "big")
                  + bytes([when.month, when.day, when.hour, 0, 0, 0, 1]))
            data = libaec_encode(X[t].ravel(), 16, J, RSI, 8)
            bodies.append(data)
            body = s1 + s3 + s4 + s5 + s6 + (5 + len(data)).to_bytes(4, "big") + b"\x07" + data + b"7777"
            f.write(b"GRIB\x00\x00\x00\x02" + (16 + len(body)).to_bytes(8, "big") + body)
    return bodies


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8760)
    ap.add_argument("--host-threads", type=int, default=16)
    a = ap.parse_args()
    hip.require_gpu()
    if load_libaec() is None:
        raise SystemExit("grib_ccsds_ingest_bench: libaec cannot be loaded; it encodes the streams")
    T = a.steps
    lat, lon = 60 - 0.25 * np.arange(NY), 235 + 0.25 * np.arange(NX)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    f32 = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1, ocean_frac=0.0) + np.float32(273.15)
    X = np.clip(np.round((np.nan_to_num(f32, nan=280.0).astype(np.float64) - R) / 2.0 ** E), 0, 65535).astype(np.uint16)
    del f32
    with tempfile.TemporaryDirectory(dir=base) as d:
        simple, ccsds = os.path.join(d, "simple16.grib"), os.path.join(d, "ccsds42.grib2")
        write_grib1(simple, X, lat, lon)
        bodies = write_grib2_ccsds(ccsds, X, lat, lon)
        sizes = {"simple16": os.path.getsize(simple), "ccsds42": os.path.getsize(ccsds)}

        def device_route(path):
            ds = af.dataset_from_path(path, "t2m", device="cuda")
            assert ds.cube().is_cuda
            return ds.cube()

        pool = concurrent.futures.ThreadPoolExecutor(a.host_threads)

        def host_route(path):
            # the host decode on `host_threads` threads (the C decoder runs without the interpreter lock), one run of steps each
            gf = grib.open_index(path)
            cuts = np.linspace(0, T, a.host_threads + 1).astype(int)
            parts = list(pool.map(lambda k: gf.read("t2m", steps=(cuts[k], cuts[k + 1])), range(a.host_threads)))
            return torch.from_numpy(np.concatenate(parts)).to("cuda")

        want, got, ref = device_route(ccsds), host_route(ccsds), device_route(simple)          # warm-up; the routes agree bit for bit
        assert got.shape == want.shape == (T, NY, NX) and torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.equal(ref.view(torch.int32), want.view(torch.int32))                       # ... and both files hold the same field
        del want, got, ref
        t = {"ccsds_device": [], "simple_device": [], "ccsds_host": []}
        for _ in range(a.reps):
            t["ccsds_device"].append(timed(lambda: device_route(ccsds))[1])
            t["simple_device"].append(timed(lambda: device_route(simple))[1])
            t["ccsds_host"].append(timed(lambda: host_route(ccsds))[1])
        med = {k: statistics.median(v) for k, v in t.items()}
        print(json.dumps({"steps": T, "file_bytes": sizes, "encoder": "libaec, block size 32, rsi 128, preprocessor on", "ccsds_5_42_device_route": stats(t["ccsds_device"]),
                          "simple_16_bit_device_route": stats(t["simple_device"]), f"ccsds_host_route_{a.host_threads}_threads_plus_upload": stats(t["ccsds_host"]),
                          "ccsds_over_simple": round(med["ccsds_device"] / med["simple_device"], 3),
                          "ccsds_device_over_host": round(med["ccsds_device"] / med["ccsds_host"], 4), "reps": a.reps}), flush=True)

    # the kernels on one slab of m fields
    npts = NY * NX
    m = min(T, 256)
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    cube = torch.empty((m, NY, NX), dtype=torch.float32, device="cuda")
    stage, rec = b"", np.zeros(m, dtype=hip.GRIB_ASTEP)
    for k in range(m):
        body = bodies[k]
        rec[k]["data_off"], rec[k]["data_bytes"], rec[k]["bitmap_off"], rec[k]["n_values"] = len(stage), len(body), -1, npts
        rec[k]["nbits"], rec[k]["flags"], rec[k]["block_size"], rec[k]["rsi"] = 16, FLAGS, J, RSI
        rec[k]["R"], rec[k]["s"], rec[k]["d"] = R, 2.0 ** E, 1.0
        stage += body + b"\x00" * (-len(body) % 4)
    mr = -(-npts // (J * RSI))
    stage_d = torch.from_numpy(np.frombuffer(stage, dtype=np.uint8).copy()).cuda()
    rec_d = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
    scratch = torch.empty(hip.grib_ccsds_scratch_bytes(m, npts, mr), dtype=torch.uint8, device="cuda")
    entry = lambda: hip.grib_unpack_ccsds(stage_d, rec_d, m, mr, (NY, NX), (0, 0, NY, NX), cube, (0, 0, 0), scratch, errors)
    ms = event_ms(entry)
    assert int(errors.item()) == 0
    whole = statistics.median(ms)
    print(json.dumps({"kernel": "afhip_grib_unpack_ccsds, all passes", "slab_steps": m, "rsis_per_step": mr, "staged_bytes": len(stage),
                      "bits_per_value_staged": round(len(stage) * 8 / (m * npts), 2), "ms_min": round(min(ms), 4), "ms_median": round(whole, 4),
                      "ms_max": round(max(ms), 4), "written_GB_per_s": round(cube.numel() * 4 / whole / 1e6, 1)}), flush=True)
    # every kernel of the entry by name: device time from the profiler's kernel activities, 20 calls after the warm-up above
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(20):
                entry()
            torch.cuda.synchronize()
        per = {}
        for ev in prof.key_averages():
            if "k_grib_" in ev.key:
                us = getattr(ev, "device_time_total", None)
                us = getattr(ev, "cuda_time_total", 0.0) if us is None else us
                per[ev.key.split("(")[0][:60]] = round(us / max(ev.count, 1) / 1e3, 4)
        print(json.dumps({"kernels_of_the_entry_ms_per_call": per, "slab_steps": m, "sum_ms": round(sum(per.values()), 4)}), flush=True)
    except Exception as e:                                               # the timing above stands without it
        print(json.dumps({"kernels_of_the_entry_ms_per_call": None, "profiler": f"{type(e).__name__}: {e}"}), flush=True)
    # the 16-bit simple-packing kernel on the same fields, for scale
    step = (npts * 2 + 3) // 4 * 4
    rec = np.zeros(m, dtype=hip.GRIB_STEP)
    rec["bitmap_off"], rec["data_off"], rec["data_bytes"], rec["nbits"] = -1, np.arange(m) * step, npts * 2, 16
    rec["R"], rec["s"], rec["d"] = R, 2.0 ** E, 1.0
    stage_d = torch.from_numpy(np.ascontiguousarray(X[:m].astype(">u2")).view(np.uint8).reshape(-1).copy()).cuda()
    rec_d = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
    rank = torch.empty(hip.grib_rank_bytes(m, npts), dtype=torch.uint8, device="cuda")
    ms = event_ms(lambda: hip.grib_unpack(stage_d, rec_d, m, (NY, NX), (0, 0, NY, NX), cube, (0, 0, 0), rank, errors))
    assert int(errors.item()) == 0
    print(json.dumps({"kernel": "k_grib_rank + k_grib_unpack, 16 bits", "slab_steps": m, "ms_median": round(statistics.median(ms), 4),
                      "ccsds_over_simple": round(whole / statistics.median(ms), 2)}), flush=True)


if __name__ == "__main__":
    main()
