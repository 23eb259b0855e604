#!/usr/bin/env python3
"""Complex-packed GRIB2 files into HBM: the device route (`afhip_grib_unpack_complex`: group pass, value pass, the running sums of
`afhip_delta_decode`, place pass) against the same integers in 16-bit simple packing on the existing device route — the yardstick of
DESIGN.md §8 —, against the numpy host route (`grib.GribFile.read`, then one upload), and its kernels one by one.

Workload: the BASELINE configs[0] cube (8760 x 104 x 236, synth.temperature_cube) as 16-bit integers of 2^-9 K from 200 K, written
into /dev/shm twice: as edition-1 messages in simple packing (scripts/grib_ingest_bench.py's writer) and as edition-2 messages in
template 5.3, spatial differencing of order 2, four-octet extra descriptors (a first value of 16 bits does not fit two).  THE GROUP RULE of the writer here: every 32 consecutive
values are one group (104 x 236 = 767 groups of 32, ``ref_len`` 32, ``nbits_len`` 0); a group's reference is its smallest member and
its width the bits of its largest remainder.  That is simpler than what NCEP's writers do (they grow and merge groups by a cost
rule), and nothing here says how their files would time.

In one process, after a warm-up in which the routes are compared bit for bit, and alternating between them, it times the three
routes and prints min / median / max; then, with device events on one slab, the whole entry and each of its kernels alone — the
entry run with only the launches up to that kernel is not possible from outside, so the kernels are timed through the library's own
entries where they have one (`delta_decode` on a buffer of the same shape) and otherwise by difference: order 0 (no sums), order 1,
order 2, and the simple-packing kernel for scale.  One JSON line per result.

    python scripts/grib_complex_ingest_bench.py [--reps 5] [--steps 8760]
"""
import argparse
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
import torch  # noqa: E402

import aggfly_amd as af  # noqa: E402
from aggfly_amd import grib, hip, synth  # noqa: E402
from grib_ingest_bench import E, NX, NY, R, START, _sm, stats, timed, write_grib1  # noqa: E402

GROUP = 32


def pack_fields(values, widths) -> bytes:
    """``values[i]`` as a ``widths[i]``-bit big-endian field each, back to back, zero bits up to the octet boundary."""
    v, w = values.astype(np.uint64), widths.astype(np.int64)
    first = np.cumsum(w) - w
    n = int(w.sum())
    bits = np.zeros(n + (-n % 8), dtype=np.uint8)
    for j in range(int(w.max()) if len(w) else 0):
        has = w > j
        bits[(first + w - 1 - j)[has]] = ((v[has] >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits).tobytes()


def complex_sections(x, order=2):
    """(section 5, section 7, record fields) of the integers ``x`` (1-D int64) in template 5.3 (order 1 / 2) or 5.2 (order 0), groups of
    GROUP values."""
    n = x.size
    if order == 2:
        raw = np.concatenate([[0, 0], x[2:] - 2 * x[1:-1] + x[:-2]])
    elif order == 1:
        raw = np.concatenate([[0], x[1:] - x[:-1]])
    else:
        raw = x.copy()
    minsd = int(raw[order:].min()) if order else 0
    raw[order:] -= minsd
    ng = (n + GROUP - 1) // GROUP
    pad = np.full(ng * GROUP, -1, dtype=np.int64)
    pad[:n] = raw
    groups = pad.reshape(ng, GROUP)
    refs = np.where(groups >= 0, groups, np.iinfo(np.int64).max).min(axis=1)
    rem = np.where(groups >= 0, groups - refs[:, None], 0)
    widths = np.ceil(np.log2(rem.max(axis=1).astype(np.float64) + 1)).astype(np.int64)       # bits of the largest remainder (exact below 2^52)
    nbits_ref, ref_width = int(refs.max()).bit_length(), int(widths.min())
    nbits_width = int((widths - ref_width).max()).bit_length()
    last_len = n - (ng - 1) * GROUP
    body = b"".join(_sm(int(v), 4) for v in ([int(x[0]), int(x[1]), minsd] if order == 2 else [int(x[0]), minsd] if order == 1 else []))
    body += pack_fields(refs, np.full(ng, nbits_ref)) + pack_fields(widths - ref_width, np.full(ng, nbits_width))
    body += pack_fields(rem.ravel()[pad >= 0], np.repeat(widths, GROUP)[pad >= 0])
    s5 = ((49 if order else 47).to_bytes(4, "big") + b"\x05" + n.to_bytes(4, "big") + (3 if order else 2).to_bytes(2, "big") + struct.pack(">f", R)
          + _sm(E, 2) + _sm(0, 2) + bytes([nbits_ref, 0, 1, 0]) + bytes(8) + ng.to_bytes(4, "big") + bytes([ref_width, nbits_width])
          + GROUP.to_bytes(4, "big") + b"\x01" + last_len.to_bytes(4, "big") + b"\x00" + (bytes([order, 4]) if order else b""))
    s7 = (5 + len(body)).to_bytes(4, "big") + b"\x07" + body
    return s5, s7, dict(n_groups=ng, ref_len=GROUP, last_len=last_len, nbits_ref=nbits_ref, ref_width=ref_width, nbits_width=nbits_width,
                        len_inc=1, nbits_len=0, order=order, extra=4 if order else 0)


def write_grib2_complex(path, X, lat, lon, order=2):
    """One edition-2 message per step of the integers ``X`` (T, ny, nx): 2 m temperature, hourly from START, template 5.3 / 5.2."""
    T, ny, nx = X.shape
    ud = lambda deg: int(round(float(deg) * 1e6))
    s3 = ((72).to_bytes(4, "big") + b"\x03\x00" + (ny * nx).to_bytes(4, "big") + b"\x00\x00\x00\x00\x06" + (b"\xff" + b"\xff" * 4) * 3
          + nx.to_bytes(4, "big") + ny.to_bytes(4, "big") + bytes(4) + b"\xff" * 4 + _sm(ud(lat[0]), 4) + _sm(ud(lon[0]), 4) + b"\x30"
          + _sm(ud(lat[-1]), 4) + _sm(ud(lon[-1]), 4) + (250000).to_bytes(4, "big") * 2 + b"\x00")
    s4 = ((34).to_bytes(4, "big") + b"\x04" + bytes(4) + b"\x00\x00\x00\x00" + bytes([145]) + bytes(3) + b"\x01" + bytes(4) + bytes([103, 0])
          + (2).to_bytes(4, "big") + b"\xff\xff" + b"\xff" * 4)
    s6 = (6).to_bytes(4, "big") + b"\x06\xff"
    assert len(s3) == 72 and len(s4) == 34
    with open(path, "wb") as f:
        for t in range(T):
            when = START + dt.timedelta(hours=t)
            s1 = ((21).to_bytes(4, "big") + b"\x01" + (98).to_bytes(2, "big") + bytes(2) + b"\x04\x00\x01" + when.year.to_bytes(2, "big")
                  + bytes([when.month, when.day, when.hour, 0, 0, 0, 1]))
            s5, s7, _ = complex_sections(X[t].ravel().astype(np.int64), order)
            body = s1 + s3 + s4 + s5 + s6 + s7 + b"7777"
            f.write(b"GRIB\x00\x00\x00\x02" + (16 + len(body)).to_bytes(8, "big") + body)


def event_ms(fn, reps=25, warm=5):
    ms = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=8760)
    ap.add_argument("--kernels-only", action="store_true", help="skip the files and the routes: the slab timings alone (what a kernel trace is taken of)")
    a = ap.parse_args()
    hip.require_gpu()
    T = a.steps
    lat, lon = 60 - 0.25 * np.arange(NY), 235 + 0.25 * np.arange(NX)
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    f32 = synth.temperature_cube(T, NY, NX, dtype=np.float32, seed=1, ocean_frac=0.0) + np.float32(273.15)
    X = np.clip(np.round((np.nan_to_num(f32, nan=280.0).astype(np.float64) - R) / 2.0 ** E), 0, 65535).astype(np.uint16)
    del f32
    if not a.kernels_only:
        with tempfile.TemporaryDirectory(dir=base) as d:
            simple, cplx = os.path.join(d, "simple16.grib"), os.path.join(d, "complex53.grib2")
            write_grib1(simple, X, lat, lon)
            write_grib2_complex(cplx, X, lat, lon)
            sizes = {"simple16": os.path.getsize(simple), "complex53": os.path.getsize(cplx)}

            def device_route(path):
                ds = af.dataset_from_path(path, "t2m", device="cuda")
                assert ds.cube().is_cuda
                return ds.cube()

            def host_route(path):
                return torch.from_numpy(np.ascontiguousarray(af.dataset_from_path(path, "t2m").cube())).to("cuda")

            want, got, ref = device_route(cplx), host_route(cplx), device_route(simple)          # warm-up; the routes agree bit for bit
            assert got.shape == want.shape == (T, NY, NX) and torch.equal(got.view(torch.int32), want.view(torch.int32))
            assert torch.equal(ref.view(torch.int32), want.view(torch.int32))                     # ... and both files hold the same field
            del want, got, ref
            t = {"complex_device": [], "simple_device": [], "complex_host": []}
            for _ in range(a.reps):
                t["complex_device"].append(timed(lambda: device_route(cplx))[1])
                t["simple_device"].append(timed(lambda: device_route(simple))[1])
                t["complex_host"].append(timed(lambda: host_route(cplx))[1])
            med = {k: statistics.median(v) for k, v in t.items()}
            print(json.dumps({"steps": T, "file_bytes": sizes, "group_rule": f"every {GROUP} consecutive values", "complex_5_3_order_2_device_route": stats(t["complex_device"]),
                              "simple_16_bit_device_route": stats(t["simple_device"]), "complex_host_route_plus_upload": stats(t["complex_host"]),
                              "complex_over_simple": round(med["complex_device"] / med["simple_device"], 3),
                              "complex_device_over_host": round(med["complex_device"] / med["complex_host"], 4), "reps": a.reps}), flush=True)

    # the kernels on one slab of m fields, by device events.  Bytes moved per value: value pass 8 written (+ the staged bits read), a
    # running sum 8 read + 8 read + 8 written, place pass 8 read + 4 written.
    npts = NY * NX
    m = min(T, 256)
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    cube = torch.empty((m, NY, NX), dtype=torch.float32, device="cuda")
    per_order = {}
    for order in (0, 1, 2):
        stage, rec = b"", np.zeros(m, dtype=hip.GRIB_CSTEP)
        for k in range(m):
            _, s7, fields = complex_sections(X[k].ravel().astype(np.int64), order)
            body = s7[5:]
            rec[k]["data_off"], rec[k]["data_bytes"], rec[k]["bitmap_off"], rec[k]["n_values"] = len(stage), len(body), -1, npts
            for key, v in fields.items():
                rec[k][key] = v
            rec[k]["R"], rec[k]["s"], rec[k]["d"] = R, 2.0 ** E, 1.0
            stage += body + b"\x00" * (-len(body) % 4)
        mg = int(rec["n_groups"].max())
        stage_d = torch.from_numpy(np.frombuffer(stage, dtype=np.uint8).copy()).cuda()
        rec_d = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
        scratch = torch.empty(hip.grib_complex_scratch_bytes(m, npts, mg), dtype=torch.uint8, device="cuda")
        ms = event_ms(lambda: hip.grib_unpack_complex(stage_d, rec_d, m, order, mg, (NY, NX), (0, 0, NY, NX), cube, (0, 0, 0), scratch, errors))
        assert int(errors.item()) == 0
        per_order[order] = statistics.median(ms)
        print(json.dumps({"kernel": "afhip_grib_unpack_complex, all passes", "order": order, "slab_steps": m, "groups_per_step": mg, "staged_bytes": len(stage),
                          "ms_min": round(min(ms), 4), "ms_median": round(statistics.median(ms), 4), "ms_max": round(max(ms), 4),
                          "written_GB_per_s": round(cube.numel() * 4 / statistics.median(ms) / 1e6, 1)}), flush=True)
    # one running sum over a buffer of the value scratch's shape, through its own entry
    vals = torch.zeros(m * npts, dtype=torch.int64, device="cuda")
    sums = torch.empty(hip.delta_scratch_bytes(m, npts, 8), dtype=torch.uint8, device="cuda")
    ms = event_ms(lambda: hip.delta_decode(vals, m, npts, 8, sums))
    one_sum = statistics.median(ms)
    print(json.dumps({"kernel": "one running sum (k_delta_tile_sums + k_delta_scan_sums + k_delta_scan_tiles)", "slab_steps": m, "ms_median": round(one_sum, 4),
                      "TB_per_s_moved": round(m * npts * 24 / one_sum / 1e9, 3), "by_difference_order_1_minus_0_ms": round(per_order[1] - per_order[0], 4),
                      "by_difference_order_2_minus_1_ms": round(per_order[2] - per_order[1], 4)}), flush=True)
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
                      "order_0_over_simple": round(per_order[0] / statistics.median(ms), 2), "order_2_over_simple": round(per_order[2] / statistics.median(ms), 2)}), flush=True)


if __name__ == "__main__":
    main()
