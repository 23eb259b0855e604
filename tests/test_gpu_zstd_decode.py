"""Zstandard frames decoded in HBM (`afhip_zstd_decode`, planned by `afcodec_zstd_plan`): every frame the real libzstd wrote
(tests/golden/zstd_fixtures.json) decodes bit-exact on the GPU, canaries around every destination untouched; damaged frames
are counted and stay inside their destination; zstd stores read through `dataset_from_path(device="cuda")` give the same cube
with the decode on the GPU (no host zstd decode at all) or on the host."""
import ctypes as C
import os
import sys

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_zstd_fixtures as zf                  # noqa: E402

import aggfly_amd as af                          # noqa: E402
from aggfly_amd import codec, synth, io as afio  # noqa: E402

pytestmark = pytest.mark.gpu
FIX = zf.load()
TAKEN = [(e, f, r) for e, f, r in FIX if e["taken"]]


def _gpu_zstd(torch, frames, sizes):
    """Plan + decode a batch of frames in HBM -> (plan, out bytes on the host, out_off, errors, rounds)."""
    from aggfly_amd import hip
    sizes = np.asarray(sizes, dtype=np.int64)
    base, co, cs, oo, nout = zf.pack(frames, sizes)
    fr, bl = np.zeros(len(frames) + 1, dtype=codec.ZSTD_FRAME), np.zeros(8192, dtype=codec.ZSTD_BLOCK)
    p = codec.zstd_plan(base, co, cs, oo, sizes, fr, bl, strict=False)
    comp = torch.from_numpy(base).cuda()
    frd = torch.from_numpy(fr[:max(p.n_frames, 1)].view(np.uint8).copy()).cuda()
    bld = torch.from_numpy(bl[:max(p.n_blocks, 1)].view(np.uint8).copy()).cuda()
    out = torch.full((nout,), 0xAB, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(hip.zstd_scratch_bytes(p), dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    rounds = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.zstd_decode(comp, base.nbytes, frd, bld, p, scratch, out, errors, rounds)
    torch.cuda.synchronize()
    return p, out.cpu().numpy(), oo, int(errors.item()), int(rounds.item()), (base, fr, bl, nout)


@pytest.mark.parametrize("one_per_launch", [False, True])
def test_real_libzstd_frames_decode_bit_exact_in_hbm(torch_cuda, one_per_launch):
    groups = [[x] for x in TAKEN] if one_per_launch else [TAKEN]
    for g in groups:
        raws = [r for _, _, r in g]
        p, host, oo, nerr, rounds, _ = _gpu_zstd(torch_cuda, [f for _, f, _ in g], [len(r) for r in raws])
        assert nerr == 0 and (p.results >= 0).all()
        canary = np.ones(host.size, dtype=bool)
        for (e, _, raw), o in zip(g, oo):
            assert host[o:o + len(raw)].tobytes() == raw, (e["recipe"], e["level"], e["n"])
            canary[o:o + len(raw)] = False
        assert (host[canary] == 0xAB).all()
        assert 0 <= rounds <= 40
    print("pointer-jump rounds (all fixtures in one batch / the last one alone):", rounds)


def test_damaged_frames_are_counted_and_stay_in_their_destination(torch_cuda):
    """A few dozen seeded corruptions that the planner accepts, batched with intact frames: the GPU counts exactly the
    damaged frames the host emulation of the same passes finds, writes no canary, and the intact frames decode bit-exact."""
    rng = np.random.default_rng(77)
    small = [(e, f, r) for e, f, r in TAKEN if 200 < len(f) < 20000]
    frames, raws, damaged = [], [], []
    while len(damaged) < 40:
        e, f, raw = small[int(rng.integers(len(small)))]
        b = bytearray(f)
        for _ in range(int(rng.integers(1, 4))):
            j = int(rng.integers(len(b) // 2, len(b)))
            b[j] ^= 1 << int(rng.integers(8))
        base, co, cs, oo, nout = zf.pack([bytes(b)], [len(raw)])
        fr, bl = np.zeros(2, dtype=codec.ZSTD_FRAME), np.zeros(64, dtype=codec.ZSTD_BLOCK)
        if codec.zstd_plan(base, co, cs, oo, [len(raw)], fr, bl, strict=False).results[0] == len(raw):
            damaged.append(len(frames))
            frames.append(bytes(b)); raws.append(raw)
        if len(damaged) % 4 == 0:
            frames.append(f); raws.append(raw)                  # an intact one between them
    p, host, oo, nerr, _, (base, fr, bl, nout) = _gpu_zstd(torch_cuda, frames, [len(r) for r in raws])
    emu = np.full(nout, 0xAB, dtype=np.uint8)
    want_err, _ = codec.zstd_emulate(base, fr, bl, p, emu)
    assert nerr == want_err and 0 < nerr <= len(damaged)
    canary = np.ones(host.size, dtype=bool)
    for i, (raw, o) in enumerate(zip(raws, oo)):
        canary[o:o + len(raw)] = False
        if i not in damaged:
            assert host[o:o + len(raw)].tobytes() == raw
    assert (host[canary] == 0xAB).all()


def _ds(T, ny, nx, dtype, seed):
    cube = synth.temperature_cube(T, ny, nx, dtype=dtype, seed=seed, scattered_nan=7)
    time = pd.date_range("2003-01-01", periods=T, freq="h")
    return af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                   {"time": time, "latitude": 30 + 0.5 * np.arange(ny), "longitude": 10 + 0.5 * np.arange(nx)}),
                      lon_is_360=True), cube


def _count_zstd_host_decodes(monkeypatch):
    calls = []
    real = codec.decode_ranges
    monkeypatch.setattr(codec, "decode_ranges", lambda kind, locs, outs, threads=8, **kw: (calls.append(kind), real(kind, locs, outs, threads, **kw))[1])
    return calls


def test_zstd_stores_read_bit_exact_on_both_routes(torch_cuda, tmp_path, monkeypatch):
    T, ny, nx = 24 * 20, 12, 16
    calls = _count_zstd_host_decodes(monkeypatch)
    layouts = [(2, {"time": 48, "latitude": ny, "longitude": nx}, None),               # time-contiguous
               (3, {"time": 96, "latitude": 5, "longitude": 7}, None),                 # space-tiled
               (3, {"time": T, "latitude": 6, "longitude": 6}, None),                  # whole-series tiles (the converter's layout)
               (3, {"time": 24, "latitude": 6, "longitude": 16}, {"time": 120, "latitude": 12, "longitude": 16})]   # shards
    for dtype in (np.float32, np.float64):
        ds, cube = _ds(T, ny, nx, dtype, seed=5)
        for fmt, chunks, shards in layouts:
            path = str(tmp_path / f"z_{np.dtype(dtype).name}_{fmt}_{chunks['time']}_{chunks['latitude']}_{shards is not None}.zarr")
            af.dataset_to_zarr(ds, path, var="t2m", chunks=chunks, shards=shards, compress="zstd", zarr_format=fmt)
            for sel, lo, hi in ((None, 0, T), (slice("2003-01-03 05:00", "2003-01-11 17:00"), 53, 258)):
                got = {}
                for mode in ("1", "0"):
                    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
                    calls.clear()
                    d = af.dataset_from_path(path, "t2m", time_sel=sel, device="cuda")
                    got[mode] = d.cube().cpu().numpy()
                    if mode == "1":
                        assert "zstd" not in calls, (path, sel)
                    else:
                        assert "zstd" in calls
                np.testing.assert_array_equal(got["1"], cube[lo:hi])
                np.testing.assert_array_equal(got["0"], got["1"])


def test_store_with_a_checksummed_chunk_finishes_on_the_host_route(torch_cuda, tmp_path, monkeypatch):
    T, ny, nx = 24 * 10, 8, 10
    ds, cube = _ds(T, ny, nx, np.float32, seed=9)
    path = str(tmp_path / "ck.zarr")
    af.dataset_to_zarr(ds, path, var="t2m", chunks={"time": 48, "latitude": ny, "longitude": nx}, compress="zstd", zarr_format=2)
    lib = C.CDLL("libzstd.so.1")
    lib.ZSTD_createCCtx.restype = C.c_void_p
    lib.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.ZSTD_compress2.restype = C.c_size_t
    cctx = lib.ZSTD_createCCtx()
    lib.ZSTD_CCtx_setParameter(cctx, zf.ZSTD_c_checksumFlag, 1)
    raw = np.ascontiguousarray(cube[96:144]).tobytes()
    dst = C.create_string_buffer(len(raw) + 4096)
    n = lib.ZSTD_compress2(cctx, dst, len(raw) + 4096, raw, len(raw))
    chunk = os.path.join(path, "t2m", "2.0.0")
    assert os.path.exists(chunk)
    with open(chunk, "wb") as f:
        f.write(dst.raw[:n])
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "1")
    calls = _count_zstd_host_decodes(monkeypatch)
    d = af.dataset_from_path(path, "t2m", device="cuda")
    np.testing.assert_array_equal(d.cube().cpu().numpy(), cube)
    assert "zstd" in calls


def test_aggregate_panel_equal_across_routes(torch_cuda, tmp_path, monkeypatch):
    T, ny, nx = 24 * 31, 16, 24
    ds, cube = _ds(T, ny, nx, np.float64, seed=12)
    path = str(tmp_path / "agg.zarr")
    af.dataset_to_zarr(ds, path, var="t2m", chunks={"time": T, "latitude": 8, "longitude": 8}, compress="zstd", zarr_format=3)
    tab = synth.weights_table(ny, nx, 9, seed=3, secondary=True)
    regions = pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]})
    spec = dict(dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": "year"})])
    panels = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
        d = af.dataset_from_path(path, "t2m", device="cuda")
        w = af.weights_from_objects(d, af.GeoRegions(regions), table=tab)
        panels[mode] = af.aggregate_dataset(dataset=d, weights=w, **spec)
    pd.testing.assert_frame_equal(panels["1"], panels["0"])


def test_reference_layout_store_above_the_threshold_takes_the_gpu_route(torch_cuda, tmp_path, monkeypatch):
    """The converter's layout (default chunks: whole time series in square tiles) at the `auto` threshold's size: decoded in
    HBM with no environment switch."""
    monkeypatch.delenv("AGGFLY_HIP_GPU_DECODE", raising=False)
    ny, nx = 104, 236
    T = -(-afio.GPU_DECODE_AUTO_BYTES_ZSTD // (ny * nx * 4))
    cube = synth.temperature_cube(T, ny, nx, dtype=np.float32, seed=21)
    time = pd.date_range("2010-01-01", periods=T, freq="h")
    ds = af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                 {"time": time, "latitude": 30 + 0.25 * np.arange(ny), "longitude": 10 + 0.25 * np.arange(nx)}))
    path = str(tmp_path / "ref_layout.zarr")
    af.dataset_to_zarr(ds, path, var="t2m", compress="zstd", zarr_format=3)
    calls = _count_zstd_host_decodes(monkeypatch)
    d = af.dataset_from_path(path, "t2m", device="cuda")
    assert "zstd" not in calls
    np.testing.assert_array_equal(d.cube().cpu().numpy(), cube)
