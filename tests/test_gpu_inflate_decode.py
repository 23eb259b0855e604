"""zlib (deflate) chunks decoded in HBM (`afhip_inflate_decode`, planned by `afcodec_inflate_plan`): every stream of
tests/test_inflate_plan.py decodes bit-exact on the GPU, canaries around every destination untouched; damaged streams are counted
exactly as the host emulation of the same passes counts them and stay inside their destination; netCDF-4 / HDF5 files and a Zarr v2
zlib store read through `dataset_from_path(device="cuda")` give the same cube with the decode on the GPU or on the host."""
import os
import sys
import zlib

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import inflate_cases as ic                       # noqa: E402

import aggfly_amd as af                          # noqa: E402
from aggfly_amd import codec, synth              # noqa: E402

pytestmark = pytest.mark.gpu
GOOD = ic.good_streams()
FIX = os.path.join(HERE, "golden", "hdf5")
TAIL = 4096                                      # canary bytes behind the scratch


def _gpu_inflate(torch, streams, sizes, typesize=1):
    """Plan + decode a batch in HBM -> (plan, out bytes on the host, out_off, errors, scratch tail, the host-side batch)."""
    from aggfly_amd import hip
    base, co, cs, oo, nout, st, sh, p = ic.plan(streams, sizes, typesize, strict=False)
    comp = torch.from_numpy(base).cuda()
    std = torch.from_numpy(st[:max(p.n_streams, 1)].view(np.uint8).copy()).cuda()
    shd = torch.from_numpy(sh[:max(p.n_shuf, 1)].view(np.uint8).copy()).cuda()
    out = torch.full((nout,), 0xAB, dtype=torch.uint8, device="cuda")
    need = hip.inflate_scratch_bytes(p)
    assert need == p.scratch_bytes()
    scratch = torch.full((need + TAIL,), 0xCD, dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    rounds = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.inflate_decode(comp, base.nbytes, std, shd, p, scratch[:need], out, errors, rounds)
    torch.cuda.synchronize()
    assert 0 <= int(rounds.item()) <= 40
    return p, out.cpu().numpy(), oo, int(errors.item()), scratch[need:].cpu().numpy(), (base, st, sh, nout)


def _check(host, oo, raws, tail, skip=()):
    for i, (raw, o) in enumerate(zip(raws, oo)):
        if i not in skip:
            assert host[o:o + len(raw)].tobytes() == raw, i
    assert (host[ic.canary_mask(host.size, oo, [len(r) for r in raws])] == 0xAB).all()
    assert (tail == 0xCD).all()


@pytest.mark.parametrize("one_per_launch", [False, True])
def test_zlib_streams_decode_bit_exact_in_hbm(torch_cuda, one_per_launch):
    groups = [[x] for x in GOOD] if one_per_launch else [GOOD]
    for g in groups:
        raws = [r for _, _, r in g]
        p, host, oo, nerr, tail, _ = _gpu_inflate(torch_cuda, [s for _, s, _ in g], [len(r) for r in raws])
        assert nerr == 0 and (p.results >= 0).all(), [n for n, _, _ in g]
        _check(host, oo, raws, tail)


@pytest.mark.parametrize("typesize", [2, 4, 8])
def test_shuffled_chunks_come_out_unshuffled_in_hbm(torch_cuda, typesize):
    raws = [ic.CUBE.tobytes(), ic.CUBE.tobytes()[:50001], b"abc", b""]
    streams = [zlib.compress(ic.shuffle(r, typesize), 4) for r in raws]
    p, host, oo, nerr, tail, _ = _gpu_inflate(torch_cuda, streams, [len(r) for r in raws], typesize)
    assert nerr == 0
    _check(host, oo, raws, tail)


def test_130_uneven_streams_in_one_launch(torch_cuda):
    """More streams than two waves have lanes, 1 byte ... 300 KB, every other one written through the shuffle filter."""
    field = synth.temperature_cube(96, 26, 40, dtype=np.float32, seed=8).tobytes()
    sizes = np.maximum(np.geomspace(1, 300000, 130).round().astype(np.int64), np.arange(1, 131))
    rng = np.random.default_rng(4)
    raws, streams, ts = [], [], []
    for i, n in enumerate(sizes):
        a = int(rng.integers(0, len(field) - int(n) + 1)) // 4 * 4
        raws.append(field[a:a + int(n)])
        ts.append(4 if i % 2 else 1)
        streams.append(zlib.compress(ic.shuffle(raws[-1], 4) if ts[-1] == 4 else raws[-1], 1 + i % 9))
    assert len(raws) == 130 and len(raws[0]) == 1 and len(raws[-1]) == 300000
    p, host, oo, nerr, tail, _ = _gpu_inflate(torch_cuda, streams, [len(r) for r in raws], np.array(ts, dtype=np.int32))
    assert nerr == 0 and p.n_streams == 130 and p.n_shuf == sum(t == 4 and len(r) >= 4 for t, r in zip(ts, raws))
    _check(host, oo, raws, tail)


def test_damaged_streams_are_counted_and_stay_in_their_destination(torch_cuda):
    """32 damaged streams (the refused ones of tests/test_inflate_plan.py, then seeded mutations that zlib refuses) mixed with 32
    good ones in ONE launch.  Each damaged stream first goes through the host emulation of the passes, where its canaries must hold."""
    damaged = ic.damaged_streams(32)
    assert len(damaged) == 32
    for s, n in damaged:
        base, co, cs, oo, nout, st, sh, p = ic.plan([s], [n], strict=False)
        assert p.results[0] == n
        out = np.full(nout, 0xAB, dtype=np.uint8)
        errors, _ = codec.inflate_emulate(base, st, sh, p, out)
        assert errors == 1 and (out[:oo[0]] == 0xAB).all() and (out[oo[0] + n:] == 0xAB).all()
    small = [(s, r) for _, s, r in GOOD if len(s) < 65536]
    streams, raws, bad = [], [], []
    for i, (s, n) in enumerate(damaged):
        bad.append(len(streams))
        streams.append(s); raws.append(b"\0" * n)
        g = small[i % len(small)]
        streams.append(g[0]); raws.append(g[1])
    p, host, oo, nerr, tail, (base, st, sh, nout) = _gpu_inflate(torch_cuda, streams, [len(r) for r in raws])
    emu = np.full(nout, 0xAB, dtype=np.uint8)
    want_err, _ = codec.inflate_emulate(base, st, sh, p, emu)
    assert want_err == 32 and nerr == want_err
    _check(host, oo, raws, tail, skip=bad)


def _spy(monkeypatch):
    calls = []
    real = codec.decode_ranges
    monkeypatch.setattr(codec, "decode_ranges", lambda kind, locs, outs, threads=8, **kw: (calls.append((kind, len(locs))), real(kind, locs, outs, threads, **kw))[1])
    return calls


def _zlib_chunks(calls):
    return sum(n for kind, n in calls if kind == "zlib" or (isinstance(kind, tuple) and kind[0] == "zlib"))


def _spy_hbm(monkeypatch):
    """Chunks that `hip.inflate_decode` was asked to decode in HBM."""
    from aggfly_amd import hip
    seen = []
    real = hip.inflate_decode
    monkeypatch.setattr(hip, "inflate_decode", lambda comp, n, st, sh, plan, *a, **kw: (seen.append(plan.n_streams), real(comp, n, st, sh, plan, *a, **kw))[1])
    return seen


@pytest.mark.parametrize("fn", ["nc4_like.nc", "old_style.h5", "unlimited_time.nc"])
def test_netcdf4_files_read_bit_exact_on_both_routes(torch_cuda, monkeypatch, fn):
    """Whole variable, a time window, a region clip: under =1 the request's chunks are decoded in HBM except its host-decoded tail
    (`io._decode_batches`: a fifth of the request's chunks at the most), under =0 every one of them on the host."""
    path = os.path.join(FIX, fn)
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE_HOST_TAIL_MIN_MB", "0")
    calls, hbm = _spy(monkeypatch), _spy_hbm(monkeypatch)
    regions = af.GeoRegions(pd.DataFrame({"geoid": ["a"], "minx": [-129.3], "miny": [48.4], "maxx": [-127.6], "maxy": [49.4]}))
    for kw in ({}, {"time_sel": slice("2000-01-03", "2000-01-05")}, {"georegions": regions, "lon_is_360": True}):
        got, request = {}, None
        for mode in ("1", "0"):
            monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
            calls.clear(); hbm.clear()
            d = af.dataset_from_path(path, "t2m", device="cuda", **kw)
            got[mode] = d.cube().cpu().numpy()
            host, gpu = _zlib_chunks(calls), sum(hbm)
            print(fn, sorted(kw), "mode", mode, "chunks decoded in HBM", gpu, "on the host", host)
            if mode == "1":
                request = gpu + host
                assert gpu > 0 and host == request * 20 // 100, (fn, kw, gpu, host)
            else:
                assert gpu == 0 and host == request, (fn, kw, gpu, host, request)
        assert got["1"].shape == got["0"].shape and got["1"].size
        np.testing.assert_array_equal(got["1"], got["0"])
        if not kw:
            np.testing.assert_array_equal(got["1"], af.dataset_from_path(path, "t2m").cube())


def _ds(T, ny, nx, dtype, seed):
    cube = synth.temperature_cube(T, ny, nx, dtype=dtype, seed=seed, scattered_nan=7)
    time = pd.date_range("2003-01-01", periods=T, freq="h")
    return af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                   {"time": time, "latitude": 30 + 0.5 * np.arange(ny), "longitude": 10 + 0.5 * np.arange(nx)}),
                      lon_is_360=True), cube


def test_zarr_v2_zlib_store_equal_across_routes(torch_cuda, tmp_path, monkeypatch):
    T, ny, nx = 24 * 31, 16, 24
    ds, cube = _ds(T, ny, nx, np.float64, seed=12)
    tab = synth.weights_table(ny, nx, 9, seed=3, secondary=True)
    regions = pd.DataFrame({"geoid": [f"r{i}" for i in range(int(tab.index_right.max()) + 1)]})
    spec = dict(dd=[("aggregate", {"calc": "dd", "groupby": "date", "ddargs": [10, 30, 0]}), ("aggregate", {"calc": "sum", "groupby": "year"})])
    calls, hbm = _spy(monkeypatch), _spy_hbm(monkeypatch)
    for name, chunks in (("rows.zarr", {"time": 48, "latitude": ny, "longitude": nx}), ("tiles.zarr", {"time": 96, "latitude": 5, "longitude": 7})):
        path = str(tmp_path / name)
        af.dataset_to_zarr(ds, path, var="t2m", chunks=chunks, compress="zlib", zarr_format=2)
        n_chunks = -(-T // chunks["time"]) * -(-ny // chunks["latitude"]) * -(-nx // chunks["longitude"])
        cubes, panels = {}, {}
        for mode in ("1", "0"):
            monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
            calls.clear(); hbm.clear()
            d = af.dataset_from_path(path, "t2m", device="cuda")
            cubes[mode] = d.cube().cpu().numpy()
            assert (_zlib_chunks(calls), sum(hbm)) == ((0, n_chunks) if mode == "1" else (n_chunks, 0))
            w = af.weights_from_objects(d, af.GeoRegions(regions), table=tab)
            panels[mode] = af.aggregate_dataset(dataset=d, weights=w, **spec)
        np.testing.assert_array_equal(cubes["1"], cube)
        np.testing.assert_array_equal(cubes["0"], cubes["1"])
        pd.testing.assert_frame_equal(panels["1"], panels["0"])


def test_store_with_a_chunk_the_gpu_route_does_not_take_finishes_on_the_host_route(torch_cuda, tmp_path, monkeypatch):
    """The store is judged by its first chunk; its third is one that `afcodec_inflate_plan` marks for the host.  A gzip member
    there (which the host's inflate reads) finishes right through the host fallback under AGGFLY_HIP_GPU_DECODE=1.  A stream with a
    preset dictionary takes the same fallback — but no route has its dictionary, so both routes end in the host decoder's error."""
    import gzip
    from aggfly_amd import io as afio
    T, ny, nx = 24 * 10, 8, 10
    ds, cube = _ds(T, ny, nx, np.float32, seed=9)
    path = str(tmp_path / "mixed.zarr")
    af.dataset_to_zarr(ds, path, var="t2m", chunks={"time": 48, "latitude": ny, "longitude": nx}, compress="zlib", zarr_format=2)
    raw = np.ascontiguousarray(cube[96:144]).tobytes()
    chunk = os.path.join(path, "t2m", "2.0.0")
    assert os.path.exists(chunk)
    with open(chunk, "wb") as f:
        f.write(gzip.compress(raw, 4))
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "1")
    assert afio._gpu_decodable(afio.ZarrArray(os.path.join(path, "t2m")), 1)
    calls = _spy(monkeypatch)
    d = af.dataset_from_path(path, "t2m", device="cuda")
    np.testing.assert_array_equal(d.cube().cpu().numpy(), cube)
    assert _zlib_chunks(calls) >= 5
    c = zlib.compressobj(zdict=raw[:512])
    with open(chunk, "wb") as f:
        f.write(c.compress(raw) + c.flush())
    for mode in ("1", "0"):
        monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", mode)
        calls.clear()
        with pytest.raises(codec.CodecError, match="failed"):
            af.dataset_from_path(path, "t2m", device="cuda")
        assert _zlib_chunks(calls) > 0
