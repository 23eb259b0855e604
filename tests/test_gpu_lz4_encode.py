"""Chunk ENCODE in HBM (aggfly_amd/csrc/afhip_lz4_encode_kernels.h) on the GPU: `k_lz4_encode_streams` byte for byte against the host
emulation of the same text (`afcodec_lz4_encode_emulate`) over the catalogue of tests/lz4_encode_cases.py, every slot between guard
bytes and whole buffers compared; `afhip_take_box`, `afhip_shuffle_blocks` and `afhip_copy_ranges` against numpy; and the public route
— `dataset_to_zarr(..., encode="gpu")` and `zarr_from_path(..., device="cuda", encode="gpu")` — read back on both decode routes."""
import filecmp
import os
import sys

import numpy as np
import pandas as pd
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import lz4_encode_cases as cases_mod            # noqa: E402

import aggfly_amd as af                         # noqa: E402
from aggfly_amd import codec, io as afio        # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
FILL = 0xAB


@pytest.fixture(scope="module")
def emulated():
    """[(name, input, the emulation's stream)] once for the module."""
    return [(name, data, codec.lz4_encode_emulate(data)) for name, data, _ in cases_mod.catalogue()]


def _launch(torch, items):
    """One `hip.lz4_encode_streams` call over ``items`` = [(name, input, expected stream)]: the inputs packed one after the other, the
    slots between guards.  -> (slots image from the GPU, expected image, csize from the GPU, expected csize)."""
    from aggfly_amd import hip
    rec = np.zeros(len(items), dtype=codec.LZ4_STREAM)
    src_off = dst_off = 0
    for i, (_, data, _) in enumerate(items):
        dst_off += GUARD
        rec[i] = (src_off, dst_off, 0, len(data), 0, 0)
        src_off += len(data)
        dst_off += len(data)
    inp = np.frombuffer(b"".join(d for _, d, _ in items) + b"\0", dtype=np.uint8)
    image = np.full(dst_off + GUARD, FILL, dtype=np.uint8)
    for r, (_, _, want) in zip(rec, items):
        image[r["dst_off"]:r["dst_off"] + len(want)] = np.frombuffer(want, dtype=np.uint8)
    slots = torch.full((len(image),), FILL, dtype=torch.uint8, device="cuda")
    csize = torch.full((len(items),), -1, dtype=torch.int32, device="cuda")
    hip.lz4_encode_streams(torch.from_numpy(inp.copy()).cuda(), torch.from_numpy(rec.view(np.uint8).copy()).cuda(), len(rec), slots, csize)
    torch.cuda.synchronize()
    return slots.cpu().numpy(), image, csize.cpu().numpy(), np.array([len(w) for _, _, w in items], dtype=np.int32)


def _assert_same(items, got, image, csize, want_csize):
    bad = np.nonzero(csize != want_csize)[0]
    assert not len(bad), [(items[i][0], int(csize[i]), int(want_csize[i])) for i in bad[:5]]
    ne = np.nonzero(got != image)[0]
    assert not len(ne), f"first difference at byte {ne[0]} of the slots image: {got[ne[0]]} for {image[ne[0]]}"


def test_kernel_bytes_are_the_emulations_over_the_catalogue(torch_cuda, emulated):
    got, image, csize, want = _launch(torch_cuda, emulated)
    _assert_same(emulated, got, image, csize, want)
    assert (want < np.array([len(d) for _, d, _ in emulated])).sum() > 300        # (most cases really compress)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_launches_of_1_64_and_65_streams(torch_cuda, emulated, n):
    small = [e for e in emulated if len(e[1]) <= 6000]
    items = small[40:40 + n]                                                     # (past the length cases: mixes, literal runs, match lengths)
    assert len(items) == n
    _assert_same(items, *_launch(torch_cuda, items))


def test_a_stored_stream_on_request(torch_cuda):
    """`to_out` != 0: the stored chunk of a buffer under 128 bytes — the raw bytes, whatever they would compress to."""
    from aggfly_amd import hip
    torch = torch_cuda
    rec = np.zeros(1, dtype=codec.LZ4_STREAM)
    rec[0] = (0, GUARD, 0, 100, 1, 0)
    slots = torch.full((100 + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    csize = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.lz4_encode_streams(torch.full((100,), 7, dtype=torch.uint8, device="cuda"), torch.from_numpy(rec.view(np.uint8).copy()).cuda(), 1, slots, csize)
    got = slots.cpu().numpy()
    assert int(csize.item()) == 100 and (got[GUARD:GUARD + 100] == 7).all() and (got[:GUARD] == FILL).all() and (got[GUARD + 100:] == FILL).all()


NP_OF = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.float64}


@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_take_box_against_numpy(torch_cuda, elem):
    """Every chunk of three grids over a (50, 13, 10) cube: chunks that stick out on the time, y and x edges are padded with the fill."""
    from aggfly_amd import hip
    torch = torch_cuda
    rng = np.random.default_rng(elem)
    cube = rng.integers(1, 120, (50, 13, 10)).astype(NP_OF[elem])
    fill = np.nan if elem >= 4 else 0
    fill_bits = int(np.array([fill], dtype=NP_OF[elem]).view(f"u{elem}")[0])
    dev = torch.from_numpy(cube).cuda()
    for chunks in ((24, 13, 10), (50, 5, 4), (7, 6, 3), (64, 16, 16)):
        for idx in np.ndindex(*[-(-s // c) for s, c in zip(cube.shape, chunks)]):
            at = tuple(i * c for i, c in zip(idx, chunks))
            box = tuple(min(c, s - a) for c, s, a in zip(chunks, cube.shape, at))
            want = np.full(chunks, fill, dtype=cube.dtype)
            want[:box[0], :box[1], :box[2]] = cube[at[0]:at[0] + box[0], at[1]:at[1] + box[1], at[2]:at[2] + box[2]]
            got = torch.zeros(chunks, dtype=dev.dtype, device="cuda")
            hip.take_box(dev, got, at, box, fill_bits)
            assert got.cpu().numpy().tobytes() == want.tobytes(), (chunks, idx)
    with pytest.raises(ValueError):
        hip.take_box(dev, torch.zeros((4, 4, 4), dtype=dev.dtype, device="cuda"), (0, 10, 0), (4, 4, 4), 0)     # beyond the cube's rows


def test_shuffle_blocks_against_numpy(torch_cuda):
    """Typesizes 1, 2, 4, 8, blocks with trailing bytes, aligned and odd sources, sizes around the tile of 256 threads and its stride."""
    from aggfly_amd import hip
    torch = torch_cuda
    rng = np.random.default_rng(5)
    rec, off = [], 0
    for ts in (1, 2, 4, 8):
        for bsize in (ts, 7 * ts + ts - 1, 256 * ts, 257 * ts + (1 if ts > 1 else 0), 64 * 256 * ts + 3 * ts, 65536):
            for shift in (0, 1):
                off += shift
                rec.append((off, off, bsize, ts))
                off += bsize
    rec = np.array(rec, dtype=codec.SHUFFLE_BLOCK)
    src = rng.integers(0, 256, off + 16, dtype=np.uint8)
    want = np.full(len(src), FILL, dtype=np.uint8)
    for r in rec:
        ts, bs, o = int(r["typesize"]), int(r["bsize"]), int(r["out_off"])
        ne = bs // ts
        want[o:o + ne * ts] = src[o:o + ne * ts].reshape(ne, ts).T.reshape(-1)
        want[o + ne * ts:o + bs] = src[o + ne * ts:o + bs]
    tmp = torch.full((len(src),), FILL, dtype=torch.uint8, device="cuda")
    hip.shuffle_blocks(torch.from_numpy(src).cuda(), tmp, torch.from_numpy(rec.view(np.uint8).copy()).cuda(), len(rec), int(rec["bsize"].max()))
    assert tmp.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        hip.shuffle_blocks(tmp, tmp, tmp, 65536, 4)


def test_copy_ranges_against_numpy(torch_cuda):
    from aggfly_amd import hip
    torch = torch_cuda
    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, 300000, dtype=np.uint8)
    rec, dst_off = [], 0
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 1023, 1024, 1025, 4099, 65536, 100001):
        for shift in (0, 1, 2, 3):
            dst_off += 4 + shift                                                 # (the gap of a stream's length field, every alignment)
            rec.append((int(rng.integers(0, len(src) - n)), dst_off, n))
            dst_off += n
    rec = np.array(rec, dtype=codec.COPY_RANGE)
    want = np.full(dst_off + 8, FILL, dtype=np.uint8)
    for r in rec:
        want[r["dst_off"]:r["dst_off"] + r["n"]] = src[r["src_off"]:r["src_off"] + r["n"]]
    dst = torch.full((len(want),), FILL, dtype=torch.uint8, device="cuda")
    hip.copy_ranges(torch.from_numpy(src).cuda(), dst, torch.from_numpy(rec.view(np.uint8).copy()).cuda(), len(rec))
    assert dst.cpu().numpy().tobytes() == want.tobytes()


def _dataset(cube):
    T, ny, nx = cube.shape
    return af.Dataset(af.DataArray(cube, ["time", "latitude", "longitude"],
                                   {"time": pd.date_range("2001-01-01", periods=T, freq="h"),
                                    "latitude": 30 + 0.25 * np.arange(ny), "longitude": 250 + 0.25 * np.arange(nx)}), lon_is_360=True)


def _cube(dtype):
    rng = np.random.default_rng(11)
    cube = (280 + np.cumsum(rng.normal(0, 0.3, (50, 13, 10)), axis=0)).astype(dtype)
    cube[rng.random(cube.shape) < 0.05] = np.nan
    cube[:, 3, 4] = np.nan
    return cube


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


METADATA = (".zarray", ".zattrs", ".zgroup", ".zmetadata", "zarr.json")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("zarr_format,shards", [(2, None), (3, None), (3, {"time": 14, "latitude": 12, "longitude": 6})], ids=["v2", "v3", "v3-sharded"])
@pytest.mark.parametrize("chunks", [(24, 13, 10), (50, 5, 4), (7, 6, 3)], ids=lambda c: "x".join(map(str, c)))
def test_gpu_written_stores_read_back_bit_for_bit(torch_cuda, tmp_path, monkeypatch, dtype, zarr_format, shards, chunks):
    if shards is not None and chunks != (7, 6, 3):
        shards = {"time": 2 * chunks[0], "latitude": chunks[1], "longitude": 2 * chunks[2]}
    cube = _cube(dtype)
    ch = dict(zip(("time", "latitude", "longitude"), chunks))
    monkeypatch.setattr(afio, "GPU_ENCODE_BATCH_BYTES", 3 * int(np.prod(chunks)) * cube.itemsize)    # three chunks a batch: several batches
    gpu, host = str(tmp_path / "gpu.zarr"), str(tmp_path / "host.zarr")
    af.dataset_to_zarr(_dataset(cube).to_device(), gpu, var="t2m", chunks=ch, zarr_format=zarr_format, shards=shards, encode="gpu")
    af.dataset_to_zarr(_dataset(cube), host, var="t2m", chunks=ch, zarr_format=zarr_format, shards=shards, encode="host")
    assert _files(gpu) == _files(host)
    for f in _files(host):
        if os.path.basename(f) in METADATA or not f.startswith("t2m"):          # metadata, and the coordinate arrays whole
            assert filecmp.cmp(os.path.join(gpu, f), os.path.join(host, f), shallow=False), f
    back = af.dataset_from_path(gpu, "t2m", lon_is_360=True).cube()
    assert back.dtype == cube.dtype and np.asarray(back).tobytes() == cube.tobytes()
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "1")
    dev = af.dataset_from_path(gpu, "t2m", lon_is_360=True, device="cuda").cube().cpu().numpy()
    assert dev.dtype == cube.dtype and dev.tobytes() == cube.tobytes()


def test_integer_cube_and_host_resident_dataset(torch_cuda, tmp_path):
    """An int16 cube from a host-resident dataset: uploaded first; edge chunks padded with 0."""
    cube = np.random.default_rng(2).integers(-300, 300, (50, 13, 10)).astype(np.int16)
    p = str(tmp_path / "i16.zarr")
    af.dataset_to_zarr(_dataset(cube), p, var="q", chunks={"time": 7, "latitude": 6, "longitude": 3}, encode="gpu")
    za = afio.ZarrArray(os.path.join(p, "q"))
    assert za.read().tobytes() == cube.tobytes()
    edge = codec.blosc_decode(open(os.path.join(p, "q", "7.2.3"), "rb").read()).view(np.int16).reshape(7, 6, 3)
    assert (edge[1:] == 0).all() and (edge[:, 1:] == 0).all() and (edge[:, :, 1:] == 0).all()


def test_what_the_gpu_route_does_not_take_is_named(torch_cuda, tmp_path):
    ds = _dataset(_cube(np.float32)).to_device()
    with pytest.raises(ValueError, match="zstd"):
        af.dataset_to_zarr(ds, str(tmp_path / "z.zarr"), var="t2m", compress="zstd", encode="gpu")
    with pytest.raises(ValueError, match="encode"):
        af.dataset_to_zarr(ds, str(tmp_path / "z.zarr"), var="t2m", encode="device")


def test_host_and_default_write_the_same_store_and_the_environment_opts_in(torch_cuda, tmp_path, monkeypatch):
    cube = _cube(np.float32)
    ch = {"time": 24, "latitude": 13, "longitude": 10}
    monkeypatch.delenv("AGGFLY_HIP_GPU_ENCODE", raising=False)
    assert afio.GPU_ENCODE_AUTO_BYTES is None or afio.GPU_ENCODE_AUTO_BYTES > cube.nbytes
    a, b, c, g = (str(tmp_path / n) for n in ("default.zarr", "host.zarr", "env.zarr", "gpu.zarr"))
    af.dataset_to_zarr(_dataset(cube).to_device(), a, var="t2m", chunks=ch)
    af.dataset_to_zarr(_dataset(cube).to_device(), b, var="t2m", chunks=ch, encode="host")
    assert _files(a) == _files(b) and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False) for f in _files(a))
    monkeypatch.setenv("AGGFLY_HIP_GPU_ENCODE", "1")
    af.dataset_to_zarr(_dataset(cube).to_device(), c, var="t2m", chunks=ch)
    af.dataset_to_zarr(_dataset(cube).to_device(), g, var="t2m", chunks=ch, encode="gpu")
    assert all(filecmp.cmp(os.path.join(c, f), os.path.join(g, f), shallow=False) for f in _files(g))
    assert not filecmp.cmp(os.path.join(c, "t2m", "0.0.0"), os.path.join(b, "t2m", "0.0.0"), shallow=False)      # (the GPU encoder's streams)


def test_zarr_from_path_on_the_device(torch_cuda, tmp_path):
    cube = _cube(np.float32)
    src, dst = str(tmp_path / "src.zarr"), str(tmp_path / "dst.zarr")
    af.dataset_to_zarr(_dataset(cube), src, var="t2m", chunks={"time": 24, "latitude": 13, "longitude": 10})
    afio.zarr_from_path(src, dst, "t2m", device="cuda", encode="gpu", lon_is_360=True, chunks={"time": 50, "latitude": 5, "longitude": 4})
    back = af.dataset_from_path(dst, "t2m", lon_is_360=True).cube()
    assert np.asarray(back).tobytes() == cube.tobytes()


def test_a_packed_dataset_writes_its_float32_values(torch_cuda, tmp_path):
    """`keep_packed`: the cube in HBM is the stored int16; both routes write the materialised float32 values."""
    import json
    T, ny, nx = 48, 8, 12
    rng = np.random.default_rng(8)
    stored = rng.integers(-30000, 30000, (T, ny, nx)).astype(np.int16)
    stored[rng.random((T, ny, nx)) < 0.02] = -32767
    attrs = {"scale_factor": 0.0017, "add_offset": 281.3, "_FillValue": -32767}
    tv, tattrs = afio._encode_time(pd.date_range("2004-03-01", periods=T, freq="h"))
    src = str(tmp_path / "p.zarr")
    os.makedirs(src)
    json.dump({"zarr_format": 2}, open(os.path.join(src, ".zgroup"), "w"))
    afio._write_array(src, "t2m", stored, ("time", "latitude", "longitude"), (24, 8, 12), attrs, None)
    afio._write_array(src, "time", np.asarray(tv, dtype=np.float64), ("time",), (T,), tattrs, None)
    afio._write_array(src, "latitude", 35 + 0.25 * np.arange(ny), ("latitude",), (ny,), {}, None)
    afio._write_array(src, "longitude", 250 + 0.25 * np.arange(nx), ("longitude",), (nx,), {}, None)
    packed = af.dataset_from_path(src, "t2m", device="cuda", keep_packed=True)
    assert packed.is_packed
    values = packed.cube().cpu().numpy()
    assert values.dtype == np.float32 and np.isnan(values).any()
    gpu, host = str(tmp_path / "gpu.zarr"), str(tmp_path / "host.zarr")
    ch = {"time": 20, "latitude": 5, "longitude": 12}
    af.dataset_to_zarr(packed, gpu, var="t2m", chunks=ch, encode="gpu")
    af.dataset_to_zarr(packed, host, var="t2m", chunks=ch, encode="host")
    for p in (gpu, host):
        back = np.asarray(af.dataset_from_path(p, "t2m").cube())
        assert back.dtype == np.float32 and back.tobytes() == values.tobytes()
    assert filecmp.cmp(os.path.join(gpu, "t2m", ".zarray"), os.path.join(host, "t2m", ".zarray"), shallow=False)
