"""Zstandard block ENCODE in HBM (aggfly_amd/csrc/afhip_zstd_encode_kernels.h) on the GPU: `k_zstd_encode_blocks` byte for byte against
the host emulation of the same text (`afcodec_zstd_encode_block_emulate`) over the catalogue of tests/zstd_encode_cases.py in one launch,
every slot and the scratch between guard bytes; and the public route — `dataset_to_zarr(..., compress="blosc-zstd", encode="gpu")` and
`zarr_from_path(..., device="cuda", encode="gpu", compress="blosc-zstd")` — read back on both decode routes."""
import filecmp
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import zstd_encode_cases as zc                  # noqa: E402

import aggfly_amd as af                         # noqa: E402
from aggfly_amd import codec, io as afio        # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 64
SCRATCH_GUARD = 256                             # (keeps the scratch aligned as the route's own allocation is)
FILL = 0xAB
METADATA = (".zarray", ".zattrs", ".zgroup", ".zmetadata", "zarr.json")
VAR = "var"


def test_kernel_bytes_are_the_emulations_over_the_catalogue(torch_cuda):
    """All blocks of the catalogue in one launch (every other one with the Last_Block bit); nothing but the slots is written in the
    slots image, nothing outside the scratch."""
    from aggfly_amd import hip
    torch = torch_cuda
    items = [(name, data, codec.zstd_encode_block_emulate(data, last=bool(i & 1))) for i, (name, data, _) in enumerate(zc.catalogue())]
    rec = np.zeros(len(items), dtype=codec.ZSTD_ENCODE_BLOCK)
    src_off = dst_off = 0
    scratch_off = hip.load().afhip_zstd_encode_scratch_bytes(0)
    assert scratch_off == codec.load().afcodec_zstd_encode_scratch_bytes(0) and scratch_off % 256 == 0
    for i, (_, data, _) in enumerate(items):
        dst_off += GUARD
        rec[i] = (src_off, dst_off, scratch_off, len(data), i & 1)
        src_off += len(data)
        dst_off += len(data) + 3
        need = hip.load().afhip_zstd_encode_scratch_bytes(len(data))
        assert need == codec.load().afcodec_zstd_encode_scratch_bytes(len(data)) and need % 256 == 0
        scratch_off += need
    inp = np.frombuffer(b"".join(d for _, d, _ in items), dtype=np.uint8)
    image = np.full(dst_off + GUARD, FILL, dtype=np.uint8)
    mask = np.zeros(len(image), dtype=bool)                 # the bytes the blocks own
    for r, (_, _, want) in zip(rec, items):
        image[r["dst_off"]:r["dst_off"] + len(want)] = np.frombuffer(want, dtype=np.uint8)
        mask[r["dst_off"]:r["dst_off"] + len(want)] = True
    slots = torch.full((len(image),), FILL, dtype=torch.uint8, device="cuda")
    csize = torch.full((len(items),), -1, dtype=torch.int32, device="cuda")
    big = torch.full((scratch_off + 2 * SCRATCH_GUARD,), FILL, dtype=torch.uint8, device="cuda")
    hip.zstd_encode_blocks(torch.from_numpy(inp.copy()).cuda(), torch.from_numpy(rec.view(np.uint8).copy()).cuda(), len(rec),
                           big[SCRATCH_GUARD:SCRATCH_GUARD + scratch_off], slots, csize)
    torch.cuda.synchronize()
    got, csize = slots.cpu().numpy(), csize.cpu().numpy()
    want_csize = np.array([len(w) for _, _, w in items], dtype=np.int32)
    bad = np.nonzero(csize != want_csize)[0]
    assert not len(bad), [(items[i][0], int(csize[i]), int(want_csize[i])) for i in bad[:5]]
    ne = np.nonzero(got != image)[0]
    where = items[int(np.searchsorted(rec["dst_off"], ne[0], side="right")) - 1][0] if len(ne) else None
    assert not len(ne), f"first difference at byte {ne[0]} of the slots image ({where}): {got[ne[0]]} for {image[ne[0]]}"
    assert (got[~mask] == FILL).all()                       # guards, and what a block leaves of its slot
    assert (big[:SCRATCH_GUARD] == FILL).all().item() and (big[SCRATCH_GUARD + scratch_off:] == FILL).all().item()
    assert (want_csize < np.array([len(d) for _, d, _ in items])).sum() > 100     # (most cases really compress)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _read_back_both_ways(path, cube, monkeypatch):
    back = af.dataset_from_path(path, VAR, lon_is_360=True).cube()
    assert back.dtype == cube.dtype and np.asarray(back).tobytes() == cube.tobytes()
    monkeypatch.setenv("AGGFLY_HIP_GPU_DECODE", "1")
    dev = af.dataset_from_path(path, VAR, lon_is_360=True, device="cuda").cube().cpu().numpy()
    if cube.dtype.kind == "f":
        assert dev.dtype == cube.dtype and dev.tobytes() == cube.tobytes()
    else:                                                   # (a device-resident dataset holds an integer cube as float32: exact for int16)
        assert dev.dtype == np.float32 and np.array_equal(dev, cube.astype(np.float32))


@pytest.mark.parametrize("zarr_format,shards", [(2, None), (3, None), (3, zc.SMALL_CHUNKS)], ids=["v2", "v3", "v3-sharded"])
def test_gpu_written_blosc_zstd_stores_read_back_bit_for_bit(torch_cuda, tmp_path, monkeypatch, zarr_format, shards):
    """The (100, 37, 29) float32 cube in chunks of (96, 37, 29): a chunk above 256 KiB with a short last Blosc block, and an edge chunk.
    Fails without the feature: the call raised ValueError."""
    ds = zc.small_dataset()
    cube = ds.cube()
    monkeypatch.setattr(afio, "GPU_ENCODE_BATCH_BYTES", 96 * 37 * 29 * 4)        # one chunk a batch: two batches
    gpu, host = str(tmp_path / "gpu.zarr"), str(tmp_path / "host.zarr")
    af.dataset_to_zarr(ds.to_device(), gpu, chunks=zc.SMALL_CHUNKS, compress="blosc-zstd", zarr_format=zarr_format, shards=shards, encode="gpu")
    af.dataset_to_zarr(ds, host, chunks=zc.SMALL_CHUNKS, compress="blosc-zstd", zarr_format=zarr_format, shards=shards, encode="host")
    assert _files(gpu) == _files(host)
    for f in _files(host):
        if os.path.basename(f) in METADATA or not f.startswith(VAR):             # metadata, and the coordinate arrays whole
            assert filecmp.cmp(os.path.join(gpu, f), os.path.join(host, f), shallow=False), f
    if zarr_format == 2:
        chunk = open(os.path.join(gpu, VAR, "0.0.0"), "rb").read()
        info = codec.blosc_info(chunk)
        assert info["nbytes"] == 96 * 37 * 29 * 4 and info["blocksize"] == 262144 and chunk[2] == 0x91      # zstd, unsplit, byte shuffle
        assert chunk[16 + 4 * 2 + 4:][:5] == b"\x28\xb5\x2f\xfd\xa0"              # a frame with the 9-byte header
        assert len(chunk) < 0.95 * info["nbytes"]
    _read_back_both_ways(gpu, cube, monkeypatch)


@pytest.mark.parametrize("dtype,on_host", [("float64", False), ("int16", False), ("float32", True)], ids=["f64", "i16", "f32-host-resident"])
def test_other_dtypes_and_a_host_resident_dataset(torch_cuda, tmp_path, monkeypatch, dtype, on_host):
    ds = zc.small_dataset(dtype)
    cube = ds.cube()
    p = str(tmp_path / "s.zarr")
    af.dataset_to_zarr(ds if on_host else ds.to_device(), p, chunks=zc.SMALL_CHUNKS, compress="blosc-zstd", encode="gpu")
    _read_back_both_ways(p, cube, monkeypatch)


def test_what_the_gpu_route_still_does_not_take_is_named(torch_cuda, tmp_path):
    ds = zc.small_dataset().to_device()
    for compress in ("blosc-zstd-bitshuffle", "zlib", "blosc-bitshuffle", "zstd"):
        with pytest.raises(ValueError, match=compress):
            af.dataset_to_zarr(ds, str(tmp_path / "z.zarr"), compress=compress, encode="gpu")


def test_host_and_default_write_the_same_store_and_the_environment_opts_in(torch_cuda, tmp_path, monkeypatch):
    ds = zc.small_dataset()
    monkeypatch.delenv("AGGFLY_HIP_GPU_ENCODE", raising=False)
    assert afio.GPU_ENCODE_AUTO_BYTES_BLOSC_ZSTD is None or afio.GPU_ENCODE_AUTO_BYTES_BLOSC_ZSTD > ds.cube().nbytes
    a, b, c, g = (str(tmp_path / n) for n in ("default.zarr", "host.zarr", "env.zarr", "gpu.zarr"))
    kw = dict(chunks=zc.SMALL_CHUNKS, compress="blosc-zstd")
    af.dataset_to_zarr(ds.to_device(), a, **kw)
    af.dataset_to_zarr(ds.to_device(), b, encode="host", **kw)
    assert _files(a) == _files(b) and all(filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False) for f in _files(a))
    monkeypatch.setenv("AGGFLY_HIP_GPU_ENCODE", "1")
    af.dataset_to_zarr(ds.to_device(), c, **kw)
    af.dataset_to_zarr(ds.to_device(), g, encode="gpu", **kw)
    assert all(filecmp.cmp(os.path.join(c, f), os.path.join(g, f), shallow=False) for f in _files(g))
    assert not filecmp.cmp(os.path.join(c, VAR, "0.0.0"), os.path.join(b, VAR, "0.0.0"), shallow=False)      # (the GPU encoder's frames)


def test_zarr_from_path_on_the_device(torch_cuda, tmp_path):
    ds = zc.small_dataset()
    src, dst = str(tmp_path / "src.zarr"), str(tmp_path / "dst.zarr")
    af.dataset_to_zarr(ds, src, chunks={"time": 24, "latitude": 37, "longitude": 29})
    afio.zarr_from_path(src, dst, VAR, device="cuda", encode="gpu", compress="blosc-zstd", lon_is_360=True, chunks=zc.SMALL_CHUNKS)
    assert codec.blosc_info(open(os.path.join(dst, VAR, "0.0.0"), "rb").read())["blocksize"] == 262144
    assert np.asarray(af.dataset_from_path(dst, VAR, lon_is_360=True).cube()).tobytes() == ds.cube().tobytes()
