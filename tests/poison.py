"""What a result must not depend on: the bytes its scratch, workspace, staging and output buffers held before the call.

`FILLS` names four contents, `filled` makes a buffer of one, and `poisoned_empty` makes `torch.empty` / `torch.empty_like` hand out
such buffers for the length of one test, which poisons everything the package takes from the caching allocator itself
(`FusedPlan._workspace`, the outputs of `run` / `run_temporal` / `CSR.wavg` / `scatter_block`, every buffer of io.py) without
rewriting it.  `POISON_ENTRIES` is the table of the C entries that take caller-owned scratch and of the tests that hold them to it
(tests/test_entry_catalogue_host.py keeps it level with include/aggfly_hip.h).  A helper module: no fixtures, no hooks."""
import struct

import numpy as np

RANDOM_SEED = 20261021
_PERIOD = (1 << 20) + 7                          # bytes of the seeded pattern before it repeats: odd, so no power-of-two stride sees a period

# name -> the bytes the fill repeats (`random`: _PERIOD seeded bytes)
FILLS = {
    "zero": b"\x00",
    "ones": b"\xff",                             # a NaN in every float view, -1 in every integer view
    "plausible": struct.pack("<d", 1.0),         # float64 1.0; the float32 pair (0, 1.875); the int32 pair (0, 1072693248)
    "random": None,
}
_HOST = {}
_DEVICE = {}


def host_pattern(fill: str) -> np.ndarray:
    """One period of ``fill`` as a read-only uint8 array."""
    if fill not in FILLS:
        raise KeyError(f"no fill named {fill!r}: {sorted(FILLS)}")
    if fill not in _HOST:
        if fill == "random":
            a = np.random.default_rng(RANDOM_SEED).integers(0, 256, _PERIOD, dtype=np.uint8)
        else:
            a = np.frombuffer(FILLS[fill], dtype=np.uint8).copy()
        a.setflags(write=False)
        _HOST[fill] = a
    return _HOST[fill]


def filled_host(nbytes: int, fill: str) -> np.ndarray:
    """A fresh, writable uint8 array of ``nbytes`` holding ``fill`` from its first byte on."""
    p, n = host_pattern(fill), int(nbytes)
    if len(p) == 1:
        return np.full(n, p[0], dtype=np.uint8)
    return np.tile(p, -(-n // len(p)))[:n].copy()


def _device_pattern(torch, nbytes, fill, device, make):
    """``nbytes`` of ``fill`` on ``device`` from a cached block that only grows; ``make(shape, **kw)`` allocates (the unpatched torch.empty)."""
    key = (fill, str(device))
    have = _DEVICE.get(key)
    if have is None or have.numel() < nbytes:
        n = max(int(nbytes), 1 << 22)
        host = torch.from_numpy(filled_host(n, fill))
        have = make((n,), dtype=torch.uint8, device=device)
        have.copy_(host)
        _DEVICE[key] = have
    return have[:nbytes]


def filled(torch, nbytes: int, fill: str, device="cuda"):
    """A fresh uint8 tensor of ``nbytes`` on ``device`` holding ``fill`` (the pattern starts at byte 0)."""
    make = getattr(torch.empty, "_unpoisoned", torch.empty)
    out = make((int(nbytes),), dtype=torch.uint8, device=device)
    if nbytes:
        dev = torch.device(device)
        out.copy_(_device_pattern(torch, int(nbytes), fill, dev, make) if dev.type == "cuda" else torch.from_numpy(filled_host(nbytes, fill)))
    return out


def poisoned_empty(monkeypatch, torch, fill: str):
    """While the test runs, every tensor `torch.empty` / `torch.empty_like` return on a GPU or in pinned host memory holds ``fill``.
    ``monkeypatch`` puts both back at the end of the test.  -> a list that receives the byte count of every poisoned tensor."""
    host_pattern(fill)
    real_empty = getattr(torch.empty, "_unpoisoned", torch.empty)
    real_like = getattr(torch.empty_like, "_unpoisoned", torch.empty_like)
    seen = []

    def poison(t):
        if not isinstance(t, torch.Tensor) or t.numel() == 0 or not (t.is_cuda or (t.device.type == "cpu" and t.is_pinned())):
            return t
        raw = torch.tensor([], dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
        n = raw.numel()
        if t.is_cuda:
            raw.copy_(_device_pattern(torch, n, fill, t.device, real_empty))
            # the fill is queued on the stream that is current here; the caller may first touch its fresh block on another stream
            # without waiting for this one (nothing of its own is pending there), so the fill must have landed before it returns
            torch.cuda.current_stream(t.device).synchronize()
        else:
            raw.copy_(torch.from_numpy(filled_host(n, fill)))
        seen.append(n)
        return t

    def empty(*a, **k):
        return poison(real_empty(*a, **k))

    def empty_like(*a, **k):
        return poison(real_like(*a, **k))

    empty._unpoisoned, empty_like._unpoisoned = real_empty, real_like
    monkeypatch.setattr(torch, "empty", empty)
    monkeypatch.setattr(torch, "empty_like", empty_like)
    return seen


def stale_empty(monkeypatch, torch, block):
    """While the test runs, every uint8 tensor `torch.empty` is asked for on the GPU is the head of ``block`` (a uint8 GPU tensor,
    256-byte aligned as the allocator's are), which nobody refills: each call's scratch holds what the call before left there.
    Everything else `torch.empty` returns is as ever.  -> a list that receives the byte count of every tensor served from the block."""
    real_empty = getattr(torch.empty, "_unpoisoned", torch.empty)
    served = []

    def empty(*a, **k):
        if k.get("dtype") is torch.uint8 and torch.device(k.get("device", "cpu")).type == "cuda" and len(a) == 1:
            n = int(a[0][0] if isinstance(a[0], (tuple, list)) else a[0])
            if n > block.numel():
                raise AssertionError(f"the stale block holds {block.numel()} bytes, {n} were asked for")
            served.append(n)
            return block[:n]
        return real_empty(*a, **k)

    empty._unpoisoned = real_empty
    monkeypatch.setattr(torch, "empty", empty)
    return served


# Every afhip_* entry of include/aggfly_hip.h that takes caller-owned scratch (a parameter named scratch_dev, workspace_dev, rank_dev,
# tmp_dev or slots_dev): entry -> (the test file that holds it to the four fills, the sequences it is held to there).
POISON_ENTRIES = {
    "afhip_delta_decode": ("test_gpu_poison_codecs.py", "fills, stale A-B-A-A"),
    "afhip_grib_unpack": ("test_gpu_poison_codecs.py", "fills, stale A-B-A-A"),
    "afhip_grib_unpack_complex": ("test_gpu_poison_codecs.py", "fills, stale A-B-A-A"),
    "afhip_grib_unpack_ccsds": ("test_gpu_poison_codecs.py", "fills, stale A-B-A-A"),
    "afhip_lz4_decode_streams": ("test_gpu_poison_codecs.py", "fills (tmp)"),
    "afhip_unshuffle_blocks": ("test_gpu_poison_codecs.py", "fills (tmp, through lz4_decode_streams)"),
    "afhip_bitunshuffle_blocks": ("test_gpu_poison_codecs.py", "fills (tmp, through lz4_decode_streams)"),
    "afhip_shuffle_blocks": ("test_gpu_poison_routes.py", "fills (tmp is its output: dataset_to_zarr(encode='gpu'))"),
    "afhip_lz4_encode_streams": ("test_gpu_poison_codecs.py", "fills (slots)"),
    "afhip_zstd_encode_blocks": ("test_gpu_poison_codecs.py", "fills, stale A-B-A-A"),
    "afhip_zstd_decode": ("test_gpu_poison_codecs.py", "fills, stale A-B-A-A"),
    "afhip_inflate_decode": ("test_gpu_poison_codecs.py", "fills, stale A-B-A-A"),
    "afhip_plan_run_temporal": ("test_gpu_poison_plan.py", "fills, explicit workspace"),
    "afhip_plan_run": ("test_gpu_poison_plan.py", "fills, explicit workspace, reuse sequence"),
}
