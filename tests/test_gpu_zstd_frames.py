"""The Zstandard kernels (`k_zstd_tables` ... `k_zstd_gather`, afhip_zstd_kernels.h) held to the hand-built frames of
tests/zstd_frames.py, placed by `layout` with no padding: the catalogue and 300 fuzzed frames decode in HBM to the bytes their
descriptions mean (`expand`; libzstd is not needed here), the frames named for launch geometry also one per launch, the pointer-jump
bound on the two offset-1 chains, and damaged frames between valid ones counted as the host emulation counts them."""
import time

import numpy as np
import pytest

import zstd_frames as zs

from aggfly_amd import codec

pytestmark = pytest.mark.gpu
FILL = 0xAB


@pytest.fixture(scope="module")
def valid():
    cat = zs.catalogue()
    frames = [(n, zs.build(fd), zs.expand(fd)) for n, fd in [(n, fd) for n, _, fd in cat] + zs.fuzz(zs.FUZZ_COUNT, zs.FUZZ_SEED)]
    return frames, len(cat)


def _gpu_zstd(torch, frames, sizes):
    """`_gpu_zstd` of test_gpu_zstd_decode.py with `layout` in place of `pack` -> (plan, out bytes on the host, out_off, errors,
    rounds, (base, frame records, block records, out bytes))."""
    from aggfly_amd import hip
    sizes = np.asarray(sizes, dtype=np.int64)
    base, co, cs, oo, nout = zs.layout(frames, sizes)
    assert co[0] == 0 and co[-1] + cs[-1] == base.size
    fr, bl = np.zeros(len(frames) + 1, dtype=codec.ZSTD_FRAME), np.zeros(8192, dtype=codec.ZSTD_BLOCK)
    p = codec.zstd_plan(base, co, cs, oo, sizes, fr, bl, strict=False)
    comp = torch.from_numpy(base).cuda()
    frd = torch.from_numpy(fr[:max(p.n_frames, 1)].view(np.uint8).copy()).cuda()
    bld = torch.from_numpy(bl[:max(p.n_blocks, 1)].view(np.uint8).copy()).cuda()
    out = torch.full((nout,), FILL, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(hip.zstd_scratch_bytes(p), dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    rounds = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.zstd_decode(comp, base.nbytes, frd, bld, p, scratch, out, errors, rounds)
    torch.cuda.synchronize()
    return p, out.cpu().numpy(), oo, int(errors.item()), int(rounds.item()), (base, fr, bl, nout)


def _expected(nout, oo, raws):
    want = np.full(nout, FILL, dtype=np.uint8)
    for o, r in zip(oo, raws):
        want[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    return want


def _exact(torch, items):
    """The whole output buffer, canaries included."""
    raws = [r for _, _, r in items]
    p, host, oo, nerr, rounds, (_, _, _, nout) = _gpu_zstd(torch, [f for _, f, _ in items], [len(r) for r in raws])
    assert nerr == 0 and (p.results == [len(r) for r in raws]).all()
    want = _expected(nout, oo, raws)
    if not np.array_equal(host, want):
        bad = [n for (n, _, r), o in zip(items, oo) if host[o:o + len(r)].tobytes() != r]
        raise AssertionError(("frames that differ", bad[:10], "canaries intact", bool((host[want == FILL] == FILL).all())))
    return p, rounds


def test_catalogue_in_one_batch(torch_cuda, valid):
    frames, ncat = valid
    t0 = time.perf_counter()
    p, rounds = _exact(torch_cuda, frames[:ncat])
    print("catalogue: %d frames, %d blocks, %d bytes, %d pointer-jump rounds, %.2f s" % (ncat, p.n_blocks, p.dec_bytes, rounds, time.perf_counter() - t0))


@pytest.mark.parametrize("name", zs.LAUNCH_GEOMETRY)
def test_launch_geometry_frames_one_per_launch(torch_cuda, valid, name):
    frames, _ = valid
    _exact(torch_cuda, [next(x for x in frames if x[0] == name)])


def test_65_frames_put_the_frames_pass_past_one_workgroup(torch_cuda, valid):
    frames, _ = valid
    items = [x for x in frames if x[0] in ("block-raw", "block-rle", "block-nseq-0", "literals-huf-1-stream", "tree-depth-11")]
    items = (items * 13)[:65]
    p, _ = _exact(torch_cuda, items)
    assert p.n_frames == 65 == p.n_blocks


@pytest.mark.parametrize("names", [("literals-huf-1-stream", "block-raw", "rep0-minus-1-three-times"), ("nseq-127", "literals-huf-4-streams-23")])
def test_first_frame_at_byte_0_and_last_frame_flush_with_the_buffer_end(torch_cuda, valid, names):
    """`afz_ld64`'s byte-wise arm: the last stream of the batch ends on the buffer's last bytes, in a word that is not whole."""
    frames, _ = valid
    items = [next(x for x in frames if x[0] == n) for n in names]
    assert sum(len(f) for _, f, _ in items) % 8 != 0
    _exact(torch_cuda, items)


def test_fuzz_in_one_batch(torch_cuda, valid):
    frames, ncat = valid
    assert len(frames) - ncat == 300
    t0 = time.perf_counter()
    p, rounds = _exact(torch_cuda, frames[ncat:])
    print("fuzz: 300 frames, %d blocks, %d bytes, %d pointer-jump rounds, %.2f s" % (p.n_blocks, p.dec_bytes, rounds, time.perf_counter() - t0))


def _rounds_host(n):
    """afz_rounds_host of zstd_passes.h: ceil(log2 n) + 1."""
    r = 1
    while (1 << (r - 1)) < n and r < 40:
        r += 1
    return r


@pytest.mark.parametrize("name", zs.JUMP_BOUND)
def test_pointer_jump_bound_on_an_offset_1_chain_as_long_as_the_frame(torch_cuda, valid, name):
    """The host emulation visits bytes in ascending order and resolves such a chain in one round; only the GPU's rounds are rounds."""
    frames, _ = valid
    item = next(x for x in frames if x[0] == name)
    assert len(item[2]) in (1 << 18, (1 << 18) + 1) and item[2] == item[2][:1] * len(item[2])
    p, rounds = _exact(torch_cuda, [item])
    print("%s: %d bytes, %d pointer-jump rounds on the GPU, afz_rounds_host %d" % (name, p.dec_bytes, rounds, _rounds_host(p.dec_bytes)))
    assert 1 <= rounds <= _rounds_host(p.dec_bytes)


def test_damaged_frames_between_valid_ones(torch_cuda, valid):
    """Every damaged frame has passed the host emulation's bounds checks under the sanitizers (`make zstd_frames_check_san`)."""
    frames, _ = valid
    good = [x for x in frames if x[0] in ("block-raw", "literals-huf-1-stream", "rep0-minus-1-three-times", "treeless-after-1-block")]
    batch, is_damaged = [], []
    for i, (name, _, fb, n) in enumerate(zs.damaged()):
        batch.append(good[i % len(good)])
        is_damaged.append(False)
        batch.append((name, fb, bytes(n)))
        is_damaged.append(True)
    batch.append(good[0])
    is_damaged.append(False)
    sizes = [len(r) for _, _, r in batch]
    p, host, oo, nerr, _, (base, fr, bl, nout) = _gpu_zstd(torch_cuda, [f for _, f, _ in batch], sizes)
    emu = np.full(nout, FILL, dtype=np.uint8)
    want_err, _ = codec.zstd_emulate(base, fr, bl, p, emu)
    planned = int((p.results[is_damaged] >= 0).sum())
    assert nerr == want_err == planned and planned >= 20
    canary = np.ones(nout, dtype=bool)
    for (name, _, raw), o, bad in zip(batch, oo, is_damaged):
        canary[o:o + len(raw)] = False
        if bad:                                                  # refused before the gather: nothing of it, or of its neighbour, is written
            assert (host[o:o + len(raw)] == FILL).all(), name
        else:
            assert host[o:o + len(raw)].tobytes() == raw, name
    assert (host[canary] == FILL).all()
    assert np.array_equal(host, emu)
