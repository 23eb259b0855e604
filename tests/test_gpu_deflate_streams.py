"""The deflate kernels (`k_inflate_front` ... `k_inflate_check`, afhip_inflate_kernels.h) held to the hand-built streams of
tests/deflate_streams.py, placed by `layout` with no padding: the catalogue and 300 fuzzed streams decode in HBM to the bytes their
descriptions mean (`expand`; zlib is not needed here), the streams named for launch geometry also one per launch, 65 and 129 streams
in one launch, multi-pseudo-block streams through the shuffle scratch, the pointer-jump bound on the two distance-1 chains, and
damaged streams between valid ones counted as the host emulation counts them."""
import time

import numpy as np
import pytest

import deflate_streams as ds
import inflate_cases as ic

from aggfly_amd import codec

pytestmark = pytest.mark.gpu
FILL = ds.FILL
TAIL = 4096                                      # canary bytes behind the scratch


@pytest.fixture(scope="module")
def valid():
    cat = ds.catalogue()
    streams = [(n, ds.build(d), ds.expand(d)) for n, d in [(n, d) for n, _, d in cat] + ds.fuzz(ds.FUZZ_COUNT, ds.FUZZ_SEED)]
    return streams, len(cat)


def _gpu_inflate(torch, streams, sizes, typesize=1):
    """`_gpu_inflate` of test_gpu_inflate_decode.py with `layout` in place of `pack` -> (plan, out bytes on the host, out_off, errors,
    rounds, (base, stream records, shuffle records, out bytes))."""
    from aggfly_amd import hip
    sizes = np.asarray(sizes, dtype=np.int64)
    base, co, cs, oo, nout = ds.layout(streams, sizes)
    assert co[0] == 0 and co[-1] + cs[-1] == base.size
    st = np.zeros(len(streams) + 1, dtype=codec.INFLATE_STREAM)
    sh = np.zeros(len(streams) + 1, dtype=codec.SHUFFLE_BLOCK)
    p = codec.inflate_plan(base, co, cs, oo, sizes, st, sh, typesize=typesize, strict=False)
    comp = torch.from_numpy(base).cuda()
    std = torch.from_numpy(st[:max(p.n_streams, 1)].view(np.uint8).copy()).cuda()
    shd = torch.from_numpy(sh[:max(p.n_shuf, 1)].view(np.uint8).copy()).cuda()
    out = torch.full((nout,), FILL, dtype=torch.uint8, device="cuda")
    need = hip.inflate_scratch_bytes(p)
    assert need == p.scratch_bytes()
    scratch = torch.full((need + TAIL,), 0xCD, dtype=torch.uint8, device="cuda")
    errors = torch.zeros(1, dtype=torch.int32, device="cuda")
    rounds = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.inflate_decode(comp, base.nbytes, std, shd, p, scratch[:need], out, errors, rounds)
    torch.cuda.synchronize()
    assert (scratch[need:].cpu().numpy() == 0xCD).all(), "the canary behind the scratch was written"
    return p, out.cpu().numpy(), oo, int(errors.item()), int(rounds.item()), (base, st, sh, nout)


def _expected(nout, oo, raws):
    want = np.full(nout, FILL, dtype=np.uint8)
    for o, r in zip(oo, raws):
        want[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    return want


def _exact(torch, items, typesize=1, streams=None):
    """The whole output buffer, canaries included."""
    raws = [r for _, _, r in items]
    p, host, oo, nerr, rounds, (_, _, _, nout) = _gpu_inflate(torch, streams or [s for _, s, _ in items], [len(r) for r in raws], typesize)
    assert nerr == 0 and (p.results == [len(r) for r in raws]).all()
    want = _expected(nout, oo, raws)
    if not np.array_equal(host, want):
        bad = [n for (n, _, r), o in zip(items, oo) if host[o:o + len(r)].tobytes() != r]
        raise AssertionError(("streams that differ", bad[:10], "canaries intact", bool((host[want == FILL] == FILL).all())))
    return p, rounds


def test_catalogue_in_one_launch(torch_cuda, valid):
    streams, ncat = valid
    t0 = time.perf_counter()
    p, rounds = _exact(torch_cuda, streams[:ncat])
    print("catalogue: %d streams, %d pseudo-block slots, %d bytes, %d pointer-jump rounds, %.2f s" % (ncat, p.n_pblocks, p.dec_bytes, rounds, time.perf_counter() - t0))


@pytest.mark.parametrize("name", ds.LAUNCH_GEOMETRY)
def test_launch_geometry_streams_one_per_launch(torch_cuda, valid, name):
    streams, _ = valid
    _exact(torch_cuda, [next(x for x in streams if x[0] == name)])


@pytest.mark.parametrize("n", [65, 129])
def test_many_streams_put_the_check_pass_past_one_and_two_workgroups(torch_cuda, valid, n):
    streams, ncat = valid
    small = [x for x in streams[:ncat] if len(x[2]) < 2000]
    assert len(small) >= 60
    items = (small * 3)[:n]
    p, _ = _exact(torch_cuda, items)
    assert p.n_streams == n and -(-n // 64) == (2 if n == 65 else 3)


@pytest.mark.parametrize("names", [("size-0-smallest-chunk", "chunk-9", "cl-repeat-extremes", "eob-bit-3-chunk-9"),
                                   ("code-lengths-1-to-15-ascending", "hclen-19", "size-0-smallest-chunk")])
def test_first_stream_at_byte_0_and_last_stream_flush_with_the_buffer_end(torch_cuda, valid, names):
    """`afi_ld64`'s byte-wise arm: the last stream of the batch ends on the buffer's last bytes, in a word that is not whole."""
    streams, _ = valid
    items = [next(x for x in streams if x[0] == n) for n in names]
    assert sum(len(s) for _, s, _ in items) % 8 != 0
    _exact(torch_cuda, items)


def test_fuzz_in_one_launch(torch_cuda, valid):
    streams, ncat = valid
    assert len(streams) - ncat == 300
    t0 = time.perf_counter()
    p, rounds = _exact(torch_cuda, streams[ncat:])
    print("fuzz: 300 streams, %d pseudo-block slots, %d bytes, %d pointer-jump rounds, %.2f s" % (p.n_pblocks, p.dec_bytes, rounds, time.perf_counter() - t0))


def test_multi_pseudo_block_streams_through_the_shuffle_scratch(torch_cuda, valid):
    """to_out = 0: the catalogue streams' bytes, shuffled with element size 4 and written again as stored plus fixed blocks."""
    streams, _ = valid
    items = [next(x for x in streams if x[0] == name) for name in ds.MULTI_PBLOCK]
    again = [ds.build(ds.restore(ic.shuffle(r, 4))) for _, _, r in items]
    t0 = time.perf_counter()
    p, _ = _exact(torch_cuda, items, typesize=4, streams=again)
    assert p.n_shuf == 2 and p.n_pblocks >= 4 and p.tmp_bytes >= sum(len(r) for _, _, r in items)
    print("shuffle scratch: 2 streams, %d pseudo-block slots, %d bytes, %.2f s" % (p.n_pblocks, p.dec_bytes, time.perf_counter() - t0))


def _rounds_host(n):
    """afz_rounds_host of zstd_passes.h: ceil(log2 n) + 1."""
    r = 1
    while (1 << (r - 1)) < n and r < 40:
        r += 1
    return r


@pytest.mark.parametrize("name", ds.JUMP_BOUND)
def test_pointer_jump_bound_on_a_distance_1_chain_as_long_as_the_stream(torch_cuda, valid, name):
    """The host emulation visits bytes in ascending order and resolves such a chain in one round; only the GPU's rounds are rounds."""
    streams, _ = valid
    item = next(x for x in streams if x[0] == name)
    assert len(item[2]) in (1 << 18, (1 << 18) + 1) and item[2] == item[2][:1] * len(item[2])
    p, rounds = _exact(torch_cuda, [item])
    print("%s: %d bytes, %d pointer-jump rounds on the GPU, afz_rounds_host %d" % (name, p.dec_bytes, rounds, _rounds_host(p.dec_bytes)))
    assert 1 <= rounds <= _rounds_host(p.dec_bytes)


def test_damaged_streams_between_valid_ones(torch_cuda, valid):
    """Every damaged stream has passed the host emulation's bounds checks under the sanitizers (`make deflate_streams_check_san`).
    The front end refuses all but four of them before a byte is written: their destinations are still the fill byte.  The four with a
    wrong bit in the Adler-32 are found by the check pass, which sums the decoded bytes in the destination: there the decoded bytes
    stay (`damaged`'s last field), and the stream is counted."""
    streams, _ = valid
    good = [x for x in streams if x[0] in ("stored-len-1", "one-distance-code-of-one-bit", "cl-repeat-extremes", "fixed-dynamic-fixed")]
    assert len(good) == 4
    batch, is_damaged = [], []
    for i, (name, _, s, n, _, left) in enumerate(ds.damaged()):
        batch.append(good[i % len(good)])
        is_damaged.append(None)
        batch.append((name, s, bytes(n)))
        is_damaged.append(left or b"")
    batch.append(good[0])
    is_damaged.append(None)
    sizes = [len(r) for _, _, r in batch]
    p, host, oo, nerr, _, (base, st, sh, nout) = _gpu_inflate(torch_cuda, [s for _, s, _ in batch], sizes)
    emu = np.full(nout, FILL, dtype=np.uint8)
    want_err, _ = codec.inflate_emulate(base, st, sh, p, emu)
    planned = int((p.results[[d is not None for d in is_damaged]] >= 0).sum())
    assert nerr == want_err == planned == len(ds.damaged()) >= 40
    canary = np.ones(nout, dtype=bool)
    for (name, _, raw), o, left in zip(batch, oo, is_damaged):
        canary[o:o + len(raw)] = False
        if left is None:
            assert host[o:o + len(raw)].tobytes() == raw, name
        else:
            assert host[o:o + len(raw)].tobytes() == (left or bytes([FILL]) * len(raw)), name
    assert (host[canary] == FILL).all()
    assert np.array_equal(host, emu)
