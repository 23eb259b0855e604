"""The pass text the host shares with the GPU (zstd_passes.h, inflate_passes.h, run by `codec.zstd_emulate` / `codec.inflate_emulate`)
reads no byte of its scratch that it has not written in the same call: over the whole catalogue, the fuzz and every damaged case
(tests/poison_batches.py) the output image, the error count and the pointer-jump rounds are the same under the four fills of
tests/poison.py, and a batch run in the scratch an earlier, different batch left gives what it gives alone.  The image is the case
writers' own expectation.  The other emulations (`lz4_encode_emulate`, `zstd_encode_block_emulate`, `aec_decode`,
`lzw_decode_ranges`) take no scratch from their caller: there is nothing to poison."""
import numpy as np
import pytest

import poison
import poison_batches as pb

from aggfly_amd import codec

KINDS = {"zstd": pb.zstd_batches, "inflate": pb.inflate_batches}


def test_the_fills_are_what_they_are_named_for():
    assert set(poison.FILLS) == {"zero", "ones", "plausible", "random"}
    z, o, p, r = (poison.filled_host(4099, f) for f in ("zero", "ones", "plausible", "random"))
    assert not z.any() and (o == 0xFF).all() and np.isnan(o[:4096].view(np.float32)).all() and np.isnan(o[:4096].view(np.float64)).all()
    assert (p[:4096].view(np.float64) == 1.0).all() and (p[:8].view(np.float32) == [0.0, 1.875]).all() and (p[:4096].view(np.int32)[1::2] > 0).all()
    assert len(np.unique(r)) == 256 and np.array_equal(r, poison.filled_host(4099, "random")) and z.flags.writeable and r.flags.writeable
    big = poison.filled_host(poison._PERIOD + 5, "random")
    assert np.array_equal(big[-5:], big[:5])


def test_the_default_scratch_is_fresh_and_zeroed_and_a_bad_one_is_refused():
    b = pb.zstd_batches()["B"]
    out, errors, rounds = pb.emulate("zstd", b)
    assert errors == 0 and np.array_equal(out, b.want)
    for bad in (np.zeros(b.plan.scratch_bytes() - 1, dtype=np.uint8), np.zeros(b.plan.scratch_bytes(), dtype=np.int8),
                np.zeros(2 * b.plan.scratch_bytes(), dtype=np.uint8)[::2]):
        with pytest.raises(ValueError, match="scratch"):
            codec.zstd_emulate(b.base, *b.records, b.plan, np.zeros(b.nout, dtype=np.uint8), scratch=bad)


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_the_emulation_is_a_function_of_its_inputs_under_every_fill(kind, which):
    b = KINDS[kind]()[which]
    n = b.plan.scratch_bytes()
    first = pb.emulate(kind, b, poison.filled_host(n, "random"))
    again = pb.emulate(kind, b, poison.filled_host(n, "random"))
    assert first[1:] == again[1:] and np.array_equal(first[0], again[0])
    assert first[1] == b.errors and np.array_equal(first[0], b.want)
    for fill in ("zero", "ones", "plausible"):
        out, errors, rounds = pb.emulate(kind, b, poison.filled_host(n + 64, fill))          # a scratch larger than needed
        assert (errors, rounds) == first[1:] and np.array_equal(out, first[0]), fill


@pytest.mark.parametrize("fill", ["random", "plausible"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_a_batch_in_the_scratch_another_batch_left(kind, fill):
    """A (catalogue, fuzz, every damaged case: bad flags and half-built tables stay behind), then B in the same scratch, nothing
    refilled: B alone.  Then A, and A again: A."""
    A, B = KINDS[kind]()["A"], KINDS[kind]()["B"]
    assert A.errors >= 20 and B.errors == 0 and B.plan.scratch_bytes() < A.plan.scratch_bytes()
    alone = {b.name: pb.emulate(kind, b) for b in (A, B)}
    assert all(np.array_equal(alone[b.name][0], b.want) and alone[b.name][1] == b.errors for b in (A, B))
    scratch = poison.filled_host(A.plan.scratch_bytes(), fill)
    for b in (A, B, A, A):
        out, errors, rounds = pb.emulate(kind, b, scratch)
        assert (errors, rounds) == alone[b.name][1:] and np.array_equal(out, alone[b.name][0]), b.name
