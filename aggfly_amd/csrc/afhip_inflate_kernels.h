// afhip_inflate_kernels.h — zlib (deflate) chunk decode in HBM for the ingestion path (HDF5 / netCDF-4 [deflate] and [shuffle,
// deflate] chunks, Zarr v2 compressor "zlib").  The host reads only the two header bytes of a chunk (afcodec_inflate_plan in
// blosc1.c); the passes are written once in inflate_passes.h (where they are described) and run here as launch-ordered kernels: the
// front end a stream at a time (a wave per stream, its tables in LDS), fill and
// gather a wave per pseudo-block, the pointer jumps by k_zstd_jump (afhip_zstd_kernels.h), the Adler-32 a wave per 64 KiB piece and
// a lane per stream, the unshuffle by k_unshuffle_blocks (afhip_lz4_kernels.h).  No workgroup ever waits for another; every
// dependency is a launch boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "inflate_passes.h"

namespace afhip {

constexpr int INFLATE_WG = 64;

// One stream per wave, walked by its first lane: the symbol loop is a chain of dependent table lookups, and the stream's tables
// (5.25 KiB) answer from LDS instead of L2 (as k_zstd_literals stages its Huffman tables).  Measured against a lane per stream with
// the tables in the scratch, this form was ahead on every layout: 49 against 52 ms on 2,734 chunks of 98 KB, 755 against 1,244 ms on
// 365 chunks of 2.4 MB, 2.66 against 3.58 s on 96 chunks of 9 MB (profiles/deflate_ingest.txt).
__global__ __launch_bounds__(INFLATE_WG) void k_inflate_front(afi_ctx c) {
    __shared__ __attribute__((aligned(16))) uint8_t slot[AFI_SLOT_BYTES];
    if (threadIdx.x == 0) afi_pass_front(&c, blockIdx.x, slot);
}

__global__ __launch_bounds__(INFLATE_WG) void k_inflate_fill(afi_ctx c) {
    afi_pass_fill(&c, blockIdx.x, threadIdx.x, INFLATE_WG);
}

__global__ __launch_bounds__(INFLATE_WG) void k_inflate_gather(afi_ctx c) {
    afi_pass_gather(&c, blockIdx.x, threadIdx.x, INFLATE_WG);
}

__global__ __launch_bounds__(INFLATE_WG) void k_inflate_adler(afi_ctx c) {
    uint32_t a;
    uint64_t b;
    afi_adler_share(&c, blockIdx.x, threadIdx.x, INFLATE_WG, &a, &b);
    for (int d = INFLATE_WG / 2; d > 0; d >>= 1) {
        a += __shfl_down(a, d, INFLATE_WG);
        b += __shfl_down(b, d, INFLATE_WG);
    }
    if (threadIdx.x == 0) afi_adler_put(&c, blockIdx.x, a, b);
}

__global__ __launch_bounds__(INFLATE_WG) void k_inflate_check(afi_ctx c) {
    afi_pass_check(&c, (int64_t)blockIdx.x * INFLATE_WG + threadIdx.x);
}

}  // namespace afhip
