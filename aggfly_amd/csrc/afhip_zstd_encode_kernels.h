// afhip_zstd_encode_kernels.h — Zstandard block ENCODE in HBM for the write side of the ingestion path (io.dataset_to_zarr,
// compress="blosc-zstd", encode="gpu"): the place of k_lz4_encode_streams between k_shuffle_blocks and k_copy_ranges
// (afhip_lz4_encode_kernels.h).
//
//   k_zstd_encode_tables  once per launch of the encoder: the encoding tables of the three predefined sequence codes
//                         (afze_build_tables) into the head of the scratch;
//   k_zstd_encode_blocks  one wave per block (a byte plane of a shuffled Blosc block, or a 128 KiB piece) through the encoder of
//                         zstd_encode_pass.h into the block's own slot of n + 3 bytes; its size to csize[block].
//
// No kernel waits for another workgroup; the tables are read only after the launch that wrote them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zstd_encode_pass.h"

namespace afhip {

struct ZstdEncodeBlock {    // == afhip_zstd_encode_block
    int64_t src_off, dst_off, scratch_off;
    int32_t n, last;
};

__global__ __launch_bounds__(64) void k_zstd_encode_tables(uint8_t* __restrict__ scratch) {
    if (threadIdx.x == 0 && blockIdx.x == 0) afze_build_tables(scratch);
}

// One wave per workgroup, one workgroup per block; the grid is (up to 65,535, rows of 65,535).  LDS: AFZE_LDS_WORDS words (19.3 KiB:
// eight waves a CU).  The first AFZE_TAB_BYTES of the scratch hold the launch's tables; every block's own scratch lies behind them
// at its record's scratch_off.
__global__ __launch_bounds__(64) void k_zstd_encode_blocks(const uint8_t* in, const ZstdEncodeBlock* __restrict__ blocks, int64_t n_blocks,
                                                           uint8_t* scratch, uint8_t* slots, int32_t* __restrict__ csize) {
    __shared__ uint32_t lds[AFZE_LDS_WORDS];
    const int64_t i = (int64_t)blockIdx.y * 65535 + blockIdx.x;
    if (i >= n_blocks) return;                              // (the whole workgroup: no barrier is left waiting)
    const ZstdEncodeBlock b = blocks[i];
    const int32_t c = afze_encode_block(in + b.src_off, b.n, b.last, slots + b.dst_off, scratch + b.scratch_off, scratch, lds, (int)threadIdx.x);
    if (threadIdx.x == 0) csize[i] = c;
}

}  // namespace afhip
