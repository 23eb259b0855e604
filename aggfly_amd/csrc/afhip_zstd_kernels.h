// afhip_zstd_kernels.h — Zstandard chunk decode in HBM for the ingestion path (Zarr v2 compressor "zstd", Zarr v3
// bytes -> zstd, inside shards too).  The host walks only headers (afcodec_zstd_plan in blosc1.c); the passes are written once in
// zstd_passes.h (where they are described) and run here as launch-ordered kernels over all blocks of a batch: a lane per block
// (tables, sequences), per Huffman stream (literals) or per frame (frames), a wave per block (fill, gather), a lane per output
// byte (jump, ceil(log2 bytes) + 1 launches, each returning at once when the round before it left no work).  No workgroup ever
// waits for another; every dependency is a launch boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zstd_passes.h"

namespace afhip {

constexpr int ZSTD_WG = 64;
constexpr int ZSTD_JUMP_WG = 256;

__global__ __launch_bounds__(ZSTD_WG) void k_zstd_tables(afz_ctx c) {
    afz_pass_tables(&c, (int64_t)blockIdx.x * ZSTD_WG + threadIdx.x);
}

// The Huffman tables of the workgroup's 16 blocks are staged in LDS (64 KiB) first: a lane's symbol loop is a chain of
// dependent table lookups, and 16 tables of 4 KiB per wave served from L2 bound the pass (profiles/zstd_ingest.txt).
__global__ __launch_bounds__(ZSTD_WG) void k_zstd_literals(afz_ctx c) {
    constexpr int NB = ZSTD_WG / 4;
    __shared__ uint16_t tabs[NB][2048];
    const int64_t b0 = (int64_t)blockIdx.x * NB;
    for (int j = 0; j < NB && b0 + j < c.n_blocks; ++j) {
        const afz_block* k = &c.blocks[b0 + j];
        if (k->btype != 2 || k->lit_type < 2 || afz_is_bad(&c, k->frame)) continue;
        const uint16_t* t = (const uint16_t*)(c.slots + (int64_t)k->huf_block * AFZ_SLOT_BYTES + AFZ_SLOT_HUF);
        for (int i = threadIdx.x; i < 2048; i += ZSTD_WG) tabs[j][i] = t[i];
    }
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * ZSTD_WG + threadIdx.x;
    afz_pass_literals(&c, g >> 2, (int)(g & 3), tabs[threadIdx.x >> 2]);
}

__global__ __launch_bounds__(ZSTD_WG) void k_zstd_sequences(afz_ctx c) {
    afz_pass_sequences(&c, (int64_t)blockIdx.x * ZSTD_WG + threadIdx.x);
}

__global__ __launch_bounds__(ZSTD_WG) void k_zstd_frames(afz_ctx c) {
    afz_pass_frame(&c, (int64_t)blockIdx.x * ZSTD_WG + threadIdx.x);
}

__global__ __launch_bounds__(ZSTD_WG) void k_zstd_fill(afz_ctx c) {
    afz_pass_fill(&c, blockIdx.x, threadIdx.x, ZSTD_WG);
}

__global__ __launch_bounds__(ZSTD_JUMP_WG) void k_zstd_jump(afz_ctx c, int r) {
    if (!c.flags[r]) return;                                   // the previous round left nothing to do
    int more = 0;
    const int64_t stride = (int64_t)gridDim.x * ZSTD_JUMP_WG;
    for (int64_t p = (int64_t)blockIdx.x * ZSTD_JUMP_WG + threadIdx.x; p < c.dec_bytes; p += stride) more |= afz_jump(&c, p);
    if (__any(more) && (threadIdx.x & 63) == 0) c.flags[r + 1] = 1;
}

__global__ __launch_bounds__(ZSTD_WG) void k_zstd_gather(afz_ctx c) {
    afz_pass_gather(&c, blockIdx.x, threadIdx.x, ZSTD_WG);
}

// rounds that had work (the logged pointer-jump round count)
__global__ __launch_bounds__(ZSTD_WG) void k_zstd_rounds(afz_ctx c, int R, int32_t* rounds) {
    if (threadIdx.x != 0) return;
    int r = 0;
    while (r < R && c.flags[r]) ++r;
    *rounds = r;
}

}  // namespace afhip
