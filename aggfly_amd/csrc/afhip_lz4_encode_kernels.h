// afhip_lz4_encode_kernels.h — chunk ENCODE in HBM for the write side of the ingestion path (io.dataset_to_zarr, encode="gpu"): the
// decode route of afhip_lz4_kernels.h in reverse.  The cube stays in HBM; per batch of chunks
//
//   k_take_box            the box of one chunk out of the time-major cube into the contiguous chunk buffer, whatever lies beyond the
//                         cube filled with the array's fill value (Zarr pads edge chunks): the inverse of k_place_box;
//   k_shuffle_blocks      Blosc's byte shuffle per block, chunk buffer -> shuffle scratch: the inverse of k_unshuffle_blocks, the same
//                         records and launch shape;
//   k_lz4_encode_streams  one wave per stream (a byte plane of a split block, or a whole short block) through the encoder of
//                         lz4_encode_pass.h into the stream's own slot; its size to csize[stream];
//   k_copy_ranges         once the host has read the sizes: every stream from its slot to its place in the batch's packed output
//                         (the Blosc containers, their headers and tables left for the host to fill).
//
// No kernel waits for another workgroup, no kernel reads what it wrote; every dependency is a launch boundary.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "afhip_lz4_kernels.h"
#include "lz4_encode_pass.h"

namespace afhip {

struct CopyRange {          // == afhip_copy_range
    int64_t src_off, dst_off, n;
};

// One thread per element of the chunk buffer [ct][cy][cx], x fastest: reads are nx-element runs of the cube, writes contiguous.
// Elements outside [0, nt) x [0, ny) x [0, nx) take `fill`.  TE = element as stored (1, 2, 4 or 8 bytes).
template <typename TE>
__global__ __launch_bounds__(256) void k_take_box(const TE* __restrict__ cube, TE* __restrict__ chunk, int64_t NY, int64_t NX,
                                                  int64_t t0, int64_t y0, int64_t x0, int64_t nt, int64_t ny, int64_t nx,
                                                  int64_t ct, int64_t cy, int64_t cx, TE fill) {
    const int64_t n = ct * cy * cx;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t x = i % cx, r = i / cx, y = r % cy, t = r / cy;
        chunk[i] = (t < nt && y < ny && x < nx) ? cube[((t0 + t) * NY + (y0 + y)) * NX + (x0 + x)] : fill;
    }
}

// Blosc's byte shuffle (shuffle_bytes in blosc1.c): tmp[j * n + i] = out[i * ts + j], n = bsize / ts; the bsize % ts trailing bytes
// are copied as they are.  The records name the buffers as the decode side does: out_off = the block in the chunk buffer (read here),
// tmp_off = the block in the shuffle scratch (written here).  grid = (element tiles, blocks); a thread takes one element apart, so a
// wave's stores of one plane are 64 contiguous bytes.
__global__ __launch_bounds__(256) void k_shuffle_blocks(const uint8_t* __restrict__ out, uint8_t* __restrict__ tmp,
                                                        const ShufBlock* __restrict__ blocks) {
    const ShufBlock b = blocks[blockIdx.y];
    const int ts = b.typesize;
    const int64_t n = b.bsize / ts;
    const uint8_t* __restrict__ src = out + b.out_off;
    uint8_t* __restrict__ dst = tmp + b.tmp_off;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (ts == 4 && (((uintptr_t)src) & 3) == 0) {
            const uint32_t v = ((const uint32_t*)src)[i];
            dst[i] = (uint8_t)v; dst[n + i] = (uint8_t)(v >> 8); dst[2 * n + i] = (uint8_t)(v >> 16); dst[3 * n + i] = (uint8_t)(v >> 24);
        } else if (ts == 8 && (((uintptr_t)src) & 7) == 0) {
            const uint64_t v = ((const uint64_t*)src)[i];
#pragma unroll
            for (int j = 0; j < 8; ++j) dst[(int64_t)j * n + i] = (uint8_t)(v >> (8 * j));
        } else {
            for (int j = 0; j < ts; ++j) dst[(int64_t)j * n + i] = src[i * ts + j];
        }
    }
    const int rem = b.bsize % ts;
    if (blockIdx.x == 0 && (int)threadIdx.x < rem) dst[b.bsize - rem + threadIdx.x] = src[b.bsize - rem + threadIdx.x];
}

// One wave per stream; the hash table of lz4_encode_pass.h is the workgroup's only LDS (16 KiB: ten waves a CU).
// Record fields as the decode side names them: src_off = the stream's raw bytes in `in`, dst_off = its slot (dsize bytes) in
// `slots`, to_out != 0 = store without a search (the stored chunk of a buffer under 128 bytes); csize is not read.
__global__ __launch_bounds__(64) void k_lz4_encode_streams(const uint8_t* __restrict__ in, const Lz4Stream* __restrict__ streams,
                                                           uint8_t* __restrict__ slots, int32_t* __restrict__ csize) {
    __shared__ uint32_t table[AFL_TABLE_ENTRIES];
    const Lz4Stream s = streams[blockIdx.x];
    const int32_t c = afl_encode_wave(in + s.src_off, s.dsize, slots + s.dst_off, table, s.to_out, (int)threadIdx.x);
    if (threadIdx.x == 0) csize[blockIdx.x] = c;
}

// One workgroup per range, bytes [src_off, src_off + n) of src -> dst + dst_off: aligned dword stores where the destination
// allows it (the loads may be unaligned: the ranges sit behind the 4-byte stream lengths of a container), bytes at the two ends.
__global__ __launch_bounds__(256) void k_copy_ranges(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                     const CopyRange* __restrict__ ranges) {
    const CopyRange r = ranges[blockIdx.x];
    const uint8_t* __restrict__ s = src + r.src_off;
    uint8_t* __restrict__ d = dst + r.dst_off;
    int64_t head = (int64_t)((4 - ((uintptr_t)d & 3)) & 3);
    if (head > r.n) head = r.n;
    const int64_t words = (r.n - head) / 4, tail0 = head + 4 * words;
    if ((int64_t)threadIdx.x < head) d[threadIdx.x] = s[threadIdx.x];
    for (int64_t i = threadIdx.x; i < words; i += 256) {
        uint32_t v;
        __builtin_memcpy(&v, s + head + 4 * i, 4);
        *(uint32_t*)(d + head + 4 * i) = v;
    }
    if ((int64_t)threadIdx.x < r.n - tail0) d[tail0 + threadIdx.x] = s[tail0 + threadIdx.x];
}

}  // namespace afhip
