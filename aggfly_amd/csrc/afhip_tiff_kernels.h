// afhip_tiff_kernels.h — the segments (strips or tiles) of a TIFF stack decoded and placed in HBM (aggfly_amd/io.py: `_TiffSource.to_device`).
//
// The host reads the image file directories only (aggfly_amd/tiff.py) and stages the segments that touch the requested box; one record
// per segment (TiffSeg == lzw_seg == afhip_tiff_seg) serves both kernels:
//
//   k_lzw_decode   one wave per segment, running the text of lzw_passes.h with the span table (24 KiB) in LDS: five waves fit the 160 KiB
//                  of a CU, and occupancy is set by that.  The stream is walked twice: a dry walk that writes nothing decides whether the
//                  segment is sound, so a bad segment's part of the decoded buffer is untouched; then the same walk with the stores.  A code
//                  is a literal (lane 0 stores a byte) or a copy of an earlier span of the output, 64 bytes a step across the lanes
//                  (lzw_copy), the source served by L2 once the wave's stores have arrived there.  No workgroup waits for another.
//   k_tiff_place   a wave per segment row: undoes the predictor along the row and writes the samples inside the box at (t, y, x) of the
//                  cube.  Predictor 2 is a wrapping running sum in the sample's width — a wave scan with a carry from one 64-lane pass to
//                  the next —, after the byte swap of a big-endian file.  Predictor 3 is a running sum mod 256 over the row's
//                  pitch * size bytes, whose planes (the most significant bytes of all samples first) are then gathered into samples: a
//                  plane's sum starts from the totals of the planes before it, so each pass scans one byte per plane and lane and no
//                  summed row is written anywhere.  Predictor 1 swaps only.  The row pitch is the tile width for tiles: the padding
//                  columns of a partial right-edge tile are part of the sum and of the plane stride, and are dropped with everything
//                  else outside the box.
//
// Whatever the records and the streams say, nothing is read outside the stage and the decoded buffer and nothing is written outside
// the decoded buffer (k_lzw_decode: inside the segment's own range) and the box of the cube (k_tiff_place).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzw_passes.h"

namespace afhip {

typedef lzw_seg TiffSeg;             // == afhip_tiff_seg (include/aggfly_hip.h)

constexpr int TIFF_WG = 256;         // k_tiff_place: four waves, a row each

__global__ __launch_bounds__(64) void k_lzw_decode(const uint8_t* __restrict__ stage, int64_t stage_bytes, TiffSeg* recs, uint8_t* out,
                                                   int64_t out_bytes, int32_t* __restrict__ errors) {
    __shared__ volatile uint32_t tab_pos[LZW_CODES];
    __shared__ volatile uint16_t tab_len[LZW_CODES];
    TiffSeg* r = recs + blockIdx.x;
    int bad = !lzw_record_ok(r, stage_bytes, out_bytes);
    if (!bad) bad = lzw_decode_segment(stage + r->src_off, r->src_bytes, out + r->dec_off, r->dec_bytes, tab_pos, tab_len, 0);
    if (!bad) bad = lzw_decode_segment(stage + r->src_off, r->src_bytes, out + r->dec_off, r->dec_bytes, tab_pos, tab_len, 1);
    if (threadIdx.x == 0) {
        r->bad = bad;
        if (bad) atomicAdd(errors, 1);
    }
}

// where the samples go: the cube (NT, NY, NX), the box (y0, x0, ny, nx) of the image and its corner (t0, cy, cx) in the cube
struct TiffBox { int64_t NT, NY, NX, y0, x0, ny, nx, t0, cy, cx; };

template <typename U>
__device__ __forceinline__ U tiff_wave_scan(U v, int lane) {          // inclusive prefix sum over the 64 lanes, wrapping
    for (int d = 1; d < 64; d <<= 1) {
        const U up = __shfl_up(v, d, 64);
        if (lane >= d) v += up;
    }
    return v;
}
__device__ __forceinline__ uint32_t tiff_wave_sum(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint8_t tiff_bswap(uint8_t v) { return v; }
__device__ __forceinline__ uint16_t tiff_bswap(uint16_t v) { return __builtin_bswap16(v); }
__device__ __forceinline__ uint32_t tiff_bswap(uint32_t v) { return __builtin_bswap32(v); }
__device__ __forceinline__ uint64_t tiff_bswap(uint64_t v) { return __builtin_bswap64(v); }

template <typename T> struct TiffScan { typedef unsigned int type; };
template <> struct TiffScan<uint64_t> { typedef unsigned long long type; };

// Is the placement half of a record sound?  In forms that cannot overflow.
template <int E>
__device__ __forceinline__ bool tiff_record_ok(const TiffSeg& r, int64_t dec_bytes, const TiffBox& g) {
    if (r.rows < 0 || r.pitch < 0 || r.t < 0 || r.y < 0 || r.x < 0 || r.t >= g.NT - g.t0) return false;
    if (r.dec_off < 0 || r.dec_off > dec_bytes || (r.dec_off & (E - 1))) return false;
    return (int64_t)r.rows * r.pitch <= (dec_bytes - r.dec_off) / E;
}

template <typename T>
__global__ __launch_bounds__(TIFF_WG) void k_tiff_place(const uint8_t* __restrict__ dec, int64_t dec_bytes, const TiffSeg* __restrict__ recs,
                                                        int predictor, int swap, T* __restrict__ cube, TiffBox g, int32_t* __restrict__ errors) {
    constexpr int E = (int)sizeof(T);
    typedef typename TiffScan<T>::type S;
    const TiffSeg r = recs[blockIdx.x];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (r.bad) return;
    if (!tiff_record_ok<E>(r, dec_bytes, g)) {
        if (blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(errors, 1);
        return;
    }
    // the columns of the segment inside the box: samples [i_lo, i_hi) of a row
    const int64_t lo = g.x0 - r.x, hi = g.x0 + g.nx - r.x;
    const int64_t i_lo = lo > 0 ? lo : 0, i_hi = hi < r.pitch ? hi : r.pitch;
    if (i_hi <= i_lo) return;
    const int64_t pitch = r.pitch;
    for (int64_t row = (int64_t)blockIdx.y * (TIFF_WG / 64) + wave; row < r.rows; row += (int64_t)gridDim.y * (TIFF_WG / 64)) {
        const int64_t yy = r.y + row;
        if (yy < g.y0 || yy >= g.y0 + g.ny) continue;
        const T* __restrict__ src = (const T*)(dec + r.dec_off) + row * pitch;
        T* __restrict__ dst = cube + ((g.t0 + r.t) * g.NY + (g.cy + yy - g.y0)) * g.NX + (g.cx + r.x - g.x0);      // + i: sample i of the row
        if (predictor == 2) {
            S carry = 0;
            for (int64_t i0 = 0; i0 < i_hi; i0 += 64) {
                const int64_t i = i0 + lane;
                T v = i < i_hi ? src[i] : (T)0;
                if (swap) v = tiff_bswap(v);
                const S incl = tiff_wave_scan<S>((S)v, lane);
                if (i >= i_lo && i < i_hi) dst[i] = (T)(carry + incl);
                carry += __shfl(incl, 63, 64);
            }
        } else if (predictor == 3) {
            const uint8_t* __restrict__ rb = (const uint8_t*)src;
            uint32_t base[E], carry[E];                                    // the sum of the bytes before plane b; of plane b so far
            uint32_t before = 0;
#pragma unroll
            for (int b = 0; b < E; ++b) {
                uint32_t part = 0;
                for (int64_t i = lane; i < pitch; i += 64) part += rb[b * pitch + i];
                base[b] = before;
                carry[b] = 0;
                before += tiff_wave_sum(part);
            }
            for (int64_t i0 = 0; i0 < i_hi; i0 += 64) {
                const int64_t i = i0 + lane;
                uint64_t v = 0;
#pragma unroll
                for (int b = 0; b < E; ++b) {                              // plane 0 holds the most significant bytes
                    const uint32_t incl = tiff_wave_scan<uint32_t>(i < i_hi ? rb[b * pitch + i] : 0u, lane);
                    v |= (uint64_t)((base[b] + carry[b] + incl) & 255u) << (8 * (E - 1 - b));
                    carry[b] += __shfl(incl, 63, 64);
                }
                if (i >= i_lo && i < i_hi) dst[i] = (T)v;
            }
        } else {
            for (int64_t i = i_lo + lane; i < i_hi; i += 64) dst[i] = swap ? tiff_bswap(src[i]) : src[i];
        }
    }
}

}  // namespace afhip
