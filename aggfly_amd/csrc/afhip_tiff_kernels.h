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
//   k_tiff_place_bands   a chunky segment of B bands (SamplesPerPixel = B, PlanarConfiguration 1): a segment row is pitch * B interleaved
//                  samples, sample i = pixel * B + band, and band b belongs to time step t + b of the time-major cube — a transpose, with the
//                  predictor's running sum taken at stride B on the way.  One workgroup per (segment, row, tile of 64 bands) walks the row in
//                  tiles of 64 pixels x the bands of its tile through LDS: on the load the lanes run along the interleaved samples, where
//                  the segment is contiguous (the band fastest; with B <= 64 a tile is one contiguous run of the row), on the store a wave
//                  takes a band and its lanes run along x, where the cube is contiguous.  The running sums are wave scans along the pixels
//                  of one band, the carry of every band kept in LDS from one pixel tile to the next.  Predictor 3: the bytes of one band
//                  are one chain through all the byte planes (pitch * B is a multiple of B), so a first pass over the row sums every
//                  (plane, band) and a plane starts from the totals of the planes before it, as in k_tiff_place; the load gathers the
//                  E plane bytes of a sample into one LDS element and the scan takes them apart again.  One tile shape serves few bands
//                  and many: with B < 64 the tile is B bands high, a load pass fills 64 * B of the 256 lanes and the waves share B scans.
//                  LDS image [band][pixel] in elements of 4 bytes (8 for 8-byte samples), rows of 65: the scan reads consecutive elements,
//                  and the load puts the lanes of one pixel 65 elements apart — distinct banks with 64 bands; with fewer, the lanes
//                  (b, p) and (b - 1, p + 1) of one pass meet in bank (b + p) mod 64.
//                  The compiler's resource lines (gfx950, -O3, -Rpass-analysis=kernel-resource-usage), 1- / 2- / 4- / 8-byte samples:
//                  70 / 67 / 74 / 115 VGPRs, 17152 / 17408 / 17920 / 35840 B LDS, ScratchSize 0 bytes/lane, 7 / 7 / 6 / 4 waves per SIMD, no
//                  VGPR spills.  No workgroup waits for another.
//                  t may be negative down to -(B - 1): bands whose step t + b lies outside [0, NT - t0) are dropped, which is how a
//                  time window that begins or ends inside a page's bands is served.
//
// Whatever the records and the streams say, nothing is read outside the stage and the decoded buffer and nothing is written outside
// the decoded buffer (k_lzw_decode: inside the segment's own range) and the box of the cube (k_tiff_place, k_tiff_place_bands).
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

// ---- chunky multi-band segments ----
constexpr int TBAND_TILE = 64;                    // pixels and (at most) bands of one LDS tile
constexpr int TBAND_PITCH = TBAND_TILE + 1;       // elements from one band's row of the tile to the next
constexpr int TBAND_MAX = 65535;                  // SamplesPerPixel is a SHORT

template <typename T> struct TiffLds { typedef uint32_t type; };
template <> struct TiffLds<uint64_t> { typedef uint64_t type; };

// tiff_record_ok for rows * pitch * B samples, and t down to -(B - 1).  In forms that cannot overflow.
template <int E>
__device__ __forceinline__ bool tiff_band_record_ok(const TiffSeg& r, int64_t dec_bytes, const TiffBox& g, int64_t B) {
    if (r.rows < 0 || r.pitch < 0 || r.y < 0 || r.x < 0 || r.t <= -B || r.t >= g.NT - g.t0) return false;
    if (r.dec_off < 0 || r.dec_off > dec_bytes || (r.dec_off & (E - 1))) return false;
    return (int64_t)r.rows * r.pitch <= (dec_bytes - r.dec_off) / E / B;
}

template <typename T>
__global__ __launch_bounds__(TIFF_WG) void k_tiff_place_bands(const uint8_t* __restrict__ dec, int64_t dec_bytes, const TiffSeg* __restrict__ recs,
                                                              int B, int predictor, int swap, T* __restrict__ cube, TiffBox g,
                                                              int32_t* __restrict__ errors) {
    constexpr int E = (int)sizeof(T);
    typedef typename TiffScan<T>::type S;
    typedef typename TiffLds<T>::type L;
    __shared__ L tile[TBAND_TILE * TBAND_PITCH];
    __shared__ S run2[TBAND_TILE];                 // predictor 2: the sum of a band's samples before the pixel tile
    __shared__ uint32_t run3[E][TBAND_TILE];       // predictor 3: of a band's bytes before the pixel tile of plane p, the planes before it included
    const TiffSeg r = recs[blockIdx.x];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (r.bad) return;
    if (!tiff_band_record_ok<E>(r, dec_bytes, g, B)) {
        if (blockIdx.y == 0 && blockIdx.z == 0 && tid == 0) atomicAdd(errors, 1);
        return;
    }
    // the bands of this tile, and those among them whose step the cube has: [b_lo, b_hi) of the tile
    const int b0 = (int)blockIdx.z * TBAND_TILE;
    const int TB = B - b0 < TBAND_TILE ? B - b0 : TBAND_TILE;
    const int64_t first = -(int64_t)r.t - b0, last = g.NT - g.t0 - r.t - b0;
    const int b_lo = first > 0 ? (int)first : 0, b_hi = last < TB ? (int)last : TB;
    if (b_hi <= b_lo) return;
    // the columns of the segment inside the box: pixels [i_lo, i_hi) of a row
    const int64_t lo = g.x0 - r.x, hi = g.x0 + g.nx - r.x;
    const int64_t i_lo = lo > 0 ? lo : 0, i_hi = hi < r.pitch ? hi : r.pitch;
    if (i_hi <= i_lo) return;
    const int64_t pitch = r.pitch, row_len = pitch * B;                      // samples of a row; bytes of a byte plane of a row
    // the load: lane -> band lb of the tile (fastest) and every PS-th pixel from lp on; TB * PS <= 256 lanes take part
    const int lb = tid % TB, lp = tid / TB, PS = TIFF_WG / TB;
    const bool loads = lp < PS;
    // (everything that decides a branch around a barrier below is the same for the whole workgroup)
    for (int64_t row = blockIdx.y; row < r.rows; row += gridDim.y) {
        const int64_t yy = r.y + row;
        if (yy < g.y0 || yy >= g.y0 + g.ny) continue;
        const T* __restrict__ src = (const T*)(dec + r.dec_off) + row * row_len;
        const uint8_t* __restrict__ rb = (const uint8_t*)src;
        const int64_t step0 = g.t0 + r.t + b0, cell0 = (g.cy + yy - g.y0) * g.NX + (g.cx + r.x - g.x0);   // band b, pixel i: step0 + b, cell0 + i
        if (predictor == 3) {
            for (int k = tid; k < E * TBAND_TILE; k += TIFF_WG) (&run3[0][0])[k] = 0;
            __syncthreads();
            if (loads) {
                uint32_t part[E];
#pragma unroll
                for (int p = 0; p < E; ++p) part[p] = 0;
                for (int64_t i = lp; i < pitch; i += PS) {
#pragma unroll
                    for (int p = 0; p < E; ++p) part[p] += rb[p * row_len + i * B + b0 + lb];
                }
#pragma unroll
                for (int p = 0; p < E; ++p) atomicAdd(&run3[p][lb], part[p]);
            }
            __syncthreads();
            if (tid < TB) {                                                  // plane p starts from the totals of the planes before it
                uint32_t before = 0;
#pragma unroll
                for (int p = 0; p < E; ++p) {
                    const uint32_t sum = run3[p][tid];
                    run3[p][tid] = before;
                    before += sum;
                }
            }
        } else if (predictor == 2) {
            if (tid < TB) run2[tid] = 0;
        }
        __syncthreads();
        for (int64_t i0 = predictor == 1 ? (i_lo & ~(int64_t)(TBAND_TILE - 1)) : 0; i0 < i_hi; i0 += TBAND_TILE) {
            if (loads) {
                for (int px = lp; px < TBAND_TILE; px += PS) {
                    const int64_t i = i0 + px;
                    L v = 0;
                    if (i < i_hi) {
                        if (predictor == 3) {
#pragma unroll
                            for (int p = 0; p < E; ++p) v |= (L)rb[p * row_len + i * B + b0 + lb] << (8 * (E - 1 - p));   // plane 0: the most significant bytes
                        } else {
                            T s = src[i * B + b0 + lb];
                            if (swap) s = tiff_bswap(s);
                            v = (L)s;
                        }
                    }
                    tile[lb * TBAND_PITCH + px] = v;
                }
            }
            __syncthreads();
            const int64_t i = i0 + lane;
            for (int b = b_lo + wave; b < b_hi; b += TIFF_WG / 64) {         // (a band stays with its wave: b_lo is the row's)
                const L v = tile[b * TBAND_PITCH + lane];
                T out;
                if (predictor == 2) {
                    const S sum = run2[b] + tiff_wave_scan<S>((S)(T)v, lane);
                    out = (T)sum;
                    if (lane == 63) run2[b] = sum;
                } else if (predictor == 3) {
                    uint64_t w = 0;
#pragma unroll
                    for (int p = 0; p < E; ++p) {
                        const uint32_t sum = run3[p][b] + tiff_wave_scan<uint32_t>((uint32_t)(v >> (8 * (E - 1 - p))) & 255u, lane);
                        w |= (uint64_t)(sum & 255u) << (8 * (E - 1 - p));
                        if (lane == 63) run3[p][b] = sum;
                    }
                    out = (T)w;
                } else {
                    out = (T)v;
                }
                if (i >= i_lo && i < i_hi) cube[(step0 + b) * g.NY * g.NX + cell0 + i] = out;
            }
            __syncthreads();
        }
    }
}

}  // namespace afhip
