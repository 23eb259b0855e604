// afhip_grib_kernels.h — GRIB simple packing unpacked in HBM (aggfly_amd/io.py: `_grib_part_to_device`).
//
// A GRIB field (editions 1 and 2, simple packing) is a big-endian bit stream of nbits-bit unsigned integers X, nbits 0..32, and the
// value is ((X * s) + R) * d with s = 2^E, d = 10^-D; an optional bitmap, one bit per grid point in scan order, most significant bit
// first, marks the points that have a value.  The host reads the section headers only (aggfly_amd/grib.py), `pread`s the packed bits
// (and the bitmap) of every time step into page-locked memory, the bytes cross PCIe as stored, and two kernels do the rest:
//
//   k_grib_rank    one workgroup per step.  It checks the step's record against the stage and the box (a refused step is flagged,
//                  counted in `errors` once, and written by nobody), and for a step with a bitmap leaves the exclusive prefix of the
//                  per-word popcounts — the number of values before each 32-point word — in the rank scratch.
//   k_grib_unpack  a lane owns GRIB_RUN consecutive x of one row of the box: value index (the grid point, or with a bitmap the rank of
//                  its bit), extraction, scaling, NaN for a missing point, and the store into the float32 cube.
//
// Loads are ALIGNED DWORDS of the stage, byte-swapped, and a value is cut out of two neighbouring dwords by a 64-bit funnel shift; no
// lane loads bytes, and a dword beyond the end of the stage reads as zero (grib_be32).  The byte-aligned widths without a bitmap (8, 16, 24, 32 bits; 16 is ERA5's) take a path of whole loads with every shift
// but one known at compile time: the run's dwords are loaded up front and realigned once.  Whatever a record says, no lane reads
// outside [0, stage_bytes) or its step's part of the rank scratch, and no lane writes outside the box.
//
// The arithmetic is float64, written as on the host (grib.py: decode_message) and compiled without contraction: X * s is exact
// (X < 2^32, s a power of two), the sum rounds once, the product by d once, the conversion to float32 once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afhip {

struct GribStep {            // == afhip_grib_step (include/aggfly_hip.h)
    int64_t data_off;        // the step's staged packed bits: stage + data_off ...
    int64_t data_bytes;      // ... this many bytes
    int64_t first_point;     // the value index (= grid point; there is no bitmap then) the first staged bit belongs to
    int64_t bitmap_off;      // the step's bitmap in the stage (ceil(NY * NX / 8) bytes), or -1
    int32_t first_bit;       // the bit (0..7, from the most significant) of the first staged byte where that value begins
    int32_t nbits;
    double R, s, d;
};

constexpr int GRIB_WG = 256;
constexpr int GRIB_RUN = 8;          // consecutive x per lane: 16 bytes of 16-bit input, 32 bytes of output

// The rank scratch of one step: [0] 1 = the record is sound, [1] the number of 1-bits of the bitmap, [2 + w] the number of 1-bits
// before word w of the bitmap.
__host__ __device__ __forceinline__ int64_t grib_rank_words(int64_t n_points) { return (n_points + 31) / 32 + 2; }

// Big-endian value of the aligned dword q of the stage; dwords at or beyond stage_bytes read as 0 (the stage is dword-aligned and a
// whole number of dwords: the entry refuses any other).
__device__ __forceinline__ uint32_t grib_be32(const uint8_t* __restrict__ stage, int64_t q, int64_t stage_bytes) {
    return q * 4 + 4 <= stage_bytes ? __builtin_bswap32(((const uint32_t*)stage)[q]) : 0u;
}

// The 32 bits from bit `bit` of the stage on (big-endian bit order: bit 0 is the most significant bit of byte 0).
__device__ __forceinline__ uint32_t grib_bits32(const uint8_t* __restrict__ stage, int64_t bit, int64_t stage_bytes) {
    const int64_t q = bit >> 5;
    const uint64_t win = ((uint64_t)grib_be32(stage, q, stage_bytes) << 32) | grib_be32(stage, q + 1, stage_bytes);
    return (uint32_t)((win << (bit & 31)) >> 32);
}

__device__ __forceinline__ float grib_value(uint32_t X, double R, double s, double d) {
    return (float)((((double)X * s) + R) * d);
}

struct GribBox {
    int64_t NY, NX;                      // the grid of the field
    int64_t y0, x0, ny, nx;              // the box of the grid ...
    int64_t CNY, CNX, t0, cy, cx;        // ... and where it lands in the cube [*, CNY, CNX]
};

// ---------------------------------------------------------------------------------------
// k_grib_rank: grid = n_steps workgroups of GRIB_WG lanes.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRIB_WG) void k_grib_rank(const uint8_t* __restrict__ stage, int64_t stage_bytes, const GribStep* __restrict__ steps,
                                                       GribBox g, uint32_t* __restrict__ rank, int32_t* __restrict__ errors) {
    __shared__ uint32_t scan[GRIB_WG];
    __shared__ uint32_t carry_s;
    const GribStep r = steps[blockIdx.x];
    const int64_t NP = g.NY * g.NX, W = (NP + 31) / 32;
    uint32_t* __restrict__ mine = rank + (int64_t)blockIdx.x * grib_rank_words(NP);
    const int tid = threadIdx.x;
    const int64_t p_first = g.y0 * g.NX + g.x0, p_last = (g.y0 + g.ny - 1) * g.NX + g.x0 + g.nx - 1;    // (ny, nx > 0: the entry returns early otherwise)
    const bool has_map = r.bitmap_off != -1;
    // every test in a form that cannot overflow: the record is whatever the caller wrote
    bool ok = r.nbits >= 0 && r.nbits <= 32 && r.first_bit >= 0 && r.first_bit <= 7 && r.data_off >= 0 && r.data_bytes >= 0 &&
              r.data_off <= stage_bytes && r.data_bytes <= stage_bytes - r.data_off;
    if (ok && has_map)
        ok = r.bitmap_off >= 0 && r.bitmap_off <= stage_bytes && (NP + 7) / 8 <= stage_bytes - r.bitmap_off && r.first_point == 0 && r.first_bit == 0;
    if (ok && !has_map)                  // the last value the box needs ends inside the staged bytes
        ok = r.first_point >= 0 && r.first_point <= p_first &&
             (r.nbits == 0 || (p_last - r.first_point + 1) <= (r.data_bytes * 8 - r.first_bit) / r.nbits);
    if (!ok || !has_map) {
        if (tid == 0) {
            mine[0] = ok ? 1u : 0u;
            mine[1] = 0;
            if (!ok) atomicAdd(errors, 1);
        }
        return;
    }
    if (tid == 0) carry_s = 0;
    __syncthreads();
    const int64_t map_bit = r.bitmap_off * 8;
    uint32_t needed = 0;                 // the number of values up to and including the last point of the box (its owner sets it)
    for (int64_t w0 = 0; w0 < W; w0 += GRIB_WG) {
        const int64_t w = w0 + tid;
        uint32_t word = 0;
        if (w < W) {
            word = grib_bits32(stage, map_bit + w * 32, stage_bytes);
            const int64_t left = NP - w * 32;                                   // bits of this word that are grid points
            if (left < 32) word &= ~(0xffffffffu >> left);
        }
        const uint32_t c = __builtin_popcount(word);
        scan[tid] = c;
        __syncthreads();
        for (int off = 1; off < GRIB_WG; off <<= 1) {                           // inclusive scan of the tile's counts
            const uint32_t add = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const uint32_t before = carry_s + scan[tid] - c;
        if (w < W) {
            mine[2 + w] = before;
            if (w == (p_last >> 5)) needed = before + __builtin_popcount(word >> (31 - (int)(p_last & 31)));
        }
        __syncthreads();
        if (tid == GRIB_WG - 1) carry_s += scan[tid];
        __syncthreads();
    }
    // one lane knows `needed`: it decides.  The staged bytes must hold every value up to the last one the box needs.
    if (((p_last >> 5) % GRIB_WG) == tid) {
        const bool fits = r.nbits == 0 || (int64_t)needed <= (r.data_bytes * 8) / r.nbits;
        mine[0] = fits ? 1u : 0u;
        mine[1] = carry_s;
        if (!fits) atomicAdd(errors, 1);
    }
}

// ---------------------------------------------------------------------------------------
// k_grib_unpack: one lane per run of GRIB_RUN x of one row of one step.
// ---------------------------------------------------------------------------------------
// The byte-aligned widths without a bitmap: the run's dwords loaded whole, realigned to the run's first bit by one funnel shift per
// dword, and every value then cut out at a position known at compile time.
template <int NBITS>
__device__ __forceinline__ void grib_run_aligned(const uint8_t* __restrict__ stage, int64_t stage_bytes, int64_t bit, const GribStep& r,
                                                 int cnt, float* __restrict__ v) {
    constexpr int ND = GRIB_RUN * NBITS / 32;            // dwords of a whole run (8 values of 8 / 16 / 24 / 32 bits: 2 / 4 / 6 / 8)
    const int64_t q = bit >> 5;
    const int o = (int)(bit & 31);
    uint32_t w[ND + 1], a[ND];
#pragma unroll
    for (int j = 0; j <= ND; ++j) w[j] = grib_be32(stage, q + j, stage_bytes);
#pragma unroll
    for (int j = 0; j < ND; ++j) a[j] = (uint32_t)(((((uint64_t)w[j]) << 32 | w[j + 1]) << o) >> 32);
#pragma unroll
    for (int k = 0; k < GRIB_RUN; ++k) {
        const int j = (k * NBITS) >> 5, off = (k * NBITS) & 31;
        const uint64_t win = ((uint64_t)a[j] << 32) | (j + 1 < ND ? a[j + 1] : 0u);
        const uint32_t X = (uint32_t)((win << off) >> (64 - NBITS));
        v[k] = grib_value(X, r.R, r.s, r.d);
    }
}

__global__ __launch_bounds__(GRIB_WG) void k_grib_unpack(const uint8_t* __restrict__ stage, int64_t stage_bytes, const GribStep* __restrict__ steps,
                                                         int64_t n_steps, GribBox g, const uint32_t* __restrict__ rank, float* __restrict__ cube) {
    const int64_t lpr = (g.nx + GRIB_RUN - 1) / GRIB_RUN;                       // lanes per row
    const int64_t i = (int64_t)blockIdx.x * GRIB_WG + threadIdx.x;
    if (i >= n_steps * g.ny * lpr) return;
    const int64_t xr = i % lpr, row = i / lpr, y = row % g.ny, t = row / g.ny;
    const int64_t NP = g.NY * g.NX;
    const uint32_t* __restrict__ mine = rank + t * grib_rank_words(NP);
    if (mine[0] != 1u) return;                                                  // a refused step is written by nobody
    const GribStep r = steps[t];
    const int64_t x = xr * GRIB_RUN;
    const int cnt = (int)(g.nx - x < GRIB_RUN ? g.nx - x : GRIB_RUN);
    const int64_t p0 = (g.y0 + y) * g.NX + g.x0 + x;                            // the run's first grid point
    float* __restrict__ out = cube + ((g.t0 + t) * g.CNY + (g.cy + y)) * g.CNX + g.cx + x;
    float v[GRIB_RUN];
    if (r.bitmap_off == -1) {
        const int64_t bit = r.data_off * 8 + r.first_bit + (p0 - r.first_point) * r.nbits;
        switch (r.nbits) {
            case 8: grib_run_aligned<8>(stage, stage_bytes, bit, r, cnt, v); break;
            case 16: grib_run_aligned<16>(stage, stage_bytes, bit, r, cnt, v); break;
            case 24: grib_run_aligned<24>(stage, stage_bytes, bit, r, cnt, v); break;
            case 32: grib_run_aligned<32>(stage, stage_bytes, bit, r, cnt, v); break;
            default: {
                // any width: a 64-bit window of two aligned dwords slides along the run, one new dword whenever 32 bits are used up
                int64_t q = bit >> 5;
                int o = (int)(bit & 31);
                uint32_t hi = 0, lo = 0;
                if (r.nbits) { hi = grib_be32(stage, q, stage_bytes); lo = grib_be32(stage, q + 1, stage_bytes); }
#pragma unroll
                for (int k = 0; k < GRIB_RUN; ++k) {
                    uint32_t X = 0;
                    if (r.nbits && k < cnt) {
                        X = (uint32_t)(((((uint64_t)hi << 32) | lo) << o) >> (64 - r.nbits));
                        o += r.nbits;
                        if (o >= 32) { o -= 32; q += 1; hi = lo; lo = grib_be32(stage, q + 1, stage_bytes); }
                    }
                    v[k] = grib_value(X, r.R, r.s, r.d);
                }
            }
        }
    } else {
        // with a bitmap: the value index of a present point is the number of 1-bits before it — the word's prefix from k_grib_rank
        // plus the popcount of the word's leading bits
        const int64_t map_bit = r.bitmap_off * 8, data_bit = r.data_off * 8;
        int64_t wi = -1;
        uint32_t word = 0, before = 0;
#pragma unroll
        for (int k = 0; k < GRIB_RUN; ++k) {
            float f = __uint_as_float(0x7fc00000u);
            if (k < cnt) {
                const int64_t p = p0 + k;
                if ((p >> 5) != wi) {
                    wi = p >> 5;
                    word = grib_bits32(stage, map_bit + wi * 32, stage_bytes);
                    before = mine[2 + wi];
                }
                const int b = (int)(p & 31);
                if ((word >> (31 - b)) & 1u) {
                    const int64_t idx = (int64_t)before + (b ? __builtin_popcount(word >> (32 - b)) : 0);
                    const uint32_t X = r.nbits ? grib_bits32(stage, data_bit + idx * r.nbits, stage_bytes) >> (32 - r.nbits) : 0u;
                    f = grib_value(X, r.R, r.s, r.d);
                }
            }
            v[k] = f;
        }
    }
    if (cnt == GRIB_RUN && ((uintptr_t)out & 15) == 0) {
        ((float4*)out)[0] = make_float4(v[0], v[1], v[2], v[3]);
        ((float4*)out)[1] = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
        for (int k = 0; k < GRIB_RUN; ++k)
            if (k < cnt) out[k] = v[k];
    }
}

}  // namespace afhip
