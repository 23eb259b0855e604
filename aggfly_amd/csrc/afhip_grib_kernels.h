// afhip_grib_kernels.h — GRIB simple, complex and CCSDS packing unpacked in HBM (aggfly_amd/io.py: `_GribSource.to_device`).
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

#include "afhip_filter_kernels.h"    // delta_wave_scan; the running sums of spatial differencing are afhip_delta_decode's launches
#include "aec_passes.h"              // CCSDS packing: the passes of k_grib_awalk and k_grib_arsi

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

// The rank table of one bitmap (at bit map_bit of the stage, NP grid points), by the GRIB_WG lanes of a workgroup: mine[2 + w] = the
// number of 1-bits before word w, 256 words a step with a carry; *carry_s ends as the number of 1-bits of the bitmap.  The lane that
// owns the word of point p_last leaves in `needed` the number of 1-bits up to and including that point.  Every lane takes every step.
__device__ __forceinline__ void grib_rank_scan(const uint8_t* __restrict__ stage, int64_t stage_bytes, int64_t map_bit, int64_t NP, int64_t p_last,
                                               uint32_t* __restrict__ mine, uint32_t* scan, uint32_t* carry_s, uint32_t& needed) {
    const int tid = threadIdx.x;
    const int64_t W = (NP + 31) / 32;
    if (tid == 0) *carry_s = 0;
    __syncthreads();
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
        const uint32_t before = *carry_s + scan[tid] - c;
        if (w < W) {
            mine[2 + w] = before;
            if (w == (p_last >> 5)) needed = before + __builtin_popcount(word >> (31 - (int)(p_last & 31)));
        }
        __syncthreads();
        if (tid == GRIB_WG - 1) *carry_s += scan[tid];
        __syncthreads();
    }
}

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
    uint32_t needed = 0;                 // the number of values up to and including the last point of the box (its owner sets it)
    grib_rank_scan(stage, stage_bytes, r.bitmap_off * 8, NP, p_last, mine, scan, &carry_s, needed);
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

// =======================================================================================
// Complex packing (edition 2, data representation templates 5.2 and 5.3; aggfly_amd/grib.py has the layout of section 7).
//
// The N packed values of a field are cut into NG groups; three tables of fixed-width bit fields give every group a reference, a
// width and a length, and the values follow group after group, width[g] bits each.  Under 5.3 the values are first (order 1) or
// second (order 2) differences, less their minimum.  The whole body of section 7 (and the bitmap) of every step is staged, and four
// passes make values of it (afhip_grib_unpack_complex launches them; `order` is 0 for 5.2 and one number for the whole call):
//
//   k_grib_cgroups  one workgroup per step.  It checks the record against the stage in forms that cannot overflow, builds the
//                   bitmap's rank table like k_grib_rank, reads ival1 / ival2 / minsd, and scans the width and length tables: an
//                   exclusive prefix over the groups, 256 a step with the running totals carried in registers, leaves every group's
//                   first value index and the stage bit where its first value begins in the group scratch.  A step with a width above
//                   32, with lengths that do not sum to N, with a table or a last value beyond its staged bytes, with a bitmap whose
//                   1-bits are not N, or of another order than the call's is refused: flagged, counted in `errors` once, and written
//                   to the cube by nobody.
//   k_grib_cvalues  ONE LANE PER VALUE: it finds its group by a binary search over the groups' first value indices, cuts its bits
//                   out of two byte-swapped aligned dwords (grib_bits32), adds the group's reference and minsd and writes g[n] (the
//                   module docstring of grib.py: g[0] = 0, g[1] = ival2 - ival1 for order 2) as int64 into the value scratch, NP
//                   elements per step, zeros behind the N-th and for a refused step.  The other way round, a wave per group, was not
//                   built: group lengths run from 1 to thousands in one field, so short groups would leave most of a wave idle and
//                   long ones serialise it, and the write of a group begins wherever the group does; a lane per value does the same
//                   work for every value, writes 8 coalesced bytes, and pays log2(NG) reads of a table that stays in L2.
//   running sums    k_delta_tile_sums / k_delta_scan_sums / k_delta_scan_tiles over the value scratch, whose layout is the one they
//                   sum (8-byte elements, chunks of NP back to back): once for order 1, twice for order 2, not at all for 5.2.
//                   Wrapping int64 throughout, as numpy's cumsum on the host route.  No workgroup waits for another.
//   k_grib_cplace   k_grib_unpack's job with X read from the value scratch: a lane owns GRIB_RUN x of a row of the box, the index is the
//                   grid point or the rank of its bit, X = ival1 + sums[index], the value is ((X * s) + R) * d in float64 without
//                   contraction — exact while |X| < 2^53, beyond that the conversion of X to float64 rounds first, as on the host —,
//                   NaN for an absent point, float4 stores where aligned.
//
// Whatever a record says, no lane reads outside [0, stage_bytes) or its step's parts of the scratch, and no lane writes outside the
// box or its step's parts of the scratch.
// =======================================================================================
struct GribCStep {           // == afhip_grib_cstep (include/aggfly_hip.h)
    int64_t data_off;        // the body of the step's section 7 (from octet 6 on) in the stage ...
    int64_t data_bytes;      // ... this many bytes
    int64_t bitmap_off;      // the step's bitmap in the stage (ceil(NY * NX / 8) bytes), or -1
    int64_t n_values;        // N: the grid points, or with a bitmap its 1-bits
    int64_t n_groups;        // NG
    int64_t ref_len, last_len;
    int32_t nbits_ref, ref_width, nbits_width, len_inc, nbits_len;
    int32_t order;           // 0: template 5.2; 1 / 2: template 5.3
    int32_t extra;           // octets of ival1 / ival2 / minsd (0..4)
    int32_t pad;
    double R, s, d;
};

// The group scratch of one step, in int64 words: [0] 1 = the record is sound, [1] ival1, [2] ival2 - ival1, [3] minsd, [4] / [5] the
// stage bits where the reference / width tables begin, [6] NG, [7] unused; then max_groups first value indices and max_groups first bits.
constexpr int GRIB_CHDR = 8;
__host__ __device__ __forceinline__ int64_t grib_cgroup_words(int64_t max_groups) { return GRIB_CHDR + 2 * max_groups; }

__device__ __forceinline__ uint32_t grib_field(const uint8_t* __restrict__ stage, int64_t bit, int width, int64_t stage_bytes) {
    return width ? grib_bits32(stage, bit, stage_bytes) >> (32 - width) : 0u;                  // (width 0..32)
}

__device__ __forceinline__ float grib_cvalue(int64_t X, double R, double s, double d) {
    return (float)((((double)X * s) + R) * d);
}

__device__ __forceinline__ int64_t grib_pad8(int64_t bits) { return (bits + 7) & ~(int64_t)7; }

// ---------------------------------------------------------------------------------------
// k_grib_cgroups: grid = n_steps workgroups of GRIB_WG lanes.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRIB_WG) void k_grib_cgroups(const uint8_t* __restrict__ stage, int64_t stage_bytes, const GribCStep* __restrict__ steps,
                                                          int order, int64_t max_groups, GribBox g, uint32_t* __restrict__ rank,
                                                          int64_t* __restrict__ gscr, int32_t* __restrict__ errors) {
    __shared__ uint32_t scan[GRIB_WG];
    __shared__ uint32_t carry_s;
    __shared__ uint64_t wcarry[2][2][GRIB_WG / 64];
    const GribCStep r = steps[blockIdx.x];
    const int64_t NP = g.NY * g.NX;
    uint32_t* __restrict__ mine = rank + (int64_t)blockIdx.x * grib_rank_words(NP);
    int64_t* __restrict__ hdr = gscr + (int64_t)blockIdx.x * grib_cgroup_words(max_groups);
    int64_t* __restrict__ vstart = hdr + GRIB_CHDR;
    int64_t* __restrict__ bstart = vstart + max_groups;
    const int tid = threadIdx.x, wave = tid >> 6;
    const bool has_map = r.bitmap_off != -1;
    const int64_t N = r.n_values, NG = r.n_groups;
    // every test in a form that cannot overflow: the record is whatever the caller wrote.  (All of it is uniform over the workgroup.)
    bool ok = r.data_off >= 0 && r.data_bytes >= 0 && r.data_off <= stage_bytes && r.data_bytes <= stage_bytes - r.data_off &&
              N >= 0 && N <= NP && NG >= 0 && NG <= max_groups && r.order == order && r.extra >= 0 && r.extra <= 4 &&
              r.nbits_ref >= 0 && r.nbits_ref <= 32 && r.nbits_width >= 0 && r.nbits_width <= 32 && r.nbits_len >= 0 && r.nbits_len <= 32 &&
              r.ref_width >= 0 && r.ref_width <= 255 && r.len_inc >= 0 && r.len_inc <= 255 &&
              r.ref_len >= 0 && r.ref_len <= 0xffffffffll && r.last_len >= 0 && r.last_len <= 0xffffffffll;
    if (ok && has_map) ok = r.bitmap_off >= 0 && r.bitmap_off <= stage_bytes && (NP + 7) / 8 <= stage_bytes - r.bitmap_off;
    if (ok && !has_map) ok = N == NP;
    // where the tables lie, in bits from the start of the body (NG <= 2^31 - 1 and 32 bits an entry: far below 2^63)
    const int64_t refs_rel = order ? 8 * (int64_t)r.extra * (order + 1) : 0;
    int64_t widths_rel = 0, lens_rel = 0, vals_rel = 0;
    if (ok) {
        widths_rel = grib_pad8(refs_rel + NG * r.nbits_ref);
        lens_rel = grib_pad8(widths_rel + NG * r.nbits_width);
        vals_rel = grib_pad8(lens_rel + NG * r.nbits_len);
        if (NG > 0) ok = (vals_rel >> 3) <= r.data_bytes;                        // the descriptors and the tables end inside the staged bytes
    }
    if (ok && has_map) {
        uint32_t unused = 0;
        grib_rank_scan(stage, stage_bytes, r.bitmap_off * 8, NP, NP - 1, mine, scan, &carry_s, unused);
        ok = (int64_t)carry_s == N;                                              // one value per 1-bit
    }
    if (!ok) {
        if (tid == 0) {
            hdr[0] = 0;
            atomicAdd(errors, 1);
        }
        return;
    }
    const int64_t base = r.data_off * 8;
    int64_t ival1 = 0, ival2 = 0, minsd = 0;
    if (order && r.extra && NG > 0) {
        const int eb = 8 * r.extra;
        const uint32_t top = 1u << (eb - 1);
        const uint32_t w0 = grib_field(stage, base, eb, stage_bytes), w1 = grib_field(stage, base + eb, eb, stage_bytes);
        const uint32_t wm = order == 2 ? grib_field(stage, base + 2 * eb, eb, stage_bytes) : w1;        // sign-magnitude, all three
        ival1 = w0 & top ? -(int64_t)(w0 & (top - 1)) : (int64_t)w0;
        if (order == 2) ival2 = w1 & top ? -(int64_t)(w1 & (top - 1)) : (int64_t)w1;
        minsd = wm & top ? -(int64_t)(wm & (top - 1)) : (int64_t)wm;
    }
    // the exclusive scan of the lengths (-> first value index) and of length * width (-> first bit), GRIB_WG groups a step.  The sums
    // are unsigned and may wrap for lengths that do not sum to N; such a step is refused below and its table is read by nobody.
    uint64_t vrun = 0, brun = 0;
    int bad = 0, flip = 0;
    for (int64_t g0 = 0; g0 < NG; g0 += GRIB_WG, flip ^= 1) {                    // (uniform: every lane takes every step)
        const int64_t gi = g0 + tid;
        uint64_t len = 0, bits = 0;
        if (gi < NG) {
            const uint64_t width = (uint64_t)r.ref_width + grib_field(stage, base + widths_rel + gi * r.nbits_width, r.nbits_width, stage_bytes);
            len = gi == NG - 1 ? (uint64_t)r.last_len
                               : (uint64_t)r.ref_len + (uint64_t)r.len_inc * grib_field(stage, base + lens_rel + gi * r.nbits_len, r.nbits_len, stage_bytes);
            if (width > 32 || len > (uint64_t)N) {
                bad = 1;
                len = 0;
            }
            bits = len * width;
        }
        const uint64_t vi = delta_wave_scan<uint64_t>(len), bi = delta_wave_scan<uint64_t>(bits);
        if ((tid & 63) == 63) {
            wcarry[flip][0][wave] = vi;
            wcarry[flip][1][wave] = bi;
        }
        __syncthreads();
        uint64_t vb = vrun, vt = vrun, bb = brun, bt = brun;
#pragma unroll
        for (int w = 0; w < GRIB_WG / 64; ++w) {
            const uint64_t cv = wcarry[flip][0][w], cb = wcarry[flip][1][w];
            if (w < wave) { vb += cv; bb += cb; }
            vt += cv;
            bt += cb;
        }
        if (gi < NG) {
            vstart[gi] = (int64_t)(vb + vi - len);
            bstart[gi] = (int64_t)((uint64_t)(base + vals_rel) + bb + bi - bits);
        }
        vrun = vt;
        brun = bt;
    }
    bad = __syncthreads_or(bad);
    // lengths that sum to N (then brun <= 32 N: nothing wrapped), and the last value ends inside the staged bytes.  NG = 0: every X is 0.
    ok = NG == 0 || (!bad && vrun == (uint64_t)N && (((uint64_t)vals_rel + brun + 7) >> 3) <= (uint64_t)r.data_bytes);
    if (tid == 0) {
        hdr[0] = ok ? 1 : 0;
        hdr[1] = ival1;
        hdr[2] = ival2 - ival1;
        hdr[3] = minsd;
        hdr[4] = base + refs_rel;
        hdr[5] = base + widths_rel;
        hdr[6] = NG;
        hdr[7] = 0;
        if (!ok) atomicAdd(errors, 1);
    }
}

// ---------------------------------------------------------------------------------------
// k_grib_cvalues: one lane per element of the value scratch (n_steps * NP).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(GRIB_WG) void k_grib_cvalues(const uint8_t* __restrict__ stage, int64_t stage_bytes, const GribCStep* __restrict__ steps,
                                                          int64_t n_steps, int64_t NP, int64_t max_groups, const int64_t* __restrict__ gscr,
                                                          int64_t* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * GRIB_WG + threadIdx.x;
    if (i >= n_steps * NP) return;
    const int64_t t = i / NP, n = i % NP;
    const int64_t* __restrict__ hdr = gscr + t * grib_cgroup_words(max_groups);
    const int64_t* __restrict__ vstart = hdr + GRIB_CHDR;
    const int64_t* __restrict__ bstart = vstart + max_groups;
    const int64_t NG = hdr[6];
    int64_t out = 0;
    if (hdr[0] == 1 && NG > 0 && NG <= max_groups) {
        const GribCStep& r = steps[t];
        if (n < r.n_values) {
            if (r.order >= 1 && n == 0) {
                out = 0;                                                         // (raw[0] is a placeholder)
            } else if (r.order == 2 && n == 1) {
                out = hdr[2];                                                    // ival2 - ival1 (raw[1] is a placeholder)
            } else {
                int64_t lo = 0, hi = NG - 1;                                     // the last group that begins at or before n (vstart[0] = 0)
                while (lo < hi) {
                    const int64_t mid = (lo + hi + 1) >> 1;
                    if (vstart[mid] <= n) lo = mid;
                    else hi = mid - 1;
                }
                const int width = r.ref_width + (int)grib_field(stage, hdr[5] + lo * r.nbits_width, r.nbits_width, stage_bytes);
                const uint32_t ref = grib_field(stage, hdr[4] + lo * r.nbits_ref, r.nbits_ref, stage_bytes);
                const uint32_t field = grib_field(stage, bstart[lo] + (n - vstart[lo]) * width, width, stage_bytes);
                out = (int64_t)ref + (int64_t)field + hdr[3];
            }
        }
    }
    vals[i] = out;
}

// ---------------------------------------------------------------------------------------
// k_grib_cplace: one lane per run of GRIB_RUN x of one row of one step.  One text for every packing whose integers lie in a value
// scratch: `Vals` says whether step t is sound (`open`) and what X its value idx is (`at`) — GribCVals for complex packing, GribAVals
// for CCSDS (below) —, `Step` is the record type (bitmap_off, n_values, R, s, d).
// ---------------------------------------------------------------------------------------
struct GribCVals {
    int64_t max_groups, NP;
    const int64_t* __restrict__ gscr;
    const int64_t* __restrict__ vals;
    struct Of {
        const int64_t* __restrict__ sums;
        uint64_t ival1;
        __device__ __forceinline__ int64_t at(int64_t idx) const { return (int64_t)(ival1 + (uint64_t)sums[idx]); }
    };
    __device__ __forceinline__ bool open(int64_t t, Of& o) const {
        const int64_t* __restrict__ hdr = gscr + t * grib_cgroup_words(max_groups);
        if (hdr[0] != 1) return false;
        o.sums = vals + t * NP;
        o.ival1 = (uint64_t)hdr[1];
        return true;
    }
};

template <class Step, class Vals>
__global__ __launch_bounds__(GRIB_WG) void k_grib_cplace(const uint8_t* __restrict__ stage, int64_t stage_bytes, const Step* __restrict__ steps,
                                                         int64_t n_steps, GribBox g, const uint32_t* __restrict__ rank, Vals src, float* __restrict__ cube) {
    const int64_t lpr = (g.nx + GRIB_RUN - 1) / GRIB_RUN;                       // lanes per row
    const int64_t i = (int64_t)blockIdx.x * GRIB_WG + threadIdx.x;
    if (i >= n_steps * g.ny * lpr) return;
    const int64_t xr = i % lpr, row = i / lpr, y = row % g.ny, t = row / g.ny;
    const int64_t NP = g.NY * g.NX;
    typename Vals::Of of;
    if (!src.open(t, of)) return;                                               // a refused step is written by nobody
    const uint32_t* __restrict__ mine = rank + t * grib_rank_words(NP);
    const Step& r = steps[t];
    const double R = r.R, s = r.s, d = r.d;
    const int64_t x = xr * GRIB_RUN;
    const int cnt = (int)(g.nx - x < GRIB_RUN ? g.nx - x : GRIB_RUN);
    const int64_t p0 = (g.y0 + y) * g.NX + g.x0 + x;                            // the run's first grid point
    float* __restrict__ out = cube + ((g.t0 + t) * g.CNY + (g.cy + y)) * g.CNX + g.cx + x;
    float v[GRIB_RUN];
    if (r.bitmap_off == -1) {
#pragma unroll
        for (int k = 0; k < GRIB_RUN; ++k) v[k] = k < cnt ? grib_cvalue(of.at(p0 + k), R, s, d) : 0.0f;
    } else {
        const int64_t map_bit = r.bitmap_off * 8, N = r.n_values;
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
                    if (idx < N) f = grib_cvalue(of.at(idx), R, s, d);             // (always: the 1-bits are N)
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

// =======================================================================================
// CCSDS packing (edition 2, data representation template 5.42): section 7 is one CCSDS 121.0-B adaptive-entropy-coded stream as libaec
// writes it (aec_passes.h has the format, the passes and their safety contract).  The whole body of section 7 (and the bitmap) of every
// step is staged, and three passes make values of it (afhip_grib_unpack_ccsds launches them):
//
//   k_grib_awalk   one workgroup per step.  Its GRIB_WG lanes check the record against the stage and build the bitmap's rank table like
//                  k_grib_cgroups (a step whose bitmap has another number of 1-bits than n_values, or without a bitmap another number
//                  of values than grid points, is refused); then its first wave alone runs aec_pass_walk: the block headers of the
//                  stream are walked, the end of a block found by a prefix popcount over 64 byte-swapped dwords held one a lane and a
//                  ballot (aec_nth_one_wave), and the stage bit where every RSI begins is left in the RSI table.
//   k_grib_arsi    ONE LANE PER RSI (aec_pass_rsi): the blocks decoded to deltas, the preprocessor undone, X written as uint32 into the
//                  value scratch, NP elements per step.  Neighbouring lanes hold neighbouring RSIs of one step.
//   k_grib_cplace  with GribAVals: X read from that scratch.
//
// A refused step is flagged in the `sound` table, counted in `errors` once and written to the cube by nobody.  No workgroup waits for
// another; whatever a record or a stream says, no lane reads outside [0, stage_bytes) or writes outside its step's parts of the scratch.
// =======================================================================================
static_assert(sizeof(aec_step) == 72, "record layout");

struct GribAVals {
    int64_t NP;
    const int32_t* __restrict__ sound;
    const uint32_t* __restrict__ vals;
    struct Of {
        const uint32_t* __restrict__ X;
        __device__ __forceinline__ int64_t at(int64_t idx) const { return (int64_t)X[idx]; }
    };
    __device__ __forceinline__ bool open(int64_t t, Of& o) const {
        o.X = vals + t * NP;
        return sound[t] == 1;
    }
};

__global__ __launch_bounds__(GRIB_WG) void k_grib_awalk(aec_ctx c, GribBox g, uint32_t* __restrict__ rank) {
    __shared__ uint32_t scan[GRIB_WG];
    __shared__ uint32_t carry_s;
    const int64_t t = blockIdx.x;
    const aec_step r = c.steps[t];
    const int64_t NP = g.NY * g.NX;
    const bool has_map = r.bitmap_off != -1;
    bool ok = aec_record_ok(&c, &r) != 0;                                       // (uniform over the workgroup, like all that follows)
    if (ok && has_map) ok = r.bitmap_off >= 0 && r.bitmap_off <= c.stage_bytes && (NP + 7) / 8 <= c.stage_bytes - r.bitmap_off;
    if (ok && !has_map) ok = r.n_values == NP;
    if (ok && has_map) {
        uint32_t unused = 0;
        grib_rank_scan(c.stage, c.stage_bytes, r.bitmap_off * 8, NP, NP - 1, rank + t * grib_rank_words(NP), scan, &carry_s, unused);
        ok = (int64_t)carry_s == r.n_values;                                    // one value per 1-bit
    }
    if (threadIdx.x >= 64) return;                                              // the walk is the first wave's
    aec_pass_walk(&c, t, ok ? 1 : 0);
}

__global__ __launch_bounds__(GRIB_WG) void k_grib_arsi(aec_ctx c) {
    const int64_t i = (int64_t)blockIdx.x * GRIB_WG + threadIdx.x;
    if (i >= c.n_steps * c.max_rsis) return;
    aec_pass_rsi(&c, i / c.max_rsis, i % c.max_rsis);
}

}  // namespace afhip
