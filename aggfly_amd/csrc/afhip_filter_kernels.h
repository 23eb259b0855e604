// afhip_filter_kernels.h — numcodecs element filters undone in HBM (aggfly_amd/io.py: `_ScatterJob`, `_FilterPlan`).
//
// A Zarr format-2 array written with element filters leaves the compressor as STORED elements — int16 where the array says
// float32 — and crosses PCIe that way.  Two kernels make values of them:
//
//   delta    Delta's decode is a running sum over the whole flattened chunk, in the stored integer type (wrapping).  Chunks lie back to
//            back in the staging buffer, chunk_elems elements each; a chunk is cut into tiles of DELTA_TILE_BYTES and summed
//            reduce-then-scan in three launches — k_delta_tile_sums (a workgroup per tile leaves the tile's sum in the scratch),
//            k_delta_scan_sums (a workgroup per chunk turns the chunk's tile sums into exclusive prefixes, 256 a step with a carry),
//            k_delta_scan_tiles (a workgroup per tile scans it in place, seeded with its prefix).  No workgroup waits for another: a
//            launch ends before the next begins, so nothing depends on which workgroups are resident.  Wrapping addition is
//            associative, so any order gives the bits of a sequential sum.  A chunk of one tile needs the last launch only.
//            Inside a tile a lane owns 16 consecutive bytes a round (one aligned 16-byte load and store where the chunk's bytes allow it,
//            element accesses with a bounds check where they do not: a chunk start that is not 16-byte aligned, the chunk's last
//            elements), sums them in registers, and the lanes' sums are scanned by DPP inside a wave (wave_scan_add's steps; 64-bit
//            sums move as two halves) and through DELTA_WAVES carries in LDS across the waves; DELTA_ROUNDS rounds make a tile, the
//            running total carried in a register.
//   fso      FixedScaleOffset's decode, elementwise from a stored buffer to a float32 / float64 one: enc / scale + offset, in float64
//            for stored integers and in the stored type for stored floats, a true IEEE division, compiled without contraction, rounded
//            once to the destination.  For stored INTEGERS scale 1 and offset 0 give the bits of the plain conversion (an integer
//            divided by 1.0 plus 0.0 is exact in float64), which is how Quantize's and AsType's decodes from integers run; for stored
//            floats they do not (-0.0 + 0.0 is +0.0, and a NaN's payload may change), so the caller converts those itself.  A lane
//            converts 16 bytes of output (4 float32 / 2 float64) from one vector load where both buffers are aligned for it, one
//            element a lane where they are not.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afhip {

constexpr int DELTA_WG = 256;
constexpr int DELTA_WAVES = DELTA_WG / 64;
constexpr int DELTA_ROUNDS = 4;                                          // rounds of 256 lanes x 16 bytes
constexpr int DELTA_TILE_BYTES = DELTA_WG * 16 * DELTA_ROUNDS;           // 16 KiB of a chunk per workgroup

__host__ __device__ __forceinline__ int64_t delta_tiles_per_chunk(int64_t chunk_elems, int elem_size) {
    const int64_t tile_elems = DELTA_TILE_BYTES / elem_size;
    return chunk_elems <= 0 ? 0 : (chunk_elems - 1) / tile_elems + 1;        // (no sum that could overflow near INT64_MAX)
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint32_t delta_dpp_or0(uint32_t v) {           // the DPP-selected lane's v, 0 where there is none / masked off
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t delta_dpp_or0(uint64_t v) {           // the same for a 64-bit sum: both halves move alike
    const uint32_t lo = delta_dpp_or0<CTRL, ROW_MASK>((uint32_t)v), hi = delta_dpp_or0<CTRL, ROW_MASK>((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
// inclusive wrapping prefix sum over the 64 lanes (wave_scan_add of afhip_lz4_kernels.h, for uint32_t and uint64_t)
template <typename W>
__device__ __forceinline__ W delta_wave_scan(W v) {
    v += delta_dpp_or0<0x111, 0xf>(v);                                   // row_shr:1, 2, 4, 8 inside each row of 16
    v += delta_dpp_or0<0x112, 0xf>(v);
    v += delta_dpp_or0<0x114, 0xf>(v);
    v += delta_dpp_or0<0x118, 0xf>(v);
    v += delta_dpp_or0<0x142, 0xa>(v);                                   // row_bcast:15 -> rows 1, 3
    v += delta_dpp_or0<0x143, 0xc>(v);                                   // row_bcast:31 -> rows 2, 3
    return v;
}

// sums travel in 32 bits for elements up to 32 bits (the low bits of a wider wrapping sum are the narrow wrapping sum), else in 64
template <typename T> struct DeltaWide { typedef uint32_t type; };
template <> struct DeltaWide<uint64_t> { typedef uint64_t type; };

template <typename T> struct alignas(16) DeltaVec { T v[16 / sizeof(T)]; };

// A lane's 16 bytes of a chunk: elements [e0, e0 + E) of the chunk at `base`, those at or beyond chunk_elems read as 0 and are not
// written.  VEC: `base` is 16-byte aligned, so a whole run is one 16-byte access.
template <typename T, bool VEC>
__device__ __forceinline__ void delta_load(const T* __restrict__ base, int64_t e0, int64_t chunk_elems, T (&x)[16 / sizeof(T)]) {
    constexpr int E = 16 / sizeof(T);
    if (VEC && e0 + E <= chunk_elems) {
        const DeltaVec<T> q = *(const DeltaVec<T>*)(base + e0);
#pragma unroll
        for (int i = 0; i < E; ++i) x[i] = q.v[i];
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i) x[i] = e0 + i < chunk_elems ? base[e0 + i] : (T)0;
    }
}
template <typename T, bool VEC>
__device__ __forceinline__ void delta_store(T* __restrict__ base, int64_t e0, int64_t chunk_elems, const T (&x)[16 / sizeof(T)]) {
    constexpr int E = 16 / sizeof(T);
    if (VEC && e0 + E <= chunk_elems) {
        DeltaVec<T> q;
#pragma unroll
        for (int i = 0; i < E; ++i) q.v[i] = x[i];
        *(DeltaVec<T>*)(base + e0) = q;
    } else {
#pragma unroll
        for (int i = 0; i < E; ++i)
            if (e0 + i < chunk_elems) base[e0 + i] = x[i];
    }
}

// launch 1: sums[chunk * tiles + tile] = the wrapping sum of the tile's elements.  grid = n_chunks * tiles workgroups of DELTA_WG.
template <typename T, bool VEC>
__global__ __launch_bounds__(DELTA_WG) void k_delta_tile_sums(const T* __restrict__ stage, T* __restrict__ sums, int64_t chunk_elems,
                                                              int64_t tiles) {
    typedef typename DeltaWide<T>::type W;
    constexpr int E = 16 / sizeof(T);
    __shared__ W carry[DELTA_WAVES];
    const int64_t chunk = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x % tiles;
    const T* base = stage + chunk * chunk_elems;
    const int64_t t0 = tile * (DELTA_TILE_BYTES / (int64_t)sizeof(T));
    W s = 0;
#pragma unroll
    for (int r = 0; r < DELTA_ROUNDS; ++r) {
        T x[E];
        delta_load<T, VEC>(base, t0 + ((int64_t)r * DELTA_WG + threadIdx.x) * E, chunk_elems, x);
#pragma unroll
        for (int i = 0; i < E; ++i) s += (W)x[i];
    }
    s = delta_wave_scan<W>(s);
    if ((threadIdx.x & 63) == 63) carry[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        W t = 0;
#pragma unroll
        for (int w = 0; w < DELTA_WAVES; ++w) t += carry[w];
        sums[blockIdx.x] = (T)t;
    }
}

// launch 2: the tile sums of each chunk become exclusive prefixes, in place.  grid = n_chunks workgroups of DELTA_WG; a chunk of more
// than DELTA_WG tiles takes several steps, the running total carried in a register.
template <typename T>
__global__ __launch_bounds__(DELTA_WG) void k_delta_scan_sums(T* __restrict__ sums, int64_t tiles) {
    typedef typename DeltaWide<T>::type W;
    __shared__ W carry[2][DELTA_WAVES];
    T* mine = sums + (int64_t)blockIdx.x * tiles;
    const int wave = threadIdx.x >> 6;
    W run = 0;
    int flip = 0;
    for (int64_t i0 = 0; i0 < tiles; i0 += DELTA_WG, flip ^= 1) {       // (uniform: every lane takes every step)
        const int64_t i = i0 + threadIdx.x;
        const W own = i < tiles ? (W)mine[i] : (W)0;
        W incl = delta_wave_scan<W>(own);
        if ((threadIdx.x & 63) == 63) carry[flip][wave] = incl;
        __syncthreads();
        W before = run, total = run;
#pragma unroll
        for (int w = 0; w < DELTA_WAVES; ++w) {
            const W c = carry[flip][w];
            if (w < wave) before += c;
            total += c;
        }
        if (i < tiles) mine[i] = (T)(before + incl - own);
        run = total;
    }
}

// launch 3: each tile scanned in place, seeded with its exclusive prefix (offsets null: every chunk is one tile, seed 0).
template <typename T, bool VEC>
__global__ __launch_bounds__(DELTA_WG) void k_delta_scan_tiles(T* __restrict__ stage, const T* __restrict__ offsets, int64_t chunk_elems,
                                                               int64_t tiles) {
    typedef typename DeltaWide<T>::type W;
    constexpr int E = 16 / sizeof(T);
    __shared__ W carry[2][DELTA_WAVES];
    const int64_t chunk = (int64_t)blockIdx.x / tiles, tile = (int64_t)blockIdx.x % tiles;
    T* base = stage + chunk * chunk_elems;
    const int64_t t0 = tile * (DELTA_TILE_BYTES / (int64_t)sizeof(T));
    const int wave = threadIdx.x >> 6;
    W run = offsets ? (W)offsets[blockIdx.x] : (W)0;
#pragma unroll
    for (int r = 0; r < DELTA_ROUNDS; ++r) {
        const int64_t e0 = t0 + ((int64_t)r * DELTA_WG + threadIdx.x) * E;
        if (t0 + (int64_t)r * DELTA_WG * E >= chunk_elems) break;       // (uniform: the round lies beyond the chunk)
        T x[E];
        delta_load<T, VEC>(base, e0, chunk_elems, x);
        W own = 0;
#pragma unroll
        for (int i = 0; i < E; ++i) own += (W)x[i];
        const W incl = delta_wave_scan<W>(own);
        if ((threadIdx.x & 63) == 63) carry[r & 1][wave] = incl;
        __syncthreads();
        W before = run, total = run;
#pragma unroll
        for (int w = 0; w < DELTA_WAVES; ++w) {
            const W c = carry[r & 1][w];
            if (w < wave) before += c;
            total += c;
        }
        W acc = before + incl - own;                                     // the sum of everything before this lane's run
#pragma unroll
        for (int i = 0; i < E; ++i) {
            acc += (W)x[i];
            x[i] = (T)acc;
        }
        delta_store<T, VEC>(base, e0, chunk_elems, x);
        run = total;
    }
}

// ---- FixedScaleOffset ----
// enc / scale + offset as numpy evaluates it: an integer array divided by a float gives float64; a float array stays in its type
// (scale and offset rounded to it first).  Division and addition round once each; -ffp-contract=off keeps them apart.
template <typename S, typename D>
__device__ __forceinline__ D fso_value(S enc, double scale, double offset) { return (D)((double)enc / scale + offset); }
template <>
__device__ __forceinline__ float fso_value<float, float>(float enc, double scale, double offset) { return enc / (float)scale + (float)offset; }
template <>
__device__ __forceinline__ double fso_value<float, double>(float enc, double scale, double offset) {
    return (double)(enc / (float)scale + (float)offset);
}

template <typename S, int V> struct alignas(sizeof(S) * V >= 16 ? 16 : sizeof(S) * V) FsoSrc { S v[V]; };
template <typename D, int V> struct alignas(16) FsoDst { D v[V]; };

// VEC: src is aligned to V stored elements (16 bytes at most) and dst to 16 bytes; a lane converts V = 16 / sizeof(D) elements, the
// last lane's missing ones one by one.  Else: an element a lane.
template <typename S, typename D, bool VEC>
__global__ __launch_bounds__(256) void k_fso_decode(const S* __restrict__ src, D* __restrict__ dst, int64_t n, double scale, double offset) {
    constexpr int V = 16 / sizeof(D);
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int64_t e0 = g * V;
        if (e0 + V <= n) {
            const FsoSrc<S, V> q = *(const FsoSrc<S, V>*)(src + e0);
            FsoDst<D, V> o;
#pragma unroll
            for (int i = 0; i < V; ++i) o.v[i] = fso_value<S, D>(q.v[i], scale, offset);
            *(FsoDst<D, V>*)(dst + e0) = o;
        } else {
            for (int64_t e = e0; e < n; ++e) dst[e] = fso_value<S, D>(src[e], scale, offset);
        }
    } else if (g < n) {
        dst[g] = fso_value<S, D>(src[g], scale, offset);
    }
}

}  // namespace afhip
