// afhip_kernels.h — device code of the MI355X (gfx950) aggregation engine.
//
// Three kernels do the work of one aggregate_dataset() call:
//
//   k_fused_temporal  one streaming pass over the raw (time, cell) cube.  A lane owns VEC
//                     neighbouring cells; it walks its time chunk once, keeps every inner
//                     accumulator (sum/min/max, threshold slots) and every column's outer
//                     accumulator in registers, and writes one partial per (slot, column,
//                     cell).  HBM-bound: algorithmic bytes = T * n_cells * sizeof(elem).
//                     Restates _block_stat/_block_dd/_block_bins/_block_sine_dd
//                     (aggfly/aggregate/nb_kernels.py:121-251) and the transforms
//                     (aggfly/dataset/dataset.py:475-481,527-543) per cell, in the
//                     reference's k-ascending order.
//   k_combine_slots   merges the partials of an outer period in slot order, applies the
//                     shared validity rule (aggfly/aggregate/spatial.py:114-119) and lays
//                     the result out cell-major for the sparse stage.
//   k_csr_spmm        region x cell CSR weighted sums in table order
//                     (_scatter_block, spatial.py:181-186), then k_panel_divide
//                     (spatial.py:127-133).
//
// Runs without per-cell output skip the middle kernel: k_csr_spmm_slots gathers the period partials directly (slot merge,
// validity and weighted sums in one pass), and plans with several output periods reduce their cells by region INSIDE
// k_fused_temporal at every period end (FusedArgs::rf_w, rf_emit; k_rf_reduce adds a region's runs) — the per-cell period
// values are then never written.
//
// No MFMA anywhere: the path is a streaming scan plus a sparse segmented sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "afhip_plan_types.h"

namespace afhip {

struct FusedArgs {
    const void* cube;
    int64_t C;                     // cells
    const int64_t* gtab;           // device [G1+1][2]: {(end step of inner group g) << 1 | (emit a slot after g),
                                   //                    bits of the double 1.0 / (steps in g)}
    const ChunkDesc* chunks;       // device [n_chunks]
    double* partial;               // device [n_slots][K][C]
    int32_t K, nthr;
    int32_t xcd_remap, n_tiles;    // 1: give each XCD a contiguous range of cell tiles (speed only)
    const double* sine_tab;        // device [2][SINE_ROWS][4]: rows of the acos table (sine_theta), or null when no column is sine_dd
    // LDS-histogram bins (FEAT_HIST): the threshold slots form a contiguous partition of equal
    // width with edges hb_edge[0..hb_n]; hb_bin_of_slot[slot] = position of that slot's bin (FEAT_END_BINS: -1 / hb_n for the slot
    // of a wide lower / upper end bin, which reads the guard bin's counter; hb_ends below).
    // guess bin (shifted by one guard bin) = floor(v * hb_c1 + hb_c0); hb_dn / hb_up are the edges
    // rounded down / up to float, so a float v compares exactly:  v > t <=> v > dn,  v < t <=> v < up.
    double hb_c1, hb_c0;
    float hb_c1f, hb_c0f;
    int32_t hb_n, hb_shift;        // hb_shift = log2(blockDim): counters are laid out [bin * VEC + i][blockDim]
    int32_t hb_bin_of_slot[MAX_THR];
    // int16-packed cubes (the PackedI16 storage) — `unpack`: how a stored integer becomes the float32 value (unpack_i16, afhip_loads.h),
    // read by scalar loads.  It shares the bytes of the histogram's DOUBLE edges: a packed cube's values are float32, so its histogram forms
    // read the float constants only (hb_dn / hb_up, hb_c1f, hb_wf ...) and never hb_edge, which the host leaves unwritten for them; the record
    // keeps its size and every field its offset (the general sixteen-column forms index `cols` at run time and hold a copy of the whole record).
    // A packed cube may carry SEVERAL rules, each for a contiguous range of time steps (one per store of a multi-file record):
    // n_rules > 1, rule i = pack_rules[i] unpacks steps pack_bounds[i] .. pack_bounds[i + 1] (device tables of the plan; pack_bounds[0] == 0,
    // pack_bounds[n_rules] == T, strictly increasing).  A row is one time step, so the rule is wave-uniform per row: choosing it is scalar
    // work.  n_rules <= 1: `unpack` is the one rule and the tables are not read.  The new fields lie in the same shared bytes.
    union {
        double hb_edge[MAX_THR + 1];
        struct {
            PackArgs unpack;
            const PackArgs* pack_rules;    // device [n_rules]
            const int64_t* pack_bounds;    // device [n_rules + 1]
            int32_t n_rules, pack_pad;
        };
    };
    float hb_dn[MAX_THR + 1], hb_up[MAX_THR + 1];
    // arithmetic edges (FEAT_ARITH_EDGES): every edge is EXACTLY hb_lo0 + g * hb_w in the input precision (host-checked with
    // the same fma), so the two edges around a guess are two fmas instead of an LDS table read; hb_gl / hb_gh sit
    // inside the lower / upper guard bin: values (and NaN) are clamped onto them first.
    // packed != 0 (single-level plans whose columns are all bin counts): the period's K counts leave as small
    // integers, cell-major, one 16- or 32-byte record per (slot, cell), all ones = NaN (empty period) — instead of
    // K doubles per cell in K planes: an eighth / a quarter of the bytes in 1 / 2 stores instead of K (the f64 stores
    // of the 13-bin CMIP6 plan cost its streaming kernel 18 %)
    int32_t packed;
    // record format: pk_nw 64-bit words per (slot, cell) — 2 (16 B) when K counts of pk_bw bits fit, else 4 with 16-bit
    // fields; column j sits in word pk_word[j] at bit pk_shift[j]; all ones (pk_mask) = NaN
    int32_t pk_nw;
    uint32_t pk_mask;
    uint8_t pk_word[MAX_COLS], pk_shift[MAX_COLS];
    // The cell map (FEAT_CELL_MAP: interior bins of unequal widths) shares the bytes of the arithmetic-edge constants, which its kernels
    // — edge-table forms all — never read: hb_cmap is the plan's device table of 256 bytes, hb_cmap[g] = guarded bin of cell g for
    // g = 0 .. hb_cells + 1 (cell 0 and cell hb_cells + 1 are the guard cells), zero behind.  hb_c1 / hb_c0 (and their float copies) then
    // guess the cell, not the bin (afhip_cell_map.h).
    union {
        struct { double hb_w, hb_lo0, hb_gl, hb_gh; };
        struct {
            const uint8_t* hb_cmap;
            int32_t hb_cells, hb_cmap_pad;
        };
    };
    float hb_wf, hb_lo0f, hb_glf, hb_ghf;
    // ... and the guess constant biased DOWN (hb_c0 - delta, host-chosen): floor(v * hb_c1 + hb_c0b) is then never above the
    // value's bin and at most one below it, and an edge value E[k] always guesses k - 1 — checked by the host on every edge
    // with the kernel's own fma in the input precision; the fma and the floor are monotone in v, so the edges decide it for
    // every value between them (ha_update)
    double hb_c0b;
    float hb_c0bf;
    // wide end bins (FEAT_END_BINS): the outer limits L / U of the partition are not stored again — they are t0 / t1 (float cubes: t0f /
    // t1f, rounded down / up) of the end slots' own thr[] entries, and this word, the record's former padding, names the two slots:
    // bits 0-7 the slot that holds L, bits 8-15 the slot that holds U.  Other kernels never read it (0).
    int32_t hb_ends;
    ThrSlot thr[MAX_THR];
    ColOp cols[MAX_COLS];
    // the lean group end's view of a column in ONE word (src | tf << 4 | (tf_iarg & 0xff) << 8): six of them stay in scalar
    // registers through the time loop; the full records do not (they were re-read, three scalar loads and their waits, per column
    // and group: 13 s_load per two-row group on a four-column polynomial)
    uint32_t ccode[MAX_COLS];
    // Region-fused period ends (rf_w != null; afhip_api.hip: rf_table): instead of one value per (slot, column, cell) the kernel
    // writes one weighted sum per (slot, RUN, column) — a run = consecutive cells of a wave's tile whose e-th table entry names the
    // same region (e = 0, 1; a cell's third, fourth ... entries are "extras", below).  Per period end a wave multiplies
    // where(valid, x_k, 0) and the valid flag of its cells by the cells' weights and adds each run's products with a segmented scan
    // over its lanes (rf_emit); k_rf_reduce then adds a region's runs in run order.  The per-cell period values — 0.4 GB per
    // launch on the reference's own benchmark shape, stores that cost its streaming kernel 6 % — are never written, and the
    // gather kernel over them does not run.
    const double* rf_w;            // device [C][2]: weight of the cell's first / second table entry (0: none)
    const int32_t* rf_tile;        // device [wave tiles][2][2]: {first run, need mask (rf_need)} of entry e in wave tile t (64 * VEC cells)
    double* rf_out;                // device: the sum of (slot, run, column k) at  slot * rf_slot_stride + run * rf_run_stride + k  —
    int64_t rf_slot_stride, rf_run_stride;      // run-major ([runs][n_slots][K + 1]) for plans of many periods: a region's periods side by side for k_rf_reduce
    // cells that sit in MORE than two regions (junctions of polygons): their third, fourth ... entries are "extras" — such a cell
    // also writes its validated period values to rf_ex[slot][rf_x[cell]][K + 1], and k_rf_reduce adds the extras of a region from there
    const int32_t* rf_x;           // device [C]: index of the cell among the cells with extras, -1 = none; null: the table has none
    double* rf_ex;                 // device [n_slots][rf_nx][K + 1]
    int64_t rf_nx;
    // per lane slot (tile * 64 + lane, tiles padded): {scan / start / end bits, run indices} of its cells for both entries, worked out
    // on the host from the regions of neighbouring cells (afhip_api.hip: rf_table; k_fused_temporal: rfbits / rfrid)
    const uint32_t* rf_lane;       // device [wave tiles * 64][2]
    int32_t rf_lds_off, rf_pad;    // byte offset, in the dynamic LDS, of the waves' parking blocks: RF_LANE_BYTES per lane (weights + lane words)
};

// The rule table of multi-rule packed cubes was added INSIDE the bytes `unpack` shares with hb_edge: the record keeps its size and every
// earlier field its offset (the sixteen-column forms hold a copy of the whole record; profiles/packed_cube.txt, section 1).
static_assert(sizeof(FusedArgs) == 3632, "FusedArgs keeps its size");
static_assert(offsetof(FusedArgs, hb_edge) == 160 && offsetof(FusedArgs, unpack) == 160 && offsetof(FusedArgs, hb_dn) == 296, "the shared bytes keep their place");
static_assert(offsetof(FusedArgs, pack_rules) == 200 && offsetof(FusedArgs, pack_bounds) == 208 && offsetof(FusedArgs, n_rules) == 216, "the rule table follows `unpack`");
static_assert(offsetof(FusedArgs, hb_bin_of_slot) == 96 && offsetof(FusedArgs, hb_up) == 364 && offsetof(FusedArgs, packed) == 432 && offsetof(FusedArgs, hb_w) == 480, "FusedArgs: field offsets");
static_assert(offsetof(FusedArgs, hb_cmap) == 480 && offsetof(FusedArgs, hb_cells) == 488 && offsetof(FusedArgs, hb_lo0) == 488 && offsetof(FusedArgs, hb_gh) == 504 &&
              offsetof(FusedArgs, hb_wf) == 512, "the cell map lies inside the arithmetic-edge constants");
static_assert(offsetof(FusedArgs, thr) == 544 && offsetof(FusedArgs, cols) == 1312 && offsetof(FusedArgs, ccode) == 3488 && offsetof(FusedArgs, rf_w) == 3552 && offsetof(FusedArgs, rf_lds_off) == 3624, "FusedArgs: field offsets");

}  // namespace afhip

#include "afhip_numerics.h"
#include "afhip_sine.h"
#include "afhip_loads.h"

namespace afhip {

// ---------------------------------------------------------------------------------------
// k_fused_temporal
//
// grid = (cell tiles, chunks).  blockIdx.x (fastest) walks neighbouring tiles of the same
// chunk, so workgroups resident together read adjacent 4 KB pieces of the same rows: the
// union is one long contiguous run per time step.  There is no reuse between workgroups
// (every byte is read once), so no XCD-aware remap is applied.
//
//   PIPE 0  lanes load straight to registers (any alignment; VEC = 1 is the fallback for
//           shapes whose rows are not 16-byte multiples).
//   PIPE 1  each wave streams its 1 KiB row pieces into a private LDS ring with
//           global_load_lds_dwordx4 (no VGPR destination), DEPTH rows ahead, and reads the
//           current row back with ds_read_b128.  The ring is wave-private, so there are no
//           workgroup barriers: a counted s_waitcnt vmcnt(DEPTH-1) is the only ordering
//           (MI355X_MICROARCH.md, "Two waves per SIMD" item 7).  The prefetch runs across
//           inner-group boundaries, so short groups (daily data, tmin/tmax pairs) stream
//           as well as long ones.
//
//   STAT 0 none | 1 sum | 2 sum+min+max | 3 sum+count+min+max with NaN skipping (nanmean)
// ---------------------------------------------------------------------------------------
// FEAT: the feature bits FEAT_* of afhip_plan_types.h, which says what each one compiles in.
//
// The workgroup size is a launch parameter (64 or 256 threads): waves never talk to each
// other, so small grids are launched as single-wave workgroups for a finer tail.
// TS: the cube's storage (afhip_loads.h: Storage) — float / double, stored as their values (TIn), or PackedI16: rows of int16 (TRaw)
// that `consume` unpacks to float32 at the point of use, so the DEPTH loads of a burst stay in flight as 2-byte elements.
template <typename TS, int PIPE, int VEC, int STAT, int NTHR, int KMAX, int DEPTH, int FEAT>
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(1))) void k_fused_temporal(const FusedArgs a) {
    typedef typename Storage<TS>::value_type TIn;
    typedef typename Storage<TS>::raw_type TRaw;
    constexpr bool PACKED = Storage<TS>::packed;
    // ---- everything the body asks of FEAT ----
    constexpr bool SINE = feat_has(FEAT, FEAT_SINE), GENERAL_TF = feat_has(FEAT, FEAT_GENERAL_TF);
    constexpr int AUX = feat_has(FEAT, FEAT_NT) ? 2 : 0;
    constexpr bool TKI = feat_has(FEAT, FEAT_INT_BINS), SL = feat_has(FEAT, FEAT_SINGLE_LEVEL);
    constexpr bool HB = feat_has(FEAT, FEAT_HIST), HA = feat_has(FEAT, FEAT_ARITH_EDGES);
    constexpr bool EB = feat_has(FEAT, FEAT_END_BINS);
    constexpr bool CM = feat_has(FEAT, FEAT_CELL_MAP);
    constexpr bool PAIR = feat_has(FEAT, FEAT_SHORT_GROUP);
    // (the lean group end skips a per-group walk of ~90 scalar instructions per wave and group, as many as the vector ones that do the
    // arithmetic: profiles/r03_kbench_c5_table_arc.txt)
    constexpr bool LEAN = feat_lean_level(FEAT) >= 1, LEAN_SINE = feat_lean_level(FEAT) == 2;
    constexpr bool RAG = feat_has(FEAT, FEAT_MIXED);
    constexpr int GL = feat_group_rows(FEAT);
    constexpr bool RF = feat_has(FEAT, FEAT_REGION_FUSED);
    constexpr int SINE_BYTES = feat_sine_bytes(FEAT);              // the sine table this variant copies into LDS
    static_assert(!LEAN_SINE || (feat_has(FEAT, FEAT_LEAN) && SINE && KMAX <= 2), "the sine-only lean form: at most two columns");
    static_assert(feat_group_form(FEAT) == 0 || (PAIR && LEAN && !LEAN_SINE), "three- / four-row / mixed groups: a lean short-group form");
    static_assert(feat_has(FEAT, FEAT_FOUR_ROW) + feat_has(FEAT, FEAT_THREE_ROW) + feat_has(FEAT, FEAT_MIXED) <= 1, "one group length rule per variant");
    static_assert(!PAIR || (PIPE == 0 && (STAT == 2 || (STAT == 1 && LEAN)) && NTHR == 0 && DEPTH % GL == 0),
                  "short-group mode: direct loads, sum (+ min + max), no threshold slots");
    static_assert(!LEAN || PAIR, "the lean group end is a short-group form");
    static_assert(!RF || !(SL || HB), "region-fused period ends: two-level plans only");
    static_assert(!(HB && SINE), "histogram variants carry no sine_dd code");
    static_assert(!EB || HB, "wide end bins: a histogram form");
    static_assert(!CM || (EB && !HA), "the cell map: an end-bin histogram form with the edge table");
    static_assert(!RF || VEC <= 2, "region-fused period ends: one or two cells per lane");
    static_assert(!PACKED || (PIPE == 0 && (!PAIR || LEAN) && (HB ? (TKI && STAT <= 1) : !(TKI || SL))),
                  "int16-packed cubes: the general forms, the lean short-group forms (both with region-fused twins) and the LDS-histogram forms of the direct-load path only");
    const int64_t C = a.C;
    const int K = a.K;
    const int lane = threadIdx.x & 63;
    // Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share one).  With xcd_remap the
    // tiles of one XCD form a contiguous run of cells; it changes which XCD reads what, never
    // what is computed (bijective for any tile count).
    int64_t tile = blockIdx.x;
    if (a.xcd_remap) {
        const int nt = a.n_tiles, q = nt / 8, r = nt % 8, x = (int)(blockIdx.x % 8), i = (int)(blockIdx.x / 8);
        tile = (x < r ? (int64_t)x * (q + 1) : (int64_t)r * (q + 1) + (int64_t)(x - r) * q) + i;
    }
    const int64_t c0 = (tile * blockDim.x + threadIdx.x) * VEC;
    const bool active = c0 < C;
    const int64_t c_ld = active ? c0 : (C - VEC);   // clamped: inactive lanes re-read valid cells
    int64_t k_lo, k_hi;
    int g_lo, g_hi, slot;
    {
        const int64_t* w = (const int64_t*)&a.chunks[blockIdx.y];
        k_lo = ld_uniform(w);
        k_hi = ld_uniform(w + 1);
        const int64_t g = ld_uniform(w + 2), sb = ld_uniform(w + 3);
        g_lo = (int32_t)(g & 0xffffffffLL); g_hi = (int32_t)(g >> 32);
        slot = (int32_t)(sb & 0xffffffffLL);
    }
    const int rows = (int)(k_hi - k_lo);            // chunk-relative 32-bit loop control: scalar ALU only
    const TRaw* __restrict__ cube = (const TRaw*)a.cube + k_lo * C + c_ld;

    // ---- per-cell state, all in registers (compile-time indexed) ----
    double s[VEC], mn[VEC], mx[VEC];
    int cnt[VEC];
    unsigned long long nanmask[VEC];                // lane masks in SGPR pairs: OR-ed on the scalar ALU
    bool pnan[VEC];                                 // pair mode: this lane's pair holds a NaN
    TIn plo[VEC], phi[VEC];                         // pair mode: the pair's min / max in the input precision
    unsigned long long nanacc[VEC];                 // lean group end: lanes that met a NaN pair since the last emitted slot
    double acc[(NTHR > 0 && !TKI) ? NTHR : 1][VEC];
    int cthr[(NTHR > 0 && TKI && !HB) ? NTHR : 1][VEC];
    double os[SL ? 1 : KMAX][VEC];

#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        s[i] = 0.0; mn[i] = inf64(); mx[i] = -inf64(); cnt[i] = 0; nanmask[i] = 0ull; nanacc[i] = 0ull;
#pragma unroll
        for (int j = 0; j < NTHR; ++j) { if (HB) {} else if (TKI) cthr[j][i] = 0; else acc[j][i] = 0.0; }
    }
    // LDS-histogram state.  With E[0] = E[hb_n + 2] = NaN (sentinels: every compare fails) and
    // E[k + 1] = edge k, bin g of the guarded partition (g = 0 and g = hb_n + 1 are the guard bins) lies
    // between E[g] and E[g + 1]:
    //   etab_a[g] = {E[g].dn, E[g+1].up}   what the common path needs: v <= dn -> below, v >= up -> above
    //   etab_b[g] = {E[g].up, E[g+1].dn}   only for lanes that leave the guessed bin: is v ON the edge?
    // then the counters [(hb_n + 2) * VEC][blockDim].
    struct EdgeT { TIn lo, hi; };
    extern __shared__ __attribute__((aligned(32))) unsigned char dynlds[];
    EdgeT* etab_a = (EdgeT*)dynlds;
    EdgeT* etab_b = (EdgeT*)(dynlds + HB_TABLE_BYTES / 2);
    int* hcnt = (int*)(dynlds + HB_TABLE_BYTES);
    const int bd = blockDim.x, tid = threadIdx.x;
    // FEAT_CELL_MAP: the cell -> bin map, 256 bytes behind the counters (hb_bins is at most sixteen: inside the launch's LDS for every VEC and bd)
    const unsigned char* cmap = nullptr;
    // sine_dd plans: every workgroup copies the acos table (sine_theta) into LDS, behind the LDS-DMA ring if there is one
    // (feat_sine_p2 variants — two-row groups: the P2 table of sine_pair_g; the others: the acos table of sine_theta — the host
    // hands over the one the variant reads)
    sine_tab_t sine_tab = nullptr;
    sine_p2_t sine_p2 = nullptr;
    if constexpr (SINE) {
        unsigned char* base = dynlds + lds_sine_offset(PIPE, bd >> 6, DEPTH);
        if (a.sine_tab != nullptr) {            // uniform: the host sets it iff a column is sine_dd (and then sizes the LDS for it)
            typedef double d2 __attribute__((ext_vector_type(2)));
            // (the sine-only lean form works in DOUBLED units — clamp, arcs and the column's sum — and halves once per period end:
            // its copy of the table is 2 H, every step an exact scaling of the undoubled one)
            for (int e = tid; e < SINE_BYTES / 16; e += bd) {
                d2 t = ((const d2*)a.sine_tab)[e];
                if constexpr (LEAN_SINE) t *= 2.0;
                ((d2*)base)[e] = t;
            }
            __syncthreads();
        }
        sine_tab = (sine_tab_t)(lds_ptr_t)base;
        sine_p2 = (sine_p2_t)(lds_ptr_t)base;
    }
    const int hb_bins = a.hb_n + 2;
    TIn hb_c1 = 0, hb_c0 = 0, hb_top = 0;
    TIn ha_w = 0, ha_c0b = 0, ha_e0 = 0, ha_gl = 0, ha_gh = 0;
    int hb_sh = 0, hb_lane[VEC] = {0};
    // wide end bins: a value counts only if  eb_lo < v < eb_hi  (the outer limits, in the input precision; +-inf where a side is open)
    TIn eb_lo = 0, eb_hi = 0;
    if constexpr (EB) {
        const int ql = a.hb_ends & 0xff, qh = (a.hb_ends >> 8) & 0xff;
        if constexpr (sizeof(TIn) == 4) { eb_lo = a.thr[ql].t0f; eb_hi = a.thr[qh].t1f; }
        else { eb_lo = a.thr[ql].t0; eb_hi = a.thr[qh].t1; }
    }
    if constexpr (HB) {
        if (tid < hb_bins) {
            auto edge = [&](int k, bool want_up) -> TIn {        // E[k].up or E[k].dn
                if (k == 0 || k == a.hb_n + 2) return (TIn)nan64();
                if constexpr (sizeof(TIn) == 4) return want_up ? a.hb_up[k - 1] : a.hb_dn[k - 1];
                else return a.hb_edge[k - 1];
            };
            EdgeT ea, eb;
            ea.lo = edge(tid, false); ea.hi = edge(tid + 1, true);
            eb.lo = edge(tid, true);  eb.hi = edge(tid + 1, false);
            etab_a[tid] = ea; etab_b[tid] = eb;
        }
        for (int b = 0; b < hb_bins * VEC; ++b) hcnt[b * bd + tid] = 0;
        if constexpr (CM) {
            // the plan's map as 64 words (a workgroup has 64 threads at least; the table is 256 bytes whatever hb_cells)
            uint32_t* cw = (uint32_t*)(hcnt + hb_bins * VEC * bd);
            if (tid < 64) cw[tid] = ((const uint32_t*)a.hb_cmap)[tid];
            cmap = (const unsigned char*)cw;
        }
        __syncthreads();
        if constexpr (sizeof(TIn) == 4) { hb_c1 = a.hb_c1f; hb_c0 = a.hb_c0f; }
        else { hb_c1 = a.hb_c1; hb_c0 = a.hb_c0; }
        hb_top = (TIn)((CM ? a.hb_cells : a.hb_n) + 1);          // the last cell / bin of the guarded range
        if constexpr (HA) {
            if constexpr (sizeof(TIn) == 4) { ha_w = a.hb_wf; ha_e0 = a.hb_lo0f + a.hb_wf; ha_gl = a.hb_glf; ha_gh = a.hb_ghf; ha_c0b = a.hb_c0bf; }
            else { ha_w = a.hb_w; ha_e0 = a.hb_lo0 + a.hb_w; ha_gl = a.hb_gl; ha_gh = a.hb_gh; ha_c0b = a.hb_c0b; }   // (lo0 + w: exact, host-checked)
            // VOP3 takes one scalar operand: keep the second operand of the clamp and the fma addends in VGPRs
            asm volatile("" : "+v"(ha_gh), "+v"(ha_c0b), "+v"(ha_e0));
        }
        asm volatile("" : "+v"(hb_c0));      // keep the addend in a VGPR: v_fma takes one scalar operand only
        hb_sh = a.hb_shift + 2 + (VEC == 4 ? 2 : (VEC == 2 ? 1 : 0));     // byte stride between bins = VEC * blockDim * 4
#pragma unroll
        for (int i = 0; i < VEC; ++i) hb_lane[i] = ((i << a.hb_shift) + tid) * 4;
    }
    auto reset_outer = [&]() {
        if (SL) return;
        if constexpr (LEAN) {          // lean forms: every outer reducer is sum | mean — no per-column identity, no j < K masks
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
#pragma unroll
                for (int i = 0; i < VEC; ++i) os[j][i] = 0.0;
            return;
        }
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < K) {
                const int o = a.cols[j].outer;
                const double init = (o == OUT_MIN) ? inf64() : ((o == OUT_MAX) ? -inf64() : 0.0);
#pragma unroll
                for (int i = 0; i < VEC; ++i) os[j][i] = init;
            }
        }
    };
    reset_outer();

    // ---- region-fused period ends (FusedArgs::rf_w): what a wave needs at every period end, read once ----
    // A wave's tile is its 64 * VEC consecutive cells.  For entry e (the cell's first / second region) a RUN is a maximal stretch of
    // cells of the tile with the same region; the host numbered the runs of a tile in cell order and worked out, per lane, how the
    // segmented scan of the period end proceeds (afhip_api.hip: rf_table — the tables depend on the weights table and VEC only):
    //   weights     of cell i's entries e = 0, 1 (0: none)
    //   bits        per lane, 16 bits per entry e:  bits 0-5   step s of the segmented scan adds the value of lane - 2^s
    //                                                bits 6+i   cell i starts a stretch (region changes, no region, or the tile starts)
    //                                                bits 8+i   cell i ends a run of a region: its sum is stored
    //   rid         byte 2 e + i: index of cell i's run among the runs of (tile, e)
    //   rf_first[e] first run of (tile, e) in rf_out
    //   rf_need[e]  (uniform) bit s: some lane of the wave adds in step s — steps no run of this tile is long enough for are skipped;
    //               bit 6: some run ends at a lane's first cell (two cells per lane); bit 7: the tile has runs of entry e at all
    // columns per block of the period end's scan (registers against overlap): two.  The general two-cell forms of six columns take ONE (RF_SLIM):
    // they are held by their bytes in flight, and with the weights re-read per block and the store addresses formed at the stores the twin fits six waves per SIMD
    constexpr bool RF_SLIM = VEC == 2 && KMAX == 6 && !PAIR && sizeof(TIn) == 4;
    constexpr int RF_CB = RF_SLIM ? 1 : 2;
    // The lane's weights and words are PARKED in LDS (a wave-private block behind the variant's other LDS: RF_LANE_BYTES per lane) and
    // read back at every period end: held in registers they cost the twins ten VGPRs for the whole kernel — 103 against the plain
    // variant's 74 on the float32 configs[1] plan, four waves per SIMD instead of six, for a kernel that is bound by bytes in flight.
    constexpr int RF_LANE_BYTES = rf_lane_bytes(VEC);
    typedef __attribute__((address_space(3))) unsigned char* rf_lds_t;
    rf_lds_t rf_park = nullptr;
    int rf_first[2] = {0, 0}, rf_need[2] = {0, 0};
    if constexpr (RF) {
        if (a.rf_w != nullptr) {
            const int64_t lane0 = (c0 - (int64_t)lane * VEC) / VEC;                      // the wave's first lane slot (uniform)
            const int64_t wt = (int64_t)__builtin_amdgcn_readfirstlane((int)(lane0 / 64));
            typedef uint32_t u2 __attribute__((ext_vector_type(2)));
            typedef double d2 __attribute__((ext_vector_type(2)));
            const u2 lw = *(const u2*)(a.rf_lane + (wt * 64 + lane) * 2);                 // (the table is padded to whole tiles)
            rf_park = (rf_lds_t)(lds_ptr_t)(dynlds + a.rf_lds_off) + (threadIdx.x * RF_LANE_BYTES);
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                d2 w = d2{0.0, 0.0};
                if (active) w = *(const d2*)(a.rf_w + (c0 + i) * 2);
                *(__attribute__((address_space(3))) d2*)(rf_park + i * 16) = w;
            }
            *(__attribute__((address_space(3))) u2*)(rf_park + VEC * 16) = lw;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                rf_first[e] = ld_uniform(a.rf_tile + (wt * 2 + e) * 2);
                rf_need[e] = ld_uniform(a.rf_tile + (wt * 2 + e) * 2 + 1);
            }
        }
    }

    // ---- the hot per-element update ----
    // LDS-histogram update of one value, in two halves so that a batch of rows can issue all its
    // table reads before the first compare needs one (see the PIPE 0 loop).
    auto hb_guess = [&](TIn vr, int& b, EdgeT& ea) {
        // guess in the input precision, clamped into the guarded range while still a float:
        // fmax(NaN, 0) = 0, so a NaN drops into the lower guard bin without a test of its own;
        // the clamped value is >= 0, so the truncating conversion is the floor
        TIn t;
        if constexpr (sizeof(TIn) == 4) t = __builtin_amdgcn_fmed3f(__fmaf_rn(vr, hb_c1, hb_c0), 0.0f, hb_top);
        else t = fmin(fmax(__fma_rn((double)vr, hb_c1, hb_c0), 0.0), hb_top);
        b = (int)t;
        if constexpr (CM) b = cmap[b];                // the cell's bin: one byte from LDS
        ea = etab_a[b];
    };
    auto hb_count = [&](TIn vr, int i, int b, const EdgeT& ea) {
        const bool up = vr >= ea.hi, dn = vr <= ea.lo;               // the value belongs above / below the guess
        bool count = true;
        if (up || dn) {                                               // rare: guess off by one, or v on an edge
            const EdgeT eb = etab_b[b];
            count = up ? !(vr <= eb.hi) : !(vr >= eb.lo);             // strict bins: an edge value is in none
            b += up ? 1 : -1;
        }
        // (wide end bins: the guard bins are counted bins, so a value beyond the outer limits — and NaN, which the clamp sent to the
        // lower guard bin — must not reach them)
        if constexpr (EB) count = count && (vr > eb_lo) && (vr < eb_hi);
        // the counter is private to this lane: a relaxed LDS atomic is one ds_add_u32 (no return value)
        if (count)
            __hip_atomic_fetch_add((int*)((char*)hcnt + (b << hb_sh) + hb_lane[i]), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    };
    // arithmetic-edge form of hb_guess + hb_count: no table read, and (round 3) a ONE-SIDED guess.  With the guess constant biased
    // down by a host-chosen delta, tf = floor(vc * c1 + c0b) is the value's bin or the one below it, and exactly the one below for a
    // value ON an edge (FusedArgs::hb_c0b: the host checks every edge with this very fma; fma and floor are monotone, so what holds
    // at E[k] and E[k + 1] holds between them).  Only the UPPER edge of the guessed bin is then needed, hi = E[tf + 1] (one exact
    // fma):  vc > hi -> bin tf + 1;  vc == hi -> on an edge, in no bin (strict inequalities, nb_kernels.py:190-196);  else bin tf.
    // 9 VALU per element where the two-sided form (both edges, two repairs, two equality tests) took 14: the kernel had become
    // issue-bound beside its stream (16 VALU per 4-byte element with the address arithmetic: the vector ALUs ~70 % busy,
    // profiles/r03_c4_bound_pmc.txt).
    auto ha_update = [&](TIn vr, int i) {
        TIn vc;                                                     // clamped into the guarded range; NaN -> lower guard bin
        if constexpr (sizeof(TIn) == 4) vc = __builtin_amdgcn_fmed3f(vr, ha_gl, ha_gh);
        else vc = fmin(fmax(vr, ha_gl), ha_gh);
        TIn tf, hi;
        if constexpr (sizeof(TIn) == 4) {
            tf = __builtin_floorf(__fmaf_rn(vc, hb_c1, ha_c0b));
            hi = __fmaf_rn(tf, ha_w, ha_e0);                        // E[tf + 1], exactly
        } else {
            tf = __builtin_floor(__fma_rn(vc, hb_c1, ha_c0b));
            hi = __fma_rn(tf, ha_w, ha_e0);
        }
        int b = (int)tf;
        b += (vc > hi) ? 1 : 0;                                     // (a carry-in add)
        bool count = vc != hi;
        if constexpr (EB) count = count && (vr > eb_lo) && (vr < eb_hi);       // wide end bins: the outer limits on the unclamped value; NaN fails
        if (count) {
            int* p = (int*)((char*)hcnt + (b << hb_sh) + hb_lane[i]);
            __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);     // the counter is private to this lane: one ds_add_u32
        }
    };
    // Packed cubes: `pr` is the rule of the row being consumed — scalars: the argument record's rule, or the rule of the plan's table
    // that holds the row (several rules: rule_at / rule_next in front of the time loop).
    PackArgs pr;
    auto consume = [&](const RawVec<TRaw, VEC>& rv, bool hb_inline = true) {
        TIn upk[PACKED ? VEC : 1];
        if constexpr (PACKED) unpack_i16<VEC>(rv.v, pr, upk);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            TIn vr_;
            if constexpr (PACKED) vr_ = upk[i]; else vr_ = rv.v[i];
            const TIn vr = vr_;
            const double v = (double)vr;
            const bool isn = vr != vr;
            // integer-bin plans without an inner statistic never look at the NaN mask (a NaN is simply in no bin)
            if constexpr (!(TKI && STAT == 0)) nanmask[i] |= __builtin_amdgcn_ballot_w64(isn);
            if (STAT == 1) {
                s[i] += v;                          // a NaN poisons s; the group is NaN anyway
            } else if (STAT == 2) {
                s[i] += v;
                mn[i] = __builtin_fmin(mn[i], v);   // minNum/maxNum skip a NaN like the reference's
                mx[i] = __builtin_fmax(mx[i], v);   // "v < mn" / "v > mx" updates: one VALU op each
                // (zeros of both signs: v_min / v_max order -0 < +0 where the reference keeps the first seen — the one rule of its
                // own, DESIGN.md §5, pinned by tests/test_gpu_special_values.py)
            } else if (STAT == 3) {
                s[i] += isn ? 0.0 : v;
                cnt[i] += isn ? 0 : 1;
                mn[i] = __builtin_fmin(mn[i], v);
                mx[i] = __builtin_fmax(mx[i], v);
            }
            if constexpr (HB) {
                if constexpr (HA) { if (hb_inline) ha_update(vr, i); }
                else if (hb_inline) { int b; EdgeT ea; hb_guess(vr, b, ea); hb_count(vr, i, b, ea); }
            }
#pragma unroll
            for (int j = 0; j < (HB ? 0 : NTHR); ++j) {
                if constexpr (TKI) {
                    bool m;                                               // strict, NaN -> false
                    if constexpr (sizeof(TIn) == 4) m = (vr > a.thr[j].t0f) && (vr < a.thr[j].t1f);
                    else m = (v > a.thr[j].t0) && (v < a.thr[j].t1);
                    cthr[j][i] += m ? 1 : 0;
                } else {
                    const double w = __fma_rn(a.thr[j].A, v, a.thr[j].B);
                    if constexpr (sizeof(TIn) == 4) add_if_between<float>(acc[j][i], w, vr, a.thr[j].t0f, a.thr[j].t1f);
                    else add_if_between<double>(acc[j][i], w, v, a.thr[j].t0, a.thr[j].t1);
                }
            }
        }
    };

    // ---- region-fused period end (FusedArgs::rf_w): the period's K values of this lane's cells -> per-run weighted sums ----
    // val[j][i]: column j of cell i (NaN = missing).  The lanes multiply their cells' values (where(valid, x, 0), and the valid flag as
    // column K) by the cells' weights; a segmented inclusive scan over the lanes — six shuffle steps whose add / skip pattern was
    // fixed at kernel start, of which the wave runs only those some run of its tile needs — carries a run's sum to its last cell,
    // and that lane stores it.  The order of the adds is a fixed tree over the cells of the tile: it depends on where the table's
    // runs lie, never on the data or the launch shape.  Products are rounded before the adds (spatial.py:183-185).
    // (Round 3 staged the values in a wave-private LDS block and let one lane per (run, column) walk its run: a serial chain of LDS
    // round trips per period end, and the weights re-read from memory at every one — 3.7 against 3.3 ms on the daily configs[1]
    // panel, 27.5 against 17.7 on a daily sine_dd panel of (tmin, tmax) pairs; profiles/r04_region_fused_scan.txt.)
    auto rf_emit = [&](double (&val)[KMAX][VEC], int at_slot) {
        const int K1 = K + 1;
        // shared validity, applied in place (the caller resets / drops its period values right after): x = where(valid, x, 0)
        bool ok[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            bool valid = active;                                     // (lanes beyond the grid carry no weight and no run)
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
                if (j < K) valid = valid && (val[j][i] == val[j][i]);
            ok[i] = valid;
            if (!valid) {
                KEEP_BRANCH();
#pragma unroll
                for (int j = 0; j < KMAX; ++j) val[j][i] = 0.0;
            }
            if (a.rf_x != nullptr) {                                 // (uniform) the table has cells in three or more regions
                const int xi = active ? a.rf_x[c0 + i] : -1;
                if (xi >= 0) {                                       // rare lanes: the cell's values for its extra entries
                    double* ex = a.rf_ex + ((int64_t)at_slot * a.rf_nx + xi) * K1;
#pragma unroll
                    for (int j = 0; j < KMAX; ++j)
                        if (j < K) ex[j] = val[j][i];
                    ex[K] = ok[i] ? 1.0 : 0.0;
                }
            }
        }
        // (the lanes' bit fields are made opaque here: tested where they are used, the compiler would otherwise hoist all the lane
        // masks they decode to out of the time loop — two dozen scalar register pairs that spilled into v_readlane traffic)
        typedef uint32_t u2 __attribute__((ext_vector_type(2)));
        const u2 lw = *(const __attribute__((address_space(3))) u2*)(rf_park + VEC * 16);
        uint32_t rb = lw.x, rr = lw.y;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("; rf_emit: begin" : "+v"(rb), "+v"(rr));
#endif
        // Per entry: the lane conditions and store addresses once, then the columns in blocks of CB.  The column list is fixed at
        // compile time — the validity weight first, then val[0 .. KMAX) — so nothing inside the scan branches on K: columns beyond K
        // carry whatever their registers hold through the shuffles and only their stores are skipped (the weight is stored at index K
        // of the record).  Per block: products, the lane's own stretch, the scan steps some run of the tile needs (a shuffle = two
        // DPP moves, dpp64 below; the adds run under the lanes' take / start / end bits as branches on lane
        // conditions, i.e. EXEC masks, not selects), the sums of the runs that end in this lane.
        constexpr int CB = RF_CB, NCOL = KMAX + 1;
        // the scan's data movement as DPP moves (no LDS round trip): steps 0 - 3 shift by 1, 2, 4, 8 lanes inside each row of 16
        // (row_shr), step 4 hands every row's last lane to the next row (row_bcast:15 -> rows 1 and 3), step 5 lane 31 to rows 2 and 3
        // (row_bcast:31); `carried` is the whole wave shifted by one lane (wave_shr:1).  Lanes without a source keep 0 — they never add.
        auto dpp64 = [&](double x, int st) -> double {
            const int xl = __double2loint(x), xh = __double2hiint(x);
            int lo, hi;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "=v"(lo));                             // (lanes a move does not write keep what the register held: no zeroing —
            asm volatile("" : "=v"(hi));                             // they are the lanes that do not add at this step)
#else
            lo = hi = 0;
#endif
            switch (st) {
                case 0: lo = __builtin_amdgcn_update_dpp(lo, xl, 0x111, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, xh, 0x111, 0xf, 0xf, false); break;
                case 1: lo = __builtin_amdgcn_update_dpp(lo, xl, 0x112, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, xh, 0x112, 0xf, 0xf, false); break;
                case 2: lo = __builtin_amdgcn_update_dpp(lo, xl, 0x114, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, xh, 0x114, 0xf, 0xf, false); break;
                case 3: lo = __builtin_amdgcn_update_dpp(lo, xl, 0x118, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, xh, 0x118, 0xf, 0xf, false); break;
                case 4: lo = __builtin_amdgcn_update_dpp(lo, xl, 0x142, 0xa, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, xh, 0x142, 0xa, 0xf, false); break;
                case 5: lo = __builtin_amdgcn_update_dpp(lo, xl, 0x143, 0xc, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, xh, 0x143, 0xc, 0xf, false); break;
                default: lo = __builtin_amdgcn_update_dpp(lo, xl, 0x138, 0xf, 0xf, false); hi = __builtin_amdgcn_update_dpp(hi, xh, 0x138, 0xf, 0xf, false); break;
            }
            return __hiloint2double(hi, lo);
        };
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            int need = rf_need[e];
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+s"(need));                           // (the same for the wave's step mask: s_bitcmp here, not a spilled mask per step)
#endif
            if (!(need & 128)) continue;                             // (uniform) no cell of this tile has an entry e
            const uint32_t bits = rb >> (16 * e), rid = rr >> (16 * e);
            double rfw0[VEC];                                        // the cells' weights for this entry, from the lane's parking block
            if constexpr (!RF_SLIM) {
#pragma unroll
                for (int i = 0; i < VEC; ++i) rfw0[i] = *(const __attribute__((address_space(3))) double*)(rf_park + i * 16 + e * 8);
            }
            double* out0 = a.rf_out + (int64_t)at_slot * a.rf_slot_stride + (int64_t)rf_first[e] * a.rf_run_stride;
            double* dst0_ = nullptr; double* dst1_ = nullptr;
            if constexpr (!RF_SLIM) {
                dst0_ = out0 + (int64_t)(rid & 0xffu) * a.rf_run_stride;              // where this lane's cells store, if they end a run
                dst1_ = out0 + (int64_t)((rid >> 8) & 0xffu) * a.rf_run_stride;
            }
#define dst0 (RF_SLIM ? out0 + (int64_t)(rid & 0xffu) * a.rf_run_stride : dst0_)
#define dst1 (RF_SLIM ? out0 + (int64_t)((rid >> 8) & 0xffu) * a.rf_run_stride : dst1_)
            const bool joins = !((bits >> 7) & 1u), fresh = ((bits >> 6) & 1u) != 0u, end0 = ((bits >> 8) & 1u) != 0u, end1 = ((bits >> 9) & 1u) != 0u;
#pragma unroll
            for (int q0 = 0; q0 < NCOL; q0 += CB) {                  // q: position in the column list (0 = the weight, q >= 1: val[q - 1])
                if (q0 > K) continue;                                // (uniform: the block's first value column is val[q0 - 1])
                double v[CB], p0[CB];
                double rfw[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) rfw[i] = RF_SLIM ? *(const __attribute__((address_space(3))) double*)(rf_park + i * 16 + e * 8) : rfw0[i];
#pragma unroll
                for (int qq = 0; qq < CB; ++qq) {
                    const int q = q0 + qq;
                    v[qq] = 0.0; p0[qq] = 0.0;
                    if (q < NCOL) {
                        // (the validity weight's product w * 1 / w * 0 is a select)
                        p0[qq] = q == 0 ? (ok[0] ? rfw[0] : 0.0) : __dmul_rn(rfw[0], val[q == 0 ? 0 : q - 1][0]);
                        v[qq] = VEC == 2 ? (q == 0 ? (ok[VEC - 1] ? rfw[VEC - 1] : 0.0) : __dmul_rn(rfw[VEC - 1], val[q == 0 ? 0 : q - 1][VEC - 1])) : p0[qq];
                    }
                }
                if constexpr (VEC == 2) {
                    if (joins) {                                     // (lanes whose second cell continues the first cell's stretch)
                        KEEP_BRANCH();
#pragma unroll
                        for (int qq = 0; qq < CB; ++qq)
                            if (q0 + qq < NCOL) v[qq] = __dadd_rn(p0[qq], v[qq]);
                    }
                }
#pragma unroll
                for (int st = 0; st < 6; ++st) {
                    if (!((need >> st) & 1)) continue;               // (uniform)
                    double pv[CB];
#pragma unroll
                    for (int qq = 0; qq < CB; ++qq) pv[qq] = q0 + qq < NCOL ? dpp64(v[qq], st) : 0.0;
                    if ((bits >> st) & 1u) {
                        KEEP_BRANCH();
#pragma unroll
                        for (int qq = 0; qq < CB; ++qq)
                            if (q0 + qq < NCOL) v[qq] = __dadd_rn(v[qq], pv[qq]);
                    }
                }
                // record index of list position q: the weight at K, val[q - 1] at q - 1 (stored when q - 1 < K)
                if constexpr (VEC == 2) {
                    if (need & 64) {                                 // (uniform) a run ends at some lane's FIRST cell: what the previous lanes
                        double carried[CB];                          // carried (unless the cell starts a stretch) + the cell
                        // (names `lane` and nothing else: the closure's layout, and with it the register allocation of the float32 two-cell
                        // twins, hangs on this lambda capturing it here — profiles/feature_bits_refactor.txt)
                        (void)lane;
#pragma unroll
                        for (int qq = 0; qq < CB; ++qq) carried[qq] = q0 + qq < NCOL ? dpp64(v[qq], 6) : 0.0;
                        if (end0) {
                            KEEP_BRANCH();
                            if (!fresh) {
                                KEEP_BRANCH();
#pragma unroll
                                for (int qq = 0; qq < CB; ++qq)
                                    if (q0 + qq < NCOL) p0[qq] = __dadd_rn(carried[qq], p0[qq]);
                            }
#pragma unroll
                            for (int qq = 0; qq < CB; ++qq) {
                                const int q = q0 + qq;
                                if (q == 0) dst0[K] = p0[qq];
                                else if (q < NCOL && q - 1 < K) dst0[q - 1] = p0[qq];
                            }
                        }
                    }
                    if (end1) {
                        KEEP_BRANCH();
#pragma unroll
                        for (int qq = 0; qq < CB; ++qq) {
                            const int q = q0 + qq;
                            if (q == 0) dst1[K] = v[qq];
                            else if (q < NCOL && q - 1 < K) dst1[q - 1] = v[qq];
                        }
                    }
                } else {
                    if (end0) {
                        KEEP_BRANCH();
#pragma unroll
                        for (int qq = 0; qq < CB; ++qq) {
                            const int q = q0 + qq;
                            if (q == 0) dst0[K] = v[qq];
                            else if (q < NCOL && q - 1 < K) dst0[q - 1] = v[qq];
                        }
                    }
                }
            }
        }
#undef dst0
#undef dst1
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("; rf_emit: end");
#endif
    };

    // ---- end of an inner group: column values, transforms, outer accumulation ----
    auto group_end = [&](bool emit_slot, int nsteps, double inv_n, int zoff, int gidx) {
        const bool empty = nsteps == 0;
        const double dn = (double)nsteps;
        bool hasnan[VEC];
        double mean[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            if constexpr (PAIR) hasnan[i] = pnan[i];
            else hasnan[i] = ((nanmask[i] >> lane) & 1ull) != 0ull;
            if constexpr (PAIR && GL == 3) mean[i] = div_by(s[i], 3.0, 1.0 / 3.0);      // == s / 3 bit for bit (1.0 / 3.0: the correctly rounded reciprocal)
            else if constexpr (PAIR && RAG) mean[i] = div_by(s[i], dn, inv_n);          // the group's own length (1 .. 4)
            else if constexpr (PAIR) mean[i] = s[i] * (1.0 / GL);      // == s / 2 (s / 4) bit for bit
            else mean[i] = (STAT >= 1) ? div_by(s[i], dn, inv_n) : 0.0;      // == s / dn bit for bit (inv_n = RN(1/n))
        }
        // single-sine degree days of one column (nb_kernels.py:218-251).  The reciprocal of the window's range and the arcs are
        // only evaluated where a threshold lies strictly inside (tmin, tmax): a branch on a lane condition skips the whole wave
        // when no lane needs it (coherent real data: most wave-days), and the other two cases are one subtraction.
        auto sine_column = [&](const ColOp& co, double (&x)[VEC]) {
            const double INV_PI = 0.31830988618379067154;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const double tavg = mean[i];
                bool in0 = false, in1 = false;
                if constexpr (PAIR && GL == 2 && LEAN) {
                    // (the lean pair form tests its windows on 2 thr - s, below)
                } else if constexpr (PAIR && GL == 2 && sizeof(TIn) == 4) {       // float data: exact float compares against the rounded thresholds
                    in0 = (plo[i] < co.s0up) && (phi[i] > co.s0dn);
                    in1 = (plo[i] < co.s1up) && (phi[i] > co.s1dn);
                } else {
                    in0 = (mn[i] < co.s0) && (co.s0 < mx[i]);
                    in1 = (mn[i] < co.s1) && (co.s1 < mx[i]);
                }
                double xv;
                if constexpr (PAIR && GL == 2 && LEAN) {
                    // the lean form in DOUBLED units: D = 2 (thr - tavg) = 2 thr - s with one rounding (= 2 d bit for bit), rng = 2 alpha
                    // exact, so  tmin < thr < tmax  <=>  |D| < rng  is ONE compare per threshold instead of two (were RN(2 thr - s)
                    // to land on rng from inside, half an ulp away, the arc it skips is exactly 0: u2 = RN(rng - |D|) = 0), u2 is one
                    // add, and the column's two max() terms are one clamp of width 2 (s1 - s0), halved exactly:
                    // max(t - s0, 0) - max(t - s1, 0) = clamp(t - s0, 0, s1 - s0) — the reference's (t - s0) - (t - s1) for t >= s1 is
                    // s1 - s0 up to its own two roundings (1e-16 relative; sine_dd's contract is 1e-10)
                    // (rd: the sine-only form keeps the pair unordered — its min and max are never formed — so the range is |rd|, an abs
                    // modifier on every instruction that reads it)
                    const double rd = mx[i] - mn[i];
                    const double D0 = __fma_rn(s[i], -1.0, co.s0x2), D1 = __fma_rn(s[i], -1.0, co.s1x2);
                    const bool i0 = fabs(D0) < fabs(rd), i1 = fabs(D1) < fabs(rd);
                    double c2;
                    if (co.skind == 0) { KEEP_BRANCH(); c2 = min_vs(max0_neg(D0), co.swidth2); }
                    else c2 = min_vs(max0(D1), co.swidth2);
                    // (folding the halving and the day's add into the column's sum into one fma: built, level; r03_session2_experiments.txt)
                    if constexpr (LEAN_SINE) xv = c2;       // doubled units all the way: the table in LDS is 2 H, the emit halves
                    else xv = c2 * 0.5;
                    if (i0 || i1) {
                        // cooling: + part(s0) - part(s1); heating: the reverse; the sign rides on u2 = +-(rng - |D|)
                        double w, p, su;
                        if (i0) {
                            if (co.skind == 0) { KEEP_BRANCH(); su = fabs(rd) - fabs(D0); } else su = fabs(D0) - fabs(rd);
                            sine_pair_g(su, rd, sine_p2, w, p);
                            xv = __fma_rn(w, p, xv);
                        }
                        if (i1) {
                            if (co.skind == 0) { KEEP_BRANCH(); su = fabs(rd) - fabs(D1); } else su = fabs(D1) - fabs(rd);
                            sine_pair_g(su, rd, sine_p2, w, p);
                            xv = __fma_rn(-w, p, xv);
                        }
                    }
                } else if constexpr (PAIR && GL == 2) {
                    // tavg is the mid-range: part = max(+-(tavg - thr), 0) + [inside] alpha F(|thr - tavg| / alpha)  (sine_pair_g)
                    // thr - tavg = thr - s / 2 (s / 2 is exact: one rounding either way)
                    const double d0 = __fma_rn(s[i], -0.5, co.s0), d1 = __fma_rn(s[i], -0.5, co.s1);
                    if (co.skind == 0) { KEEP_BRANCH(); xv = max0_neg(d0) - max0_neg(d1); }
                    else xv = max0(d1) - max0(d0);
                    if (in0 || in1) {
                        const double rng = mx[i] - mn[i];               // = 2 alpha, exact
                        // cooling: + part(s0) - part(s1); heating: the reverse.  (ONE arc site for both thresholds — a lane's window
                        // rarely holds both, but some lanes of a wave hold s0 while others hold s1 on spring / autumn days — was built
                        // and measured: only 7 % fewer arcs on the ERA5-like field, and the operand selects cost more: 23.1 -> 24.9
                        // VALU per cell-step, same time; profiles/r03_kbench_c5_table_arc.txt)
                        // (the sign rides on u2 = rng - 2 |d|: a scalar branch around one instruction instead of a multiplication)
                        double w, p, su;
                        if (in0) {
                            if (co.skind == 0) { KEEP_BRANCH(); su = __fma_rn(fabs(d0), -2.0, rng); } else su = __fma_rn(fabs(d0), 2.0, -rng);
                            sine_pair_g(su, rng, sine_p2, w, p);
                            xv = __fma_rn(w, p, xv);
                        }
                        if (in1) {
                            if (co.skind == 0) { KEEP_BRANCH(); su = __fma_rn(fabs(d1), -2.0, rng); } else su = __fma_rn(fabs(d1), 2.0, -rng);
                            sine_pair_g(su, rng, sine_p2, w, p);
                            xv = __fma_rn(-w, p, xv);
                        }
                    }
                } else {
                    const double rng = mx[i] - mn[i], alpha = rng * 0.5;
                    double inv_rng = 0.0;
                    if (in0 || in1) inv_rng = rcp_range(rng);
                    if (co.skind == 0) {
                        KEEP_BRANCH();
                        xv = sine_cool(co.s0, co.s0x2, in0, mn[i], mx[i], tavg, alpha, inv_rng, sine_tab)
                           - sine_cool(co.s1, co.s1x2, in1, mn[i], mx[i], tavg, alpha, inv_rng, sine_tab);
                    } else {
                        xv = -sine_heat(co.s0, in0, mn[i], mx[i], tavg, alpha, 2.0 * inv_rng, sine_tab)
                           + sine_heat(co.s1, in1, mn[i], mx[i], tavg, alpha, 2.0 * inv_rng, sine_tab);
                    }
                }
                if constexpr (LEAN) {
                    x[i] = xv;                                  // the NaN pairs are kept in nanacc (below)
                } else {
                    // a NaN window: any NaN will do — only the high word is replaced (one v_cndmask instead of two)
                    const int hi = (hasnan[i] || empty) ? 0x7ff80000 : __double2hiint(xv);
                    x[i] = __hiloint2double(hi, __double2loint(xv));
                }
            }
        };
        if constexpr (LEAN) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) nanacc[i] |= __builtin_amdgcn_ballot_w64(pnan[i]);
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                if (j < K) {
                    double x[VEC];
                    if constexpr (LEAN_SINE) {
                        sine_column(a.cols[j], x);              // a.cols[j]: loop-invariant kernel argument, scalar registers
                    } else {
                        // (the empty asm makes the word opaque at this point: the six words stay in scalar registers through the time
                        // loop while their decoded fields — a multiplier, masks and a trip count per column — are NOT hoisted out of
                        // it, where they overflowed the scalar register file and came back through v_readlane)
                        uint32_t cc = a.ccode[j];
#if defined(__HIP_DEVICE_COMPILE__)
                        asm volatile("" : "+s"(cc));
#endif
                        const int src = (int)(cc & 15u);
                        if (SINE && src == SRC_SINE) {
                            KEEP_BRANCH();
                            // (the full record of a sine_dd column is read where it is used: zoff is 0, but only known at run time)
                            if constexpr (SINE) { const ColOp co = a.cols[KMAX > 2 ? j + zoff : j]; sine_column(co, x); }
                        } else if constexpr (STAT == 1) {
                            // mean | sum: s / n with n = 2 or 4 is s * (1 / n) exactly; one multiply by a scalar either way (n = 3: the
                            // correctly rounded quotient, already in mean[])
                            const double sc = src == SRC_SUM ? 1.0 : 1.0 / GL;
#pragma unroll
                            for (int i = 0; i < VEC; ++i) x[i] = ((GL == 3 || RAG) && src != SRC_SUM) ? mean[i] : s[i] * sc;
                        } else {
#pragma unroll
                            for (int i = 0; i < VEC; ++i) {
                                x[i] = mean[i];                                        // SRC_MEAN: (u + v) / 2, the reference's s / n
                                if (src == SRC_SUM) x[i] = s[i];
                                if (STAT >= 2 && src == SRC_MIN) x[i] = mn[i];
                                if (STAT >= 2 && src == SRC_MAX) x[i] = mx[i];
                            }
                        }
                        // (continuing ONE double-double chain through consecutive exponents of a polynomial — 3 steps instead of 6 for
                        // power[1..4] — was built and measured: the chain state's registers cost more than the steps save, 5.8 -> 6.5 ms
                        // on 1801 x 3600 f32; profiles/r03_pairs_mean_poly.txt)
                        // powi_dd_vec's chain for exponents >= 2 (the host keeps e < 1 off the lean forms; e = 1 adds x itself),
                        // written out: nested scalar branches with straight-line code for the squares, cubes and fourth powers of a
                        // polynomial, and the column's add at every leaf (one merged add would cost a register copy per path)
                        const int n = ((cc >> 4) & 15u) == (uint32_t)TF_POWI ? (int)(cc >> 8) : 1;
                        if (n >= 2) {
                            KEEP_BRANCH();
                            double hi[VEC], lo[VEC];
#pragma unroll
                            for (int i = 0; i < VEC; ++i) hi[i] = x[i] * x[i];
                            if (n >= 3) {
                                KEEP_BRANCH();
                                auto step = [&]() {
#pragma unroll
                                    for (int i = 0; i < VEC; ++i) {
                                        const double p = hi[i] * x[i];
                                        const double err = __fma_rn(hi[i], x[i], -p);
                                        lo[i] = __fma_rn(lo[i], x[i], err);
                                        hi[i] = p;
                                    }
                                };
#pragma unroll
                                for (int i = 0; i < VEC; ++i) lo[i] = __fma_rn(x[i], x[i], -hi[i]);
                                step();
                                if (n >= 4) {
                                    KEEP_BRANCH();
                                    step();
                                    if (n > 4) {
                                        KEEP_BRANCH();
                                        for (int it = 4; it < n; ++it) step();
                                    }
                                }
#pragma unroll
                                for (int i = 0; i < VEC; ++i) os[j][i] += powi_finish(hi[i], lo[i]);      // (an overflowed power adds +-inf, not NaN)
                                asm volatile("; leaf: x^n, n >= 3");          // (distinct tails: the leaves are not merged back)
                            } else {
#pragma unroll
                                for (int i = 0; i < VEC; ++i) os[j][i] += hi[i];
                                asm volatile("; leaf: x^2");
                            }
                            continue;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < VEC; ++i) os[j][i] += x[i];
                }
            }
            if (emit_slot) {
                if (RF && a.rf_w != nullptr) {
                    KEEP_BRANCH();
                    double val[KMAX][VEC];
#pragma unroll
                    for (int j = 0; j < KMAX; ++j)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) val[j][i] = ((nanacc[i] >> lane) & 1ull) ? nan64() : (LEAN_SINE ? os[j][i] * 0.5 : os[j][i]);
                    if constexpr (RF) rf_emit(val, slot);
                } else {
#pragma unroll
                for (int j = 0; j < KMAX; ++j) {
                    if (j < K) {
                        double* dst = a.partial + ((int64_t)slot * K + j) * C + c0;
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            const double val = ((nanacc[i] >> lane) & 1ull) ? nan64() : (LEAN_SINE ? os[j][i] * 0.5 : os[j][i]);
                            if (active) dst[i] = val;
                        }
                    }
                }
                }
#pragma unroll
                for (int i = 0; i < VEC; ++i) nanacc[i] = 0ull;
                ++slot;
                reset_outer();
            }
            return;
        }
        uint64_t pk[VEC][4];
        if constexpr (SL && TKI) {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
#pragma unroll
                for (int u = 0; u < 4; ++u) pk[i][u] = 0ull;
        }
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (j < K) {
                // zoff is 0, but only known at run time (it comes from the group table word): the column
                // record is then read from the kernel-argument segment HERE, by scalar loads, instead of
                // being hoisted out of the time loop into ~18 SGPRs per column — which overflowed the
                // SGPR file and came back as v_readlane (VALU) traffic in every group end.
                const ColOp co = a.cols[j + zoff];
                // Every test on a column field below is wave-uniform.  KEEP_BRANCH() pins those tests
                // as real scalar branches: left alone, hipcc if-converts the cheap-looking arms (a
                // float round trip, 1/x for negative exponents) and runs them on every group end.
                double x[VEC];
                const int src = co.src;
                if (SINE && STAT >= 2 && src == SRC_SINE) {
                    KEEP_BRANCH();
                    if constexpr (SINE && STAT >= 2) sine_column(co, x);
                } else
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const bool bad = hasnan[i] || empty;
                    x[i] = nan64();
                    if (STAT >= 1 && src == SRC_MEAN) x[i] = bad ? nan64() : mean[i];
                    else if (STAT >= 1 && src == SRC_SUM) x[i] = bad ? nan64() : s[i];
                    else if (STAT >= 2 && src == SRC_MIN) x[i] = bad ? nan64() : mn[i];
                    else if (STAT >= 2 && src == SRC_MAX) x[i] = bad ? nan64() : mx[i];
                    else if (STAT == 3 && src == SRC_NANMEAN)
                        x[i] = (empty || cnt[i] == 0) ? nan64() : s[i] / (double)cnt[i];
                    else if (NTHR > 0 && src == SRC_THR) {
                        double t = 0.0;
                        bool poisons = false;
#pragma unroll
                        for (int q = 0; q < NTHR; ++q)
                            if (q == co.src_idx) {
                                if constexpr (HB && EB) {
                                    // (the slot's bin is made opaque here: left visible, the sixteen counter addresses — and a copy of their
                                    // common term each — were hoisted out of the time loop into 27 VGPRs, a wave per SIMD or two)
                                    int bin = a.hb_bin_of_slot[q] + 1;
#if defined(__HIP_DEVICE_COMPILE__)
                                    asm volatile("" : "+s"(bin));
#endif
                                    t = (double)hcnt[(bin * VEC + i) * bd + tid];
                                } else if constexpr (HB) t = (double)hcnt[((a.hb_bin_of_slot[q] + 1) * VEC + i) * bd + tid];
                                else t = TKI ? (double)cthr[q][i] : acc[q][i];
                                poisons = a.thr[q].nan_poisons != 0;
                            }
                        x[i] = (empty || (poisons && hasnan[i])) ? nan64() : t;
                    }
                }
                if (co.rounding & 1) {                                // the reference stored this step in float32
                    KEEP_BRANCH();
#pragma unroll
                    for (int i = 0; i < VEC; ++i) x[i] = (double)(float)x[i];
                }
                const int tf = co.tf;
                if (tf == TF_POWI) {
                    powi_dd_vec<VEC>(x, co.tf_iarg);
                } else if (tf == TF_HINGE) {
                    KEEP_BRANCH();
                    if (co.rounding & 2) {
                        const float kf = (float)co.tf_arg;
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            const float xf = (float)x[i];
                            x[i] = (double)(((xf > kf) ? 1.0f : 0.0f) * (xf - kf));
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) x[i] = ((x[i] > co.tf_arg) ? 1.0 : 0.0) * (x[i] - co.tf_arg);
                    }
                } else if (GENERAL_TF && tf == TF_POW) {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) x[i] = pow(x[i], co.tf_arg);
                } else if (GENERAL_TF && tf == TF_INTER) {
                    // np.multiply(block, other) (dataset.py:563): this group's value times other[g][cell]; lanes beyond the
                    // grid re-read valid cells (c_ld) and are never stored
                    KEEP_BRANCH();
                    const int64_t at = (int64_t)gidx * C + c_ld;
                    if (co.inter_f32) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) x[i] *= (double)((const float*)co.inter)[at + i];
                    } else {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) x[i] *= ((const double*)co.inter)[at + i];
                    }
                    if (co.rounding & 2) {                            // float32 times float32 stays float32 in the reference
#pragma unroll
                        for (int i = 0; i < VEC; ++i) x[i] = (double)(float)x[i];
                    }
                }
                if constexpr (SL && TKI) {
                    if (a.packed) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            const uint64_t u = (x[i] != x[i]) ? (uint64_t)a.pk_mask : (uint64_t)(uint32_t)x[i];
                            const int wi = a.pk_word[j];
                            const uint64_t f = u << a.pk_shift[j];
#pragma unroll
                            for (int w = 0; w < 4; ++w) pk[i][w] |= (wi == w) ? f : 0ull;
                        }
                        continue;
                    }
                }
                if constexpr (SL) {
                    if (active) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) a.partial[((int64_t)slot * K + j) * C + c0 + i] = x[i];
                    }
                    continue;
                }
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const double xi = x[i];
                    double o = os[j][i];
                    switch (co.outer) {
                        case OUT_FIRST: o = xi; break;
                        case OUT_SUM:
                        case OUT_MEAN: o += xi; break;              // NaN is sticky
                        case OUT_MIN: { double t = (xi < o) ? xi : o; o = (xi != xi) ? xi : t; break; }
                        case OUT_MAX: { double t = (xi > o) ? xi : o; o = (xi != xi) ? xi : t; break; }
                        case OUT_DD: {
                            const bool m = (xi > co.o0) && (xi < co.o1);
                            o += (xi != xi) ? xi : (m ? fabs(xi - co.obase) : 0.0);
                            break;
                        }
                        default: {  // OUT_BINS: a NaN value is simply out of range
                            const bool m = (xi > co.o0) && (xi < co.o1);
                            o += m ? 1.0 : 0.0;
                            break;
                        }
                    }
                    os[j][i] = o;
                }
            }
        }
        if constexpr (SL && TKI) {
            if (a.packed && active) {
                typedef uint32_t u4 __attribute__((ext_vector_type(4)));
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const u4 lo = u4{(uint32_t)pk[i][0], (uint32_t)(pk[i][0] >> 32), (uint32_t)pk[i][1], (uint32_t)(pk[i][1] >> 32)};
                    if (a.pk_nw == 2) {
                        // non-temporal stores: the records are not read again by this kernel; measured 1.9 % faster
                        // than plain stores on configs[3] (sc0 sc1 stores 1.6 %), profiles/r01_ab_packed_store_policy.txt
                        __builtin_nontemporal_store(lo, (u4*)((char*)a.partial + ((int64_t)slot * C + c0 + i) * 16));
                    } else {
                        u4* dst = (u4*)((char*)a.partial + ((int64_t)slot * C + c0 + i) * 32);
                        __builtin_nontemporal_store(lo, dst);
                        __builtin_nontemporal_store(u4{(uint32_t)pk[i][2], (uint32_t)(pk[i][2] >> 32), (uint32_t)pk[i][3], (uint32_t)(pk[i][3] >> 32)}, dst + 1);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            s[i] = 0.0; mn[i] = inf64(); mx[i] = -inf64(); cnt[i] = 0; nanmask[i] = 0ull;
#pragma unroll
            for (int j = 0; j < NTHR; ++j) { if (HB) {} else if (TKI) cthr[j][i] = 0; else acc[j][i] = 0.0; }
        }
        if constexpr (HB) {
            for (int b = 0; b < hb_bins * VEC; ++b) hcnt[b * bd + tid] = 0;
        }
        if constexpr (SL) {
            ++slot;
        } else if (emit_slot) {
            if (RF && a.rf_w != nullptr) {
                KEEP_BRANCH();
                if constexpr (RF) rf_emit(os, slot);
            } else if (active) {
#pragma unroll
                for (int j = 0; j < KMAX; ++j) {
                    if (j < K) {
                        double* dst = a.partial + ((int64_t)slot * K + j) * C + c0;
#pragma unroll
                        for (int i = 0; i < VEC; ++i) dst[i] = os[j][i];
                    }
                }
            }
            ++slot;
            reset_outer();
        }
    };

    int kk = 0;                 // row index relative to the chunk
    int g = g_lo;

    // ---- packed cubes with several unpack rules (FusedArgs::n_rules > 1) ----
    // pr: the rule that holds the row about to be consumed; rule_at: its index; rule_next: the chunk-relative row at which the next rule
    // starts (INT32_MAX: not inside this chunk).  All scalars.  The workgroup finds the rule of its first row by a binary search over the
    // bounds (invariant: bounds[lo] <= k_lo < bounds[hi]; every index read lies in 0 .. n_rules) and from there on reads a rule — ten
    // scalar words — only at a row where it changes.  One rule: a scalar branch skips all of it, pr is the argument record's rule and
    // rule_next stays out of reach of the one compare a burst makes.
    int rule_at = 0, rule_next = INT32_MAX;
    auto rule_advance = [&]() {                      // the rule changes at the row about to be consumed
        ++rule_at;
        const int64_t b = ld_uniform(a.pack_bounds + rule_at + 1);        // (rule_at + 1 <= n_rules: the last bound is T, never a change)
        rule_next = b < k_hi ? (int)(b - k_lo) : INT32_MAX;
        pr = ld_pack_rule(a.pack_rules + rule_at);
    };
    if constexpr (PACKED) {
        pr = a.unpack;                             // (uniform fields of the argument record: scalar loads)
        if (a.n_rules > 1) {
            KEEP_BRANCH();
            int lo = 0, hi = a.n_rules;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (ld_uniform(a.pack_bounds + mid) <= k_lo) lo = mid; else hi = mid;
            }
            rule_at = lo - 1;
            rule_advance();
        }
    }

    if constexpr (PAIR) {
        const TRaw* p = cube;
        constexpr int GB = DEPTH / GL;                // groups per block of rows
        // the group's statistics: min / max in the input precision (exact), the sum in time order — for a pair min + max, the same
        // two addends the reference adds; a NaN in any row marks the lane (the group is NaN, nb_kernels.py:145-147)
        auto short_stats = [&](const RawVec<TIn, VEC>* r) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const TIn u = r[0].v[i], v = r[1].v[i];
                pnan[i] = u != u || v != v;
                if constexpr (GL == 2 && LEAN_SINE) {
                    // every column a plain sine_dd: the lean group end reads only the pair's sum and |difference| (sine_column) —
                    // no min, no max; mn / mx hold the pair as it came
                    mn[i] = (double)u; mx[i] = (double)v;
                    s[i] = mn[i] + mx[i];
                    continue;
                }
                // v_min / v_max straight on the loaded values: the builtins first canonicalise both operands (v_max x, x)
                // against signalling NaNs; a group with any NaN is a NaN group anyway
                TIn lo, hi;
                if constexpr (sizeof(TIn) == 4) {
                    asm("v_min_f32 %0, %1, %2" : "=v"(lo) : "v"(u), "v"(v));
                    asm("v_max_f32 %0, %1, %2" : "=v"(hi) : "v"(u), "v"(v));
                } else {
                    asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(u), "v"(v));
                    asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(u), "v"(v));
                }
                if constexpr (GL == 2) {
                    plo[i] = lo; phi[i] = hi;
                    mn[i] = (double)lo; mx[i] = (double)hi;
                    s[i] = mn[i] + mx[i];
                    if constexpr (STAT == 1) s[i] = (double)u + (double)v;     // (the same two addends; no min / max needed)
                } else if constexpr (GL == 3) {
                    const TIn u2 = r[2].v[i];
                    pnan[i] = pnan[i] || u2 != u2;
                    s[i] = ((double)u + (double)v) + (double)u2;                            // nb_kernels.py:130-137: k ascending
                    if constexpr (STAT >= 2) {
                        if constexpr (sizeof(TIn) == 4) {
                            asm("v_min_f32 %0, %1, %2" : "=v"(lo) : "v"(lo), "v"(u2));
                            asm("v_max_f32 %0, %1, %2" : "=v"(hi) : "v"(hi), "v"(u2));
                        } else {
                            asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(lo), "v"(u2));
                            asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(hi), "v"(u2));
                        }
                        plo[i] = lo; phi[i] = hi;
                        mn[i] = (double)lo; mx[i] = (double)hi;
                    }
                } else {
                    const TIn u2 = r[2].v[i], u3 = r[3].v[i];
                    pnan[i] = pnan[i] || u2 != u2 || u3 != u3;
                    s[i] = (((double)u + (double)v) + (double)u2) + (double)u3;             // nb_kernels.py:130-137: k ascending
                    if constexpr (STAT >= 2) {
                        TIn lo2, hi2;
                        if constexpr (sizeof(TIn) == 4) {
                            asm("v_min_f32 %0, %1, %2" : "=v"(lo2) : "v"(u2), "v"(u3));
                            asm("v_max_f32 %0, %1, %2" : "=v"(hi2) : "v"(u2), "v"(u3));
                            asm("v_min_f32 %0, %1, %2" : "=v"(lo) : "v"(lo), "v"(lo2));
                            asm("v_max_f32 %0, %1, %2" : "=v"(hi) : "v"(hi), "v"(hi2));
                        } else {
                            asm("v_min_f64 %0, %1, %2" : "=v"(lo2) : "v"(u2), "v"(u3));
                            asm("v_max_f64 %0, %1, %2" : "=v"(hi2) : "v"(u2), "v"(u3));
                            asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(lo), "v"(lo2));
                            asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(hi), "v"(hi2));
                        }
                        plo[i] = lo; phi[i] = hi;
                        mn[i] = (double)lo; mx[i] = (double)hi;
                    }
                }
            }
        };
        // Loads run one block ahead, group by group: as soon as a group's rows have been reduced to its statistics the same
        // group's rows of the NEXT block are requested, so the memory pipe works while the arcs run (a block that loads, then
        // waits, then computes left it idle: VALU busy 0.81 of the kernel; with this 0.90).  The requests sit under the branch
        // "the next block has this group", which makes the compiler land them in fresh registers and move them into place at the
        // loop's back edge behind one s_waitcnt vmcnt(0).  The textbook form — unconditional loads straight into the ring's
        // registers, counted waits vmcnt(DEPTH - GL) per group, no moves — was built too and measured BEHIND this one on every
        // short-group shape (C5 3.59 vs 3.53 ms, mean -> power[1..4] -> sum f32 5.66 vs 5.53, f64 3.74 vs 3.61; the old
        // load-wait-compute block on the latter two: 5.76 / 3.90; profiles/r03_short_group_loads.txt); depths 4, 6, 8 measure alike.
        // Addresses: ONE scalar row pointer that advances by a row per load, in a buffer descriptor, + the lane's 32-bit byte
        // offset — no vector address arithmetic (a global_load needs a v_lshl_add_u64 per row) and two scalar adds per row; the host
        // keeps plans whose rows reach 4 GiB off this path.
        const char* nx = (const char*)a.cube + (size_t)(k_lo * C) * sizeof(TRaw);      // the next row to load (uniform)
        const uint32_t voff = (uint32_t)((uint64_t)c_ld * sizeof(TRaw));
        const size_t rowb = (size_t)C * sizeof(TRaw);
        // Packed cubes: the rows wait in their registers as 2-byte elements (TRaw) and a group's rows are unpacked to float32 right in
        // front of its statistics, in time order — `n` rows from chunk-relative row `row0`.  Several rules: the scheme of the general
        // path (`pr`, rule_next, rule_advance), `straddles` being the caller's one scalar compare for the rows it is about to consume;
        // only then is each row tested, and the next rule read at the row where it starts.  From here on the code is the float32 form's.
        auto unpack_rows = [&](const RawVec<TRaw, VEC>* rr, int n, int row0, bool straddles, RawVec<TIn, VEC>* u) {
            if constexpr (PACKED) {
#pragma unroll
                for (int d = 0; d < GL; ++d) {
                    if (d == 0 || d < n) {
                        if (straddles && row0 + d == rule_next) { KEEP_BRANCH(); rule_advance(); }
                        unpack_i16<VEC>(rr[d].v, pr, u[d].v);
                    } else {
                        u[d] = u[0];                   // (never read: the statistics stop at the group's length)
                    }
                }
            }
        };
        if constexpr (RAG) {
            // groups of one to four rows: slot q of the block holds group g + q in its four row registers, as many of them filled
            // as the group is long.  Rows are requested in time order through the one scalar row pointer, a group's successor in
            // its slot (group g + GB + q) as soon as its own rows have been reduced — the uniform forms' schedule with a scalar
            // trip count on the loads.
            auto rag_stats = [&](const RawVec<TIn, VEC>* rr, int len) {
                TIn lo[VEC], hi[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) {
                    const TIn u = rr[0].v[i];
                    pnan[i] = u != u; s[i] = (double)u; lo[i] = u; hi[i] = u;
                }
#pragma unroll
                for (int d = 1; d < GL; ++d) {
                    if (d < len) {
                        KEEP_BRANCH();
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            const TIn v = rr[d].v[i];
                            pnan[i] = pnan[i] || v != v;
                            s[i] += (double)v;                                      // nb_kernels.py:130-137: k ascending
                            if constexpr (STAT >= 2) {
                                if constexpr (sizeof(TIn) == 4) {
                                    asm("v_min_f32 %0, %1, %2" : "=v"(lo[i]) : "v"(lo[i]), "v"(v));
                                    asm("v_max_f32 %0, %1, %2" : "=v"(hi[i]) : "v"(hi[i]), "v"(v));
                                } else {
                                    asm("v_min_f64 %0, %1, %2" : "=v"(lo[i]) : "v"(lo[i]), "v"(v));
                                    asm("v_max_f64 %0, %1, %2" : "=v"(hi[i]) : "v"(hi[i]), "v"(v));
                                }
                            }
                        }
                    }
                }
                if constexpr (STAT >= 2) {
#pragma unroll
                    for (int i = 0; i < VEC; ++i) { plo[i] = lo[i]; phi[i] = hi[i]; mn[i] = (double)lo[i]; mx[i] = (double)hi[i]; }
                }
            };
            RawVec<TRaw, VEC> r[DEPTH];
            int lens[GB];
            int k_next = (int)k_lo;                     // the next row to request (the cube's row index)
#pragma unroll
            for (int q = 0; q < GB; ++q) {
                lens[q] = 0;
                if (g + q < g_hi) {
                    const int e = (int)(ld_uniform(&a.gtab[2 * (g + q)]) >> 1) & 0x7fffffff;
                    lens[q] = e - k_next;
                    k_next = e;
                }
#pragma unroll
                for (int d = 0; d < GL; ++d) {
                    if (d < lens[q]) { r[GL * q + d] = ld_stream_row<TRaw, VEC, AUX>(nx, voff); nx += rowb; }
                    else r[GL * q + d] = r[0];         // (never read: the statistics stop at the group's length)
                }
            }
            while (g < g_hi) {
                const int ng = (g_hi - g) < GB ? (g_hi - g) : GB;
#pragma unroll
                for (int q = 0; q < GB; ++q) {
                    if (q < ng) {
                        const int64_t w = ld_uniform(&a.gtab[2 * (g + q)]);
                        const int len = lens[q];
                        if constexpr (PACKED) {
                            const int gend = ((int)(w >> 1) & 0x7fffffff) - (int)k_lo;        // the group's end, chunk-relative
                            RawVec<TIn, VEC> u[GL];
                            unpack_rows(&r[GL * q], len, gend - len, gend > rule_next, u);
                            rag_stats(u, len);
                        } else {
                            rag_stats(&r[GL * q], len);
                        }
                        if (g + GB + q < g_hi) {
                            const int e = (int)(ld_uniform(&a.gtab[2 * (g + GB + q)]) >> 1) & 0x7fffffff;
                            const int ln = e - k_next;
                            k_next = e;
                            lens[q] = ln;
#pragma unroll
                            for (int d = 0; d < GL; ++d) {
                                if (d < ln) { r[GL * q + d] = ld_stream_row<TRaw, VEC, AUX>(nx, voff); nx += rowb; }
                            }
                        }
                        const double inv = len == 3 ? 1.0 / 3.0 : (len == 2 ? 0.5 : (len == 4 ? 0.25 : 1.0));
                        group_end((w & 1) != 0, len, inv, (int)((uint64_t)w >> 63), g + q);
                    }
                }
                g += ng;
            }
        } else {
        RawVec<TRaw, VEC> r[DEPTH];
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) {
            if (d < rows) { r[d] = ld_stream_row<TRaw, VEC, AUX>(nx, voff); nx += rowb; }
            else r[d] = r[0];                      // (a chunk shorter than a block: these rows' groups are not evaluated)
        }
        while (g < g_hi) {
            const int ng = (g_hi - g) < GB ? (g_hi - g) : GB;
            bool straddles = false;                    // packed cubes: a rule starts inside this block of rows
            if constexpr (PACKED) straddles = kk + DEPTH > rule_next;
            // one copy of the group end per group of the block: since the arcs come from a table the copies fit the instruction
            // cache, and the rows need not be shifted down GL registers per group (round 2's rolled loop: 4 VALU per cell-day)
#pragma unroll
            for (int q = 0; q < GB; ++q) {
                if (q < ng) {
                    const int64_t w = ld_uniform(&a.gtab[2 * (g + q)]);
                    if constexpr (PACKED) {
                        RawVec<TIn, VEC> u[GL];
                        unpack_rows(&r[GL * q], GL, kk + GL * q, straddles, u);
                        short_stats(u);
                    } else {
                        short_stats(&r[GL * q]);
                    }
                    if (kk + DEPTH + GL * (q + 1) <= rows) {       // (groups are whole: all of the next block's group q, or none)
#pragma unroll
                        for (int d = 0; d < GL; ++d) { r[GL * q + d] = ld_stream_row<TRaw, VEC, AUX>(nx, voff); nx += rowb; }
                    }
                    group_end((w & 1) != 0, GL, 1.0 / GL, (int)((uint64_t)w >> 63), g + q);
                }
            }
            g += ng;
            kk += GL * ng;
        }
        }
    } else if constexpr (PIPE == 0) {
        const TRaw* p = cube;
        // histogram variants with arithmetic edges are issue-bound beside their stream: their rows are addressed like the short-group
        // forms' — ONE scalar row pointer in a buffer descriptor + the lane's 32-bit byte offset, no vector address arithmetic (a
        // global_load wants a 64-bit vector address: one v_lshl_add_u64 per row and lane, a fifteenth of the element's instructions);
        // the host keeps plans whose rows reach 4 GiB off these variants
        const char* nx = (const char*)a.cube + (size_t)(k_lo * C) * sizeof(TRaw);
        const uint32_t voff = (uint32_t)((uint64_t)c_ld * sizeof(TRaw));
        const size_t rowb = (size_t)C * sizeof(TRaw);
        // group table word for g is fetched one group ahead: its scalar-load latency hides behind
        // the previous group's work (matters for 1-2 step groups: daily data, tmin/tmax pairs)
        int64_t w_next = ld_uniform(&a.gtab[2 * g]), iv_next = ld_uniform(&a.gtab[2 * g + 1]);
        while (g < g_hi) {
            const int64_t w = w_next, iv = iv_next;
            w_next = ld_uniform(&a.gtab[2 * g + 2]);             // table is padded by one entry
            iv_next = ld_uniform(&a.gtab[2 * g + 3]);
            const int gend = (int)((w >> 1) - k_lo);
            const int gbeg = kk;
            // DEPTH rows in flight per lane inside a group.  (Issuing the next block's loads before the
            // current block is consumed was built and measured: no gain on any shape, -11 % on the f32
            // K = 5 plan — other waves already cover the gap, the extra live registers cost more.  A register
            // ring that re-arms each row's load right after the row is consumed, across group ends, was
            // measured too: f64 6.88 -> 6.48 TB/s, f32 unchanged.  Bursts of DEPTH rows per wave win.)
            auto load_block = [&](RawVec<TRaw, VEC> (&r)[DEPTH]) {
                if constexpr (HA) {
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) { r[d] = ld_stream_row<TRaw, VEC, AUX>(nx, voff); nx += rowb; }
                    return;
                }
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) r[d] = ld_stream<TRaw, VEC, AUX>(p + (int64_t)d * C);
                p += (int64_t)DEPTH * C;
            };
            auto use_block = [&](const RawVec<TRaw, VEC> (&r)[DEPTH]) {
                if constexpr (HA && !PACKED) {
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) consume(r[d]);
                } else if constexpr (HB && !HA && PACKED) {
                    // the table form on packed storage: an element is unpacked ONCE, under the rule of its row (the rule logic of the PACKED
                    // arm below), and guess, count and statistic all take that value; the burst's table reads are issued before the first
                    // compare needs one, as on float storage
                    const bool straddles = kk + DEPTH > rule_next;
                    TIn u[DEPTH][VEC];
                    int hb_b[DEPTH][VEC];
                    EdgeT hb_e[DEPTH][VEC];
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) {
                        if (straddles && kk + d == rule_next) { KEEP_BRANCH(); rule_advance(); }
                        unpack_i16<VEC>(r[d].v, pr, u[d]);
#pragma unroll
                        for (int i = 0; i < VEC; ++i) hb_guess(u[d][i], hb_b[d][i], hb_e[d][i]);
                    }
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) {
#pragma unroll
                        for (int i = 0; i < VEC; ++i) {
                            const TIn vr = u[d][i];
                            if constexpr (STAT == 1) {              // (what `consume` does for the histogram forms: STAT <= 1, no threshold slots)
                                nanmask[i] |= __builtin_amdgcn_ballot_w64(vr != vr);
                                s[i] += (double)vr;
                            }
                            hb_count(vr, i, hb_b[d][i], hb_e[d][i]);
                        }
                    }
                } else if constexpr (HB && !HA) {
                    int hb_b[DEPTH][VEC];
                    EdgeT hb_e[DEPTH][VEC];
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
                        for (int i = 0; i < VEC; ++i) hb_guess(r[d].v[i], hb_b[d][i], hb_e[d][i]);
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) {
                        consume(r[d], false);
#pragma unroll
                        for (int i = 0; i < VEC; ++i) hb_count(r[d].v[i], i, hb_b[d][i], hb_e[d][i]);
                    }
                } else if constexpr (PACKED) {
                    // A burst wholly inside one rule fails one scalar compare and runs as for one rule; one that straddles a change tests
                    // each of its rows and reads the next rule where it starts.  One copy of the burst's body serves both: a second,
                    // test-free copy for the common case was built — 44 of the 69 kernels lost a wave per SIMD or two to it, one gained
                    // scratch memory (profiles/packed_cube.txt, section 3).  (The arithmetic-edge histogram forms take this arm too: `consume`
                    // unpacks the row and hands each value to ha_update.)
                    const bool straddles = kk + DEPTH > rule_next;
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) {
                        if (straddles && kk + d == rule_next) { KEEP_BRANCH(); rule_advance(); }
                        consume(r[d]);
                    }
                } else {
#pragma unroll
                    for (int d = 0; d < DEPTH; ++d) consume(r[d]);
                }
            };
            for (; kk + DEPTH <= gend; kk += DEPTH) {
                RawVec<TRaw, VEC> r[DEPTH];
                load_block(r);
                use_block(r);
            }
            // the group's last rows (fewer than DEPTH; ALL rows of a group shorter than DEPTH): their loads
            // are issued together too — one at a time, a 4-step group ran at a quarter of the bandwidth
            if (kk < gend) {
                const int rem = gend - kk;
                RawVec<TRaw, VEC> r[DEPTH];
                if constexpr (HA) {
#pragma unroll
                    for (int d = 0; d < DEPTH - 1; ++d)
                        if (d < rem) { r[d] = ld_stream_row<TRaw, VEC, AUX>(nx, voff); nx += rowb; }
                } else {
#pragma unroll
                    for (int d = 0; d < DEPTH - 1; ++d)
                        if (d < rem) r[d] = ld_stream<TRaw, VEC, AUX>(p + (int64_t)d * C);
                    p += (int64_t)rem * C;
                }
                bool straddles = false;
                if constexpr (PACKED) straddles = gend > rule_next;
#pragma unroll
                for (int d = 0; d < DEPTH - 1; ++d)
                    if (d < rem) {
                        if constexpr (PACKED) {
                            if (straddles && kk + d == rule_next) { KEEP_BRANCH(); rule_advance(); }
                        }
                        consume(r[d]);
                    }
                kk = gend;
            }
            group_end((w & 1) != 0, gend - gbeg, __longlong_as_double(iv), (int)((uint64_t)w >> 63), g);
            ++g;
        }
    } else {
        // ---- LDS-DMA ring, wave-private ----
        unsigned char* ring = dynlds;                                         // waves * DEPTH KiB
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const uint32_t ring_lds = (uint32_t)(uintptr_t)(lds_ptr_t)ring;
        const uint32_t wave_lds = __builtin_amdgcn_readfirstlane(ring_lds + (uint32_t)wave * (uint32_t)lds_ring_bytes_per_wave(DEPTH));
        const uint32_t rd_lane = wave_lds + (uint32_t)lane * 16u;
        const int last = rows - 1;
        const int64_t row_bytes = C * (int64_t)sizeof(TIn);
        const char* lane_base = (const char*)cube;
        auto issue = [&](int row, int sl) {
            const int r = row < last ? row : last;                       // tail: re-load the last row
            __builtin_amdgcn_global_load_lds((glb_ptr_t)(lane_base + (int64_t)r * row_bytes),
                                             (lds_ptr_t)(uintptr_t)(wave_lds + (uint32_t)sl * 1024u), 16, 0, AUX);
        };
        int sl = 0;  // ring slot of row kk
        if (rows > 0) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) issue(d, d);
        }
        int64_t w_next = ld_uniform(&a.gtab[2 * g]), iv_next = ld_uniform(&a.gtab[2 * g + 1]);
        while (g < g_hi) {
            const int64_t w = w_next, iv = iv_next;
            w_next = ld_uniform(&a.gtab[2 * g + 2]);
            iv_next = ld_uniform(&a.gtab[2 * g + 3]);
            const int gend = (int)((w >> 1) - k_lo);
            const int gbeg = kk;
            for (; kk < gend; ++kk) {
                u32x4 raw;
                // row kk has landed once at most DEPTH-1 younger DMAs are outstanding
                asm volatile("s_waitcnt vmcnt(%1)\n\t"
                             "ds_read_b128 %0, %2\n\t"
                             "s_waitcnt lgkmcnt(0)"
                             : "=v"(raw)
                             : "n"(DEPTH - 1), "v"(rd_lane + (uint32_t)sl * 1024u)
                             : "memory");
                issue(kk + DEPTH, sl);           // slot is free again: its row is in registers
                sl = (sl + 1 == DEPTH) ? 0 : sl + 1;
                RawVec<TIn, VEC> rv;
                __builtin_memcpy(&rv, &raw, 16);
                consume(rv);
            }
            group_end((w & 1) != 0, gend - gbeg, __longlong_as_double(iv), (int)((uint64_t)w >> 63), g);
            ++g;
        }
        // no DMA may still target this workgroup's LDS when the wave retires
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

}  // namespace afhip
