// afhip_planner.h — plan building: from a plan description to the kernel variant, the chunk table and the workspace sizes.
//
// Plain C++ (the Makefile compiles afhip_planner.cpp without HIP): everything the planner decides follows from the description,
// the experiment knobs and two facts about the device, which the caller hands in (DeviceFacts).  afhip_api.hip uploads the
// tables of the layout and runs it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/aggfly_hip.h"
#include "afhip_plan_types.h"
#include "afhip_variants.h"

namespace afhip {

// The library's one error channel (afhip_last_error): sets the calling thread's message and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
const char* last_error();

// 16-bit integer storage whose values are float32 by a bound afhip_packing: one packed kernel table serves both
inline bool is_packed_dtype(int dtype) { return dtype == AFHIP_I16 || dtype == AFHIP_U16; }

// What plan building needs to know about the device.
struct DeviceFacts {
    int cu_count = 0;                                                  // compute units
    int (*resident_wgs)(const void* fn, int wg, size_t lds) = nullptr;  // workgroups of kernel `fn` one CU holds at once at `wg` threads
                                                                       // and `lds` bytes of dynamic LDS (registers, LDS, wave slots); 0: unknown
};

// Experiment knobs of the run path, read when the plan is created (never on the run path).
struct RunKnobs {
    bool counts_spmm = true;       // AFHIP_NO_COUNTS_SPMM unset — packed-count plans: gather the records directly when no per-cell output is asked for
    int counts_spmm_sub = -1;      // AFHIP_COUNTS_SPMM_SUB=0|4|8|16: lanes per (row, period) pair of the packed-count gather (0: one, table order)
    bool no_slot_spmm = false;     // AFHIP_NO_SLOT_SPMM=1: keep k_combine_slots + k_csr_spmm on every route
    int slot_spmm_sub = 0;         // AFHIP_SLOT_SPMM_SUB=8|16|32|64: lanes per (segment, period) of the slot gather
    int slot_spmm_order = -1;      // AFHIP_SLOT_SPMM_ORDER=v|p: SlotSpmmArgs::p_major forced off / on
    int rf_layout = -1;            // AFHIP_RF_LAYOUT=slot|run: layout of the run sums forced (rf_run_major)
};

// Every knob of plan creation, read once per plan by read_knobs().
struct PlanKnobs : RunKnobs {
    int force_wg = 0;              // AFHIP_FORCE_WG=64|128|256: threads per workgroup
    int wgs_per_cu = 0;            // AFHIP_WGS_PER_CU=n: workgroups per CU the chunk count aims for (switches period chunks and round fill off)
    bool no_period_chunks = false, no_round_fill = false;                    // AFHIP_NO_PERIOD_CHUNKS, AFHIP_NO_ROUND_FILL
    bool no_pair_mode = false, no_quad_mode = false, no_ragged_mode = false;  // AFHIP_NO_PAIR_MODE, AFHIP_NO_QUAD_MODE, AFHIP_NO_RAGGED_MODE
    bool no_region_fused = false;                                            // AFHIP_NO_REGION_FUSED
    bool no_packed_rf = false;     // AFHIP_NO_PACKED_RF: packed cubes' plans choose their kernels and routes as they did without the region-fused twins of MENU_PACKED_RF
    bool no_packed_hist = false;   // AFHIP_NO_PACKED_HIST: packed cubes' partition plans take the general packed kernel, not the LDS-histogram forms
    int packed_hist_vec = 0;       // AFHIP_PACKED_HIST_VEC=1|2: the cells per lane such a plan takes where the library holds the kernel, arms included (0: the planner's rule)
    bool no_packed_short = false;  // AFHIP_NO_PACKED_SHORT: packed cubes' short-group plans take the general packed kernel, not the lean short-group forms
    int packed_short_vec = 0;      // AFHIP_PACKED_SHORT_VEC=1|2|4: the cells per lane such a plan takes where the rows allow it and the library holds the kernel, arms included (0: the planner's rule)
    bool no_cell_map_hist = false; // AFHIP_NO_CELL_MAP_HIST: partitions of unequal interior widths take the route they took without the cell-map histogram forms
    bool no_end_bins_hist = false; // AFHIP_NO_END_BINS_HIST: partitions with a wide end bin take the route they took without the end-bin histogram forms
};
PlanKnobs read_knobs();

// LDS-histogram bins: the threshold slots as a contiguous equal-width partition (find_partition).  hb_n = 0: none.
struct HistPartition {
    int hb_n = 0; double hb_c1 = 0, hb_c0 = 0;
    bool hb_arith = false; double hb_w = 0, hb_lo0 = 0, hb_gl = 0, hb_gh = 0, hb_c0b = 0;   // ... with exactly representable edges (+ the biased guess constant)
    int hb_bin_of_slot[MAX_THR] = {0};
    double hb_edge[MAX_THR + 1] = {0};
    // wide end bins (FEAT_END_BINS): hb_n counts the equal-width bins only and every field above describes that lattice; the slot of a
    // wide lower end has hb_bin_of_slot = -1, that of a wide upper end hb_n (the guard bins).  hb_slot_lo / hb_slot_hi: the slots
    // whose t0 / t1 are the outer limits L / U of the whole partition
    bool hb_wide = false;
    int hb_slot_lo = 0, hb_slot_hi = 0;
    // interior bins of unequal widths (FEAT_CELL_MAP; afhip_cell_map.h): hb_wide is set, hb_c1 / hb_c0 guess one of hb_cells cells (0: none)
    // between two guard cells, and hb_cmap[cell] is the cell's guarded bin; no arithmetic edges
    int hb_cells = 0;
    uint8_t hb_cmap[256] = {0};
};

// What the planner produces.  Host data only: afhip_plan (afhip_api.hip) adds the device tables, scratch and run state.
struct PlanLayout : RunKnobs, HistPartition {
    bool has_sine = false;                // a column is sine_dd: launches carry the acos table and its LDS
    afhip_plan_desc desc{};
    std::vector<int64_t> ib, ob;          // host copies
    std::vector<afhip_column> columns;
    // lowering
    int stat = 0, nthr = 0, K = 0;
    std::vector<ThrSlot> thr;
    std::vector<ColOp> cols;               // cols[j].inter / inter_f32 are set by afhip_plan_bind_inter
    std::vector<ChunkDesc> chunks;
    std::vector<int32_t> emit;
    std::vector<int64_t> gtab;            // {(end step) << 1 | emit, bits of 1.0/len} per inner group, padded by one
    std::vector<int32_t> slot_ptr;        // [P+1]
    int64_t n_slots = 0;
    const Variant* variant = nullptr;
    const Variant* variant_rf = nullptr;   // its twin with the region-fused period ends compiled in (null: none in the menu)
    bool rf_plan_ok = false;               // the plan's columns and slots allow the route (the table decides the rest at run time)
    int64_t tiles = 0;
    int wg = WG;                          // threads per workgroup (64 for small grids, else 256)
    bool packed = false;      // single-level, all columns plain bin counts: partial holds packed records (FusedArgs::packed)
    PackFmt pk{};             // their format; pk_bw = bits per count
    int64_t ws_partial = 0, ws_panel = 0;   // workspace: byte sizes
};

// Fills `out` from `desc` (validated here).  Returns AFHIP_OK or the error code, with the message in last_error().
int build_plan(const afhip_plan_desc* desc, const DeviceFacts& dev, PlanLayout* out);

// dynamic LDS of a launch of the plan's variant with pl->wg threads per workgroup
size_t plan_lds_bytes(const PlanLayout* pl);

}  // namespace afhip
