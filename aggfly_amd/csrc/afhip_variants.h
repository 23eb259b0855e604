// afhip_variants.h — the menu of compiled k_fused_temporal specialisations.
//
// The hot per-element loop must be straight-line code with every accumulator in a
// register, so the accumulator counts are template parameters.  gen_variants.py writes
// one translation unit per group of instantiations (compiled in parallel) plus the table
// below; find_variant() picks the cheapest instantiation that covers a lowered plan.
#pragma once
#include <stdint.h>
#include "afhip_plan_types.h"

namespace afhip {

struct Variant {
    int dtype;    // AFHIP_F32 / AFHIP_F64; AFHIP_I16 in the packed table
    int pipe;     // 0 direct loads, 1 LDS-DMA ring
    int vec;      // cells per lane
    int stat;     // 0 none, 1 sum, 2 sum+min+max, 3 NaN-skipping sum+count+min+max
    int nthr;     // threshold slots
    int kmax;     // columns
    int depth;    // LDS ring depth in rows (pipe 1)
    int feat;     // FEAT_* bits (afhip_plan_types.h): what else the kernel has compiled in
    int production;   // 1: part of the default menu; 0: tuning arm only
    const void* fn;
    const char* name;

    bool nt() const { return feat_has(feat, FEAT_NT); }
    bool tki() const { return feat_has(feat, FEAT_INT_BINS); }            // integer bin counters (all threshold slots must be bins)
    bool sl() const { return feat_has(feat, FEAT_SINGLE_LEVEL); }         // single-level plans only
    bool hb() const { return feat_has(feat, FEAT_HIST); }                 // LDS-histogram bins
    bool ha() const { return feat_has(feat, FEAT_ARITH_EDGES); }          // ... with computed edges
    bool pair() const { return feat_has(feat, FEAT_SHORT_GROUP); }        // a short-group form (two rows per inner group unless group_form() says otherwise)
    int lean() const { return feat_lean_level(feat); }                    // its lean group end: 0 none, 1 lean, 2 sine-only
    int group_form() const { return feat_group_form(feat); }              // 1 four rows, 2 three rows, 3 mixed one to four; lean form only
    bool rf() const { return feat_has(feat, FEAT_REGION_FUSED); }         // the region-fused twin of the variant with the same other fields and bits
    bool sine_p2() const { return feat_sine_p2(feat); }                   // sine_dd plans: the P2 table instead of the acos table
};

const Variant* variants_table(int* n);   // generated (variants_table.hip)
const char* variants_menu();             // "full" (the production menu), "arms" (+ the tuning arms) or "dev"
// The kernels of int16- and uint16-packed cubes (AFHIP_I16, AFHIP_U16: one set, the signedness is in the unpack record;
// gen_variants.py: packed_menu), a table of their own (packed_table.hip): general
// two-level forms on the direct-load path only, so a plan's stat / slots / columns and the cells per lane are all there is to match.
const Variant* packed_variants_table(int* n);
// ... and their LDS-histogram forms (gen_variants.py: packed_hist_menu; packed_hist_table.hip): integer-bin forms for plans whose
// threshold slots are a contiguous equal-width partition, matched on cells per lane, stat tier, single level and arithmetic edges.
const Variant* packed_hist_variants_table(int* n);
// ... and the LDS-histogram forms with FEAT_END_BINS, for partitions with a wide end bin on one side or both — float32, float64 and
// packed storage in one table (gen_variants.py: end_bins_menu; end_bins_table.hip), matched like the packed histogram forms plus the dtype.
const Variant* end_bins_variants_table(int* n);

// What a lowered plan asks of the menu (afhip_planner.cpp: choose_variant).  A fallback is the same query with a field changed.
// tuning: 0 = the default choice below; otherwise an explicit arm
//         pipe*1000 + vec*100 + depth  (+10000: default cache policy instead of nt)
//         e.g. 1404 LDS ring, 4 cells per lane, depth 4;  108 direct loads, 1 cell per lane, 8 rows in flight
struct VariantQuery {
    int dtype = 0;              // AFHIP_F32 / AFHIP_F64
    int pipe = 0;               // 0 direct loads, 1 LDS-DMA ring
    int stat = 0, nthr = 0, K = 0;      // what the columns need: STAT mode, threshold slots, columns
    int tuning = 0;
    int vec = 0;                // cells per lane (0: any)
    bool all_bins = false;      // every threshold slot is a bin count
    bool single_level = false;  // one inner group per period, every outer `first`
    bool partition = false;     // the slots are a contiguous equal-width partition (LDS histogram)
    bool arith = false;         // ... with exactly representable edges
    bool pairs = false;         // every inner group holds exactly two rows
    int lean = 0;               // lean group end the plan qualifies for: 0 none, 1 lean, 2 sine-only (Variant::lean)
    int depth_hint = 0;         // among equals, the burst depth to prefer (0: none)
    int quads = 0;              // Variant::group_form of a four- / three-row / mixed short-group plan
    bool rf = false;            // the region-fused twins instead of the plain variants
};

inline const Variant* find_variant(const VariantQuery& q) {
    const int dtype = q.dtype, pipe = q.pipe, stat = q.stat, nthr = q.nthr, K = q.K, tuning = q.tuning, vec = q.vec, lean = q.lean,
              depth_hint = q.depth_hint, quads = q.quads;
    const bool all_bins = q.all_bins, single_level = q.single_level, partition = q.partition, arith = q.arith, pairs = q.pairs, rf = q.rf;
    const Variant* best = nullptr;
    long best_cost = 0;
    int n = 0;
    const Variant* tab = variants_table(&n);
    int want_nt = 1, want_pipe = pipe, want_vec = -1, want_depth = -1;
    if (tuning > 0) {
        int t = tuning;
        if (t >= 10000) { want_nt = 0; t -= 10000; }
        want_pipe = t / 1000; want_vec = (t % 1000) / 100; want_depth = t % 100;
    }
    for (int i = 0; i < n; ++i) {
        const Variant& v = tab[i];
        if (v.dtype != dtype || v.stat < stat || v.nthr < nthr || v.kmax < K || v.rf() != rf) continue;
        if ((v.tki() && !(all_bins && nthr > 0)) || (v.sl() && !single_level) || (v.hb() && !partition) || (v.ha() && !arith)) continue;
        if (v.pair() && !((pairs || quads) && nthr == 0)) continue;
        if ((v.pair() && v.group_form() != quads) || (quads && !v.pair())) continue;    // a three- / four-row plan takes the variants of its group length only, and vice versa
        if (v.lean() > lean) continue;                      // a lean variant needs a plan that qualifies for its form (2 implies 1)
        if (v.pipe != want_pipe || (int)v.nt() != want_nt) continue;
        if (tuning > 0) {
            if (v.vec != want_vec || v.depth != want_depth) continue;
        } else if (!v.production || (vec > 0 && v.vec != vec)) continue;
        // specialised forms (integer bins, single level) are cheaper than the general one
        const long cost = (long)v.nthr * 1000 + (long)v.kmax * 10 + v.stat - (v.tki() ? 400 : 0) - (v.sl() ? 5 : 0) - (v.hb() ? 300 : 0) - (v.ha() ? 50 : 0) - (v.pair() ? 5 : 0) - 3 * v.lean()
                          + ((depth_hint > 0 && v.depth != depth_hint) ? 1 : 0);      // among equals, the burst depth that measured best for the shape
        if (!best || cost < best_cost) { best = &v; best_cost = cost; }
    }
    return best;
}

// the cheapest packed kernel with `vec` cells per lane that covers the plan (null: the menu has none at that width)
inline const Variant* find_packed_variant(int vec, int stat, int nthr, int K) {
    const Variant* best = nullptr;
    long best_cost = 0;
    int n = 0;
    const Variant* tab = packed_variants_table(&n);
    for (int i = 0; i < n; ++i) {
        const Variant& v = tab[i];
        if (v.vec != vec || v.stat < stat || v.nthr < nthr || v.kmax < K) continue;
        const long cost = (long)v.nthr * 1000 + (long)v.kmax * 10 + v.stat;
        if (!best || cost < best_cost) { best = &v; best_cost = cost; }
    }
    return best;
}

// the packed LDS-histogram kernel with `vec` cells per lane for a partition plan (null: the menu has none at that width).  The form is
// matched exactly — the single-level form for single-level plans, arithmetic edges when the plan's edges are exact, else the edge table:
// the menu holds every form at one cell per lane, and a wider kernel of ANOTHER form is no substitute (the widths were measured per form).
// `arms`: the kernels outside the production menu too (a forced width: AFHIP_PACKED_HIST_VEC)
inline const Variant* find_packed_hist_variant(int vec, int stat, int nthr, int K, bool single_level, bool arith, bool arms = false) {
    const Variant* best = nullptr;
    long best_cost = 0;
    int n = 0;
    const Variant* tab = packed_hist_variants_table(&n);
    for (int i = 0; i < n; ++i) {
        const Variant& v = tab[i];
        if (!v.hb() || v.vec != vec || v.stat < stat || v.nthr < nthr || v.kmax < K || (!v.production && !arms)) continue;
        if (v.sl() != single_level || v.ha() != arith) continue;
        const long cost = (long)v.nthr * 1000 + (long)v.kmax * 10 + v.stat;
        if (!best || cost < best_cost) { best = &v; best_cost = cost; }
    }
    return best;
}

// the end-bin histogram kernel of storage `dtype` (AFHIP_I16 for either packed dtype) with `vec` cells per lane; the form is matched exactly,
// as in find_packed_hist_variant (null: the menu has none)
inline const Variant* find_end_bins_variant(int dtype, int vec, int stat, int nthr, int K, bool single_level, bool arith) {
    const Variant* best = nullptr;
    long best_cost = 0;
    int n = 0;
    const Variant* tab = end_bins_variants_table(&n);
    for (int i = 0; i < n; ++i) {
        const Variant& v = tab[i];
        if (!v.hb() || !feat_has(v.feat, FEAT_END_BINS) || v.dtype != dtype || v.vec != vec || v.stat < stat || v.nthr < nthr || v.kmax < K || !v.production) continue;
        if (v.sl() != single_level || v.ha() != arith) continue;
        const long cost = (long)v.nthr * 1000 + (long)v.kmax * 10 + v.stat;
        if (!best || cost < best_cost) { best = &v; best_cost = cost; }
    }
    return best;
}

}  // namespace afhip
