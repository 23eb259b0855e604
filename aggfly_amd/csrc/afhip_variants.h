// afhip_variants.h — the menus of compiled k_fused_temporal specialisations.
//
// The hot per-element loop must be straight-line code with every accumulator in a
// register, so the accumulator counts are template parameters.  gen_variants.py writes
// one translation unit per group of instantiations (compiled in parallel) plus ONE table
// (variants_table.hip) with a slice per menu: menu_table() hands out a slice, find_variant()
// picks the cheapest float instantiation that covers a lowered plan, find_exact_form() the
// kernel of one of the other menus.
#pragma once
#include <stdint.h>
#include "afhip_plan_types.h"

namespace afhip {

struct Variant {
    int dtype;    // AFHIP_F32 / AFHIP_F64; AFHIP_I16 for packed storage
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

// The kernel menus (gen_variants.py: TABLE_MENUS, same names and order; the generated table asserts it).
//   MENU_FLOAT        float32 / float64 cubes: every form (gen_variants.py: menu), searched by find_variant
//   MENU_PACKED       int16- and uint16-packed cubes (AFHIP_I16, AFHIP_U16: one set of AFHIP_I16 kernels, the signedness is in the unpack
//                     record; packed_menu): general two-level forms on the direct-load path only, all production
//   MENU_PACKED_HIST  ... and their LDS-histogram forms (packed_hist_menu): integer-bin forms for plans whose threshold slots are a
//                     contiguous equal-width partition; the kernels outside production are tuning arms
//   MENU_END_BINS     the LDS-histogram forms with FEAT_END_BINS, for partitions with a wide end bin on one side or both — float32,
//                     float64 and packed storage together (end_bins_menu), all production
//   MENU_CELL_MAP     the edge-table forms of MENU_END_BINS with FEAT_CELL_MAP, for partitions whose interior widths differ
//                     (cell_map_menu), all production
//   MENU_PACKED_SHORT the lean short-group forms of packed cubes (gen_variants.py: MORE_MENUS, packed_short_menu): two-, three-, four-row
//                     and mixed inner groups, the float32 lean menu's shapes at two cells and at one cell per lane, most of them at four as well, all production
//   MENU_PACKED_RF    the region-fused twins (FEAT_REGION_FUSED) of MENU_PACKED's and MENU_PACKED_SHORT's kernels at two cells and at one cell
//                     per lane (gen_variants.py: LATER_MENUS, packed_rf_menu), all production; searched by twin_of (afhip_planner.cpp)
// MENU_PACKED ... MENU_PACKED_SHORT are searched by find_exact_form.
enum Menu { MENU_FLOAT, MENU_PACKED, MENU_PACKED_HIST, MENU_END_BINS, MENU_CELL_MAP, MENU_PACKED_SHORT, MENU_PACKED_RF, MENU_COUNT };
const Variant* menu_table(Menu menu, int* n);   // generated (variants_table.hip): the menu's kernels, in gen_variants.py's order
const char* menu_key(Menu menu);                // generated: the menu's key in gen_variants.py's TABLE_MENUS ("float", "packed", ... "packed_rf")
const char* variants_menu();                    // "full" (the production menu), "arms" (+ the tuning arms) or "dev"

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
    const Variant* tab = menu_table(MENU_FLOAT, &n);
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

// The cheapest kernel of `menu` of storage `dtype` (AFHIP_I16 for either packed dtype) with `vec` cells per lane that covers the plan's
// stat / slots / columns (null: the menu has none at that width).  The form — single level, arithmetic edges — is matched exactly: the
// single-level form for single-level plans only, arithmetic edges when the plan's edges are exact, else the edge table.  The histogram
// menus hold every form at one cell per lane, and a wider kernel of ANOTHER form is no substitute (the widths were measured per form);
// MENU_PACKED holds the form (false, false) only.  What else a kernel has compiled in (LDS histogram, end bins) follows from the menu it
// stands in.  `arms`: the kernels outside the production menu too (a forced width: AFHIP_PACKED_HIST_VEC).  Among equally cheap
// kernels the first in table order.
//   `group_form` >= 0 asks for a short-group form (MENU_PACKED_SHORT) of that Variant::group_form — 0: two-row groups — and is matched
// exactly too; `lean` is the lean group end the plan qualifies for (VariantQuery::lean): a kernel may ask for less, and the leanest that
// fits is the cheapest.  -1: no short-group form, which is all the other menus hold.
inline const Variant* find_exact_form(Menu menu, int dtype, int vec, int stat, int nthr, int K, bool single_level, bool arith, bool arms = false,
                                      int group_form = -1, int lean = 0) {
    const Variant* best = nullptr;
    long best_cost = 0;
    int n = 0;
    const Variant* tab = menu_table(menu, &n);
    for (int i = 0; i < n; ++i) {
        const Variant& v = tab[i];
        if (v.dtype != dtype || v.vec != vec || v.stat < stat || v.nthr < nthr || v.kmax < K || (!v.production && !arms)) continue;
        if (v.sl() != single_level || v.ha() != arith) continue;
        if (group_form < 0 ? v.pair() : (!v.pair() || v.group_form() != group_form || v.lean() > lean)) continue;
        const long cost = (long)v.nthr * 1000 + (long)v.kmax * 10 + v.stat - 3 * v.lean();
        if (!best || cost < best_cost) { best = &v; best_cost = cost; }
    }
    return best;
}

}  // namespace afhip
