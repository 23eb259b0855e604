// afhip_planner.cpp — plan building (afhip_planner.h).  Host code only: compiled as C++, no HIP header, no hip* call.
//
// build_plan turns the column list into
//   * one inner accumulator set (STAT mode) + deduplicated threshold slots evaluated on
//     raw data, + one ColOp per column (source, transform, outer reducer);
//   * a chunk table over time: chunks are ranges of whole inner groups; a chunk either
//     holds whole outer periods (each emits its final value) or is a piece of one long
//     period (it emits a partial that k_combine_slots merges in time order);
//   * the kernel variant (dtype, LDS-DMA or direct loads, STAT, slots, columns).
// One function per decision, in the order build_plan calls them; each takes what it reads as parameters and returns its
// result as a small value.
#include "afhip_planner.h"
#include "afhip_cell_map.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace afhip {

namespace {
thread_local std::string g_err;
}

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char* last_error() { return g_err.c_str(); }

// ---- knobs ----
PlanKnobs read_knobs() {
    auto set = [](const char* name) { return getenv(name) != nullptr; };
    PlanKnobs k;
    if (const char* e = getenv("AFHIP_FORCE_WG")) { int w = atoi(e); if (w == 64 || w == 128 || w == 256) k.force_wg = w; }
    if (const char* e = getenv("AFHIP_WGS_PER_CU")) k.wgs_per_cu = std::max(1, atoi(e));
    k.no_period_chunks = set("AFHIP_NO_PERIOD_CHUNKS");
    k.no_round_fill = set("AFHIP_NO_ROUND_FILL");
    k.no_pair_mode = set("AFHIP_NO_PAIR_MODE");
    k.no_quad_mode = set("AFHIP_NO_QUAD_MODE");
    k.no_ragged_mode = set("AFHIP_NO_RAGGED_MODE");
    k.no_region_fused = set("AFHIP_NO_REGION_FUSED");
    k.no_packed_rf = set("AFHIP_NO_PACKED_RF");
    k.no_packed_hist = set("AFHIP_NO_PACKED_HIST");
    if (const char* e = getenv("AFHIP_PACKED_HIST_VEC")) { const int v = atoi(e); if (v == 1 || v == 2) k.packed_hist_vec = v; }
    k.no_packed_short = set("AFHIP_NO_PACKED_SHORT");
    if (const char* e = getenv("AFHIP_PACKED_SHORT_VEC")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) k.packed_short_vec = v; }
    k.no_end_bins_hist = set("AFHIP_NO_END_BINS_HIST");
    k.no_cell_map_hist = set("AFHIP_NO_CELL_MAP_HIST");
    k.counts_spmm = !set("AFHIP_NO_COUNTS_SPMM");
    if (const char* e = getenv("AFHIP_COUNTS_SPMM_SUB")) k.counts_spmm_sub = atoi(e);
    if (const char* e = getenv("AFHIP_NO_SLOT_SPMM")) k.no_slot_spmm = atoi(e) != 0;
    if (const char* e = getenv("AFHIP_RF_LAYOUT")) k.rf_layout = (e[0] == 'r') ? 1 : 0;
    if (const char* e = getenv("AFHIP_SLOT_SPMM_ORDER")) k.slot_spmm_order = (e[0] == 'p') ? 1 : 0;
    if (const char* e = getenv("AFHIP_SLOT_SPMM_SUB")) { const int sb = atoi(e); if (sb == 8 || sb == 16 || sb == 32 || sb == 64) k.slot_spmm_sub = sb; }
    return k;
}

// ---- 1. column lowering ----
static int add_thr_slot(std::vector<ThrSlot>& thr, const double* a3, bool bins) {
    ThrSlot s{};
    s.t0 = a3[0]; s.t1 = a3[1];
    const bool base_is_t0 = (a3[2] == 0.0);                 // nb_kernels.py:167
    if (bins) { s.A = 0.0; s.B = 1.0; }
    else if (base_is_t0) { s.A = 1.0; s.B = -a3[0]; }
    else { s.A = -1.0; s.B = a3[1]; }
    // float thresholds equivalent to the double compares for float inputs
    s.t0f = (float)a3[0]; if ((double)s.t0f > a3[0]) s.t0f = std::nextafterf(s.t0f, -INFINITY);
    s.t1f = (float)a3[1]; if ((double)s.t1f < a3[1]) s.t1f = std::nextafterf(s.t1f, INFINITY);
    s.nan_poisons = bins ? 0 : 1;
    for (size_t i = 0; i < thr.size(); ++i)
        if (!memcmp(&thr[i], &s, sizeof s)) return (int)i;
    thr.push_back(s);
    return (int)thr.size() - 1;
}

static int lower_columns(PlanLayout* pl) {
    const int K = pl->desc.K;
    int stat = 0;
    pl->thr.clear(); pl->cols.clear();
    pl->has_sine = false;
    for (int j = 0; j < K; ++j) {
        const afhip_column& c = pl->columns[j];
        ColOp co{};
        co.rounding = c.rounding;
        switch (c.inner) {
            case AFHIP_MEAN: co.src = SRC_MEAN; stat = std::max(stat, 1); break;
            case AFHIP_SUM: co.src = SRC_SUM; stat = std::max(stat, 1); break;
            case AFHIP_MIN: co.src = SRC_MIN; stat = std::max(stat, 2); break;
            case AFHIP_MAX: co.src = SRC_MAX; stat = std::max(stat, 2); break;
            case AFHIP_NANMEAN: co.src = SRC_NANMEAN; stat = 3; break;
            case AFHIP_DD: co.src = SRC_THR; co.src_idx = add_thr_slot(pl->thr, c.inner_args, false); break;
            case AFHIP_BINS: co.src = SRC_THR; co.src_idx = add_thr_slot(pl->thr, c.inner_args, true); break;
            case AFHIP_SINE_DD:
                co.src = SRC_SINE; stat = std::max(stat, 2);
                co.s0 = c.inner_args[0]; co.s1 = c.inner_args[1];
                co.s0x2 = 2.0 * co.s0; co.s1x2 = 2.0 * co.s1;
                {   // the pair-mode window tests on float data compare in float: s rounded down / up (afhip_plan_types.h: ColOp)
                    auto dn = [](double t) { float f = (float)t; return (double)f > t ? std::nextafterf(f, -INFINITY) : f; };
                    auto up = [](double t) { float f = (float)t; return (double)f < t ? std::nextafterf(f, INFINITY) : f; };
                    co.s0dn = dn(co.s0); co.s0up = up(co.s0); co.s1dn = dn(co.s1); co.s1up = up(co.s1);
                }
                co.swidth = co.s1 - co.s0; co.swidth2 = 2.0 * co.swidth;
                pl->has_sine = true;
                if (c.inner_args[2] != 0.0 && c.inner_args[2] != 1.0)
                    return fail(AFHIP_E_INVALID, "column %d: sine_dd flag must be 0 or 1 (temporal.py:324)", j);
                co.skind = (int)c.inner_args[2];
                break;
            default: return fail(AFHIP_E_INVALID, "column %d: unknown inner reducer %d", j, c.inner);
        }
        switch (c.transform) {
            case AFHIP_TF_NONE: co.tf = TF_NONE; break;
            case AFHIP_TF_POW: {
                const double e = c.transform_arg;
                if (e == std::floor(e) && std::fabs(e) <= 64.0) { co.tf = TF_POWI; co.tf_iarg = (int)e; }
                else { co.tf = TF_POW; co.tf_arg = e; }
                break;
            }
            case AFHIP_TF_HINGE: co.tf = TF_HINGE; co.tf_arg = c.transform_arg; break;
            case AFHIP_TF_INTER: co.tf = TF_INTER; break;
            default: return fail(AFHIP_E_INVALID, "column %d: unknown transform %d", j, c.transform);
        }
        // pow() and `inter` are compiled into the all-purpose (STAT 3) variants only (FEAT_GENERAL_TF)
        if (co.tf == TF_POW || co.tf == TF_INTER) stat = 3;
        switch (c.outer) {
            case AFHIP_IDENTITY: co.outer = OUT_FIRST; break;
            case AFHIP_SUM: co.outer = OUT_SUM; break;
            case AFHIP_MEAN: co.outer = OUT_MEAN; break;
            case AFHIP_MIN: co.outer = OUT_MIN; break;
            case AFHIP_MAX: co.outer = OUT_MAX; break;
            case AFHIP_DD:
            case AFHIP_BINS:
                co.outer = c.outer == AFHIP_DD ? OUT_DD : OUT_BINS;
                co.o0 = c.outer_args[0]; co.o1 = c.outer_args[1];
                co.obase = (c.outer_args[2] == 0.0) ? c.outer_args[0] : c.outer_args[1];
                break;
            default:
                return fail(AFHIP_E_UNSUPPORTED, "column %d: outer reducer %d is not fused (use the staged path)", j, c.outer);
        }
        pl->cols.push_back(co);
    }
    if ((int)pl->thr.size() > MAX_THR) return fail(AFHIP_E_UNSUPPORTED, "more than %d threshold slots in one pass", MAX_THR);
    if (K > MAX_COLS) return fail(AFHIP_E_UNSUPPORTED, "more than %d columns in one pass", MAX_COLS);
    pl->stat = stat;
    pl->nthr = (int)pl->thr.size();
    pl->K = K;
    return AFHIP_OK;
}

// (rows of 4 GiB and more: the short-group and arithmetic-edge variants address a row by a 32-bit byte offset per lane)
// bytes of one stored element
static int elem_bytes(int dtype) { return dtype == AFHIP_F64 ? 8 : (is_packed_dtype(dtype) ? 2 : 4); }

static bool rows_fit_32bit(const afhip_plan_desc& d) {
    return (uint64_t)d.n_cells * (uint64_t)elem_bytes(d.dtype) < (1ull << 32);
}

// ---- 2. short-group form ----
struct GroupForm {
    int glen = 0;           // length class of the inner groups: 2 / 3 / 4 rows throughout, 5 = mixed one to four rows, 0 = none of these
    bool pairs = false;     // short-group mode (two-, three- or four-row groups)
    bool lean = false, lean_sine = false;      // the lean group end (FEAT_LEAN), its sine-only form (FEAT_LEAN_SINE)
    bool quad_len() const { return glen >= 3; }      // three / four / mixed rows: the lean form only, general sine closed forms
    int glcode() const { return glen == 5 ? 3 : (glen == 4 ? 1 : (glen == 3 ? 2 : 0)); }      // feat_group_form
};

// short inner groups: the direct path keeps DEPTH rows in flight only INSIDE a group, the LDS-DMA ring
// prefetches across group ends.  Measured (mean plan, 721x1440 / 1801x3600): 2-step groups f64 4.5 vs
// 6.0 TB/s, f32 3.5 vs 4.3; 4-step groups f32 4.4 vs 5.6, f64 equal; 8 steps and longer: equal.
// every inner group exactly two rows ((tmin, tmax) pairs) and min / max / sine columns: the pair-mode variants of the
// direct-load path keep DEPTH / 2 whole groups in flight, so they need no ring either
// ... and the same for groups of exactly four rows (6-hourly data), in the lean form only (FEAT_FOUR_ROW)
static int group_length_class(const PlanLayout& pl, const PlanKnobs& knobs) {
    const afhip_plan_desc* desc = &pl.desc;
    int glen = 0;
    if (desc->G1 > 0 && pl.nthr == 0 && (pl.stat == 1 || pl.stat == 2) && !knobs.no_pair_mode) {
        for (int L : {2, 3, 4}) {
            bool all = desc->T == (int64_t)L * desc->G1;
            for (int64_t g = 0; all && g < desc->G1; ++g) all = pl.ib[(size_t)g + 1] - pl.ib[(size_t)g] == L;
            if (all) glen = L;
        }
        // mixed lengths of one to four rows (a sub-daily series with missing steps): the four-row form with a length per group
        // (FEAT_MIXED); a series of single rows throughout is not a short-group plan
        if (glen == 0 && desc->T > desc->G1 && !knobs.no_ragged_mode) {
            bool all = true;
            for (int64_t g = 0; all && g < desc->G1; ++g) {
                const int64_t L = pl.ib[(size_t)g + 1] - pl.ib[(size_t)g];
                all = L >= 1 && L <= 4;
            }
            if (all) glen = 5;
        }
    }
    if (glen >= 3 && knobs.no_quad_mode) glen = 0;
    // (its loads address a row by a 32-bit byte offset per lane: rows of 4 GiB and more take the general path)
    if (!rows_fit_32bit(*desc)) glen = 0;
    return glen;
}

static GroupForm short_group_form(const PlanLayout& pl, const PlanKnobs& knobs) {
    const afhip_plan_desc* desc = &pl.desc;
    GroupForm f;
    f.glen = group_length_class(pl, knobs);
    f.pairs = f.glen >= 2;
    // pair plans whose columns are all  mean | sum | min | max | sine_dd -> (integer power) -> sum | mean  without float32 rounding
    // take the lean group end (FEAT_LEAN); when every column is a plain sine_dd, its tightest form (FEAT_LEAN_SINE).  A sine_dd
    // column there needs s0 < s1: its two max() terms are one clamp of width s1 - s0.
    f.lean = f.pairs; f.lean_sine = f.lean && pl.K <= 2 && !f.quad_len();
    for (const ColOp& c : pl.cols) {
        const bool sine_ok = c.src == SRC_SINE && c.s0 < c.s1 && std::isfinite(c.swidth);
        const bool src_ok = c.src == SRC_MEAN || c.src == SRC_SUM || c.src == SRC_MIN || c.src == SRC_MAX || sine_ok;
        f.lean = f.lean && src_ok && (c.tf == TF_NONE || (c.tf == TF_POWI && c.tf_iarg >= 1)) && c.rounding == 0 && (c.outer == OUT_SUM || c.outer == OUT_MEAN);
        f.lean_sine = f.lean_sine && sine_ok && c.tf == TF_NONE;
    }
    f.lean_sine = f.lean_sine && f.lean;
    // four-row groups exist in the lean form only, for as many columns as its variants hold
    // (packed storage: the form is asked of its own menu afterwards, and which light plans take it is that menu's rule — choose_packed_short_variant)
    const bool packed = is_packed_dtype(desc->dtype);
    if (f.quad_len()) {
        VariantQuery q;
        q.dtype = desc->dtype; q.stat = pl.stat; q.K = pl.K; q.lean = 1; q.quads = f.glcode();
        if (!(f.lean && (packed || find_variant(q)))) f.pairs = f.lean = false;
    }
    // mean / sum columns alone (no min, max or sine): the pair path exists in the lean form only, and a light plan (one or two
    // columns) streams faster through the LDS-DMA ring, whose prefetch runs across the two-row groups (5.99 vs 5.44 TB/s on
    // 1801 x 3600 f32); with more columns the lean group end wins (profiles/r03_pairs_mean_poly.txt)
    // (four-row groups: the lean form measured ahead of the ring at every column count, profiles/r03_quad_groups.txt)
    if (f.pairs && pl.stat == 1) {
        // (three-row groups on float32: one- and two-column plans stream faster through the ring, 4.59 / 4.94 against 4.93 / 5.04 ms on
        // 1801 x 3600; from three columns on, and on float64 at every count, the lean form is ahead: profiles/r04_three_row_groups.txt)
        // (mixed lengths likewise: 6.25 / 6.39 against 6.89 / 6.83 ms, float64 level; profiles/r04_mixed_short_groups.txt)
        const int min_k = f.quad_len() ? (((f.glen == 3 || f.glen == 5) && desc->dtype == AFHIP_F32) ? 3 : 1) : 3;
        if (!f.lean || (!packed && pl.K < min_k)) f.pairs = f.lean = f.lean_sine = false;
    }
    return f;
}

// a short-group form lives on the direct-load path (load_path takes the LDS-DMA ring only for plans that have none: this keeps the two in step)
static GroupForm on_load_path(GroupForm f, int pipe) {
    f.pairs = f.pairs && pipe == 0;
    f.lean = f.lean && f.pairs; f.lean_sine = f.lean_sine && f.pairs;
    return f;
}

// ---- 3. load path ----
struct LoadPath {
    int pipe = 0;      // 0 direct loads, 1 LDS-DMA ring
    int vec = 1;       // cells per lane
};

// variant: the load path that measured fastest for the dtype and grid size
// (profiles/r01_sweep_load_arms.txt), subject to row alignment.
static LoadPath load_path(const PlanLayout& pl, bool pairs) {
    const afhip_plan_desc* desc = &pl.desc;
    const int64_t C_ = desc->n_cells;
    LoadPath p;
    if (desc->dtype == AFHIP_F64) {
        // one cell per lane, direct loads — on small grids too: round 1 had the LDS-DMA ring ahead there (6.1 vs 5.4 TB/s on
        // 104x236), the re-sweep on round 2's kernel has it behind (5.99 vs 6.67 TB/s; profiles/r02_kbench_resweep.txt)
    } else {
        // two cells per lane, unless the plan carries many accumulators (register pressure):
        // one cell per lane measured 1.6x faster on the 13-bin plan (profiles/r01_kbench_c4_f32.json)
        if (C_ % 2 == 0 && pl.nthr < 4 && pl.K < 8) p.vec = 2;
        // ... and unless it is a light one (one or two mean / sum columns, no threshold slots): one cell per lane then keeps
        // more waves resident and measured 6.6 % faster on configs[0] at 215x1440 (6,534 -> 6,966 GB/s), level on the 104x236
        // window (profiles/r02_kbench_light_f32_plans.txt)
        if (pl.stat <= 1 && pl.nthr == 0 && pl.K <= 2) p.vec = 1;
    }
    // short inner groups that are no short-group plan: the LDS-DMA ring (see group_length_class)
    if (!pairs) {
        const double avg_group = desc->G1 > 0 ? (double)desc->T / (double)desc->G1 : 0.0;
        const int vec16 = desc->dtype == AFHIP_F64 ? 2 : 4;
        bool sine = false;                          // sine_dd on short windows is fp64-VALU-bound: direct loads measured 4 % faster
        for (const ColOp& c : pl.cols) sine = sine || c.src == SRC_SINE;
        if (!sine && avg_group > 0 && avg_group < (desc->dtype == AFHIP_F64 ? 4.0 : 8.0) && C_ % vec16 == 0) { p.pipe = 1; p.vec = vec16; }
    }
    return p;
}

// the tuning arm of the description, or 0 when the rows do not allow it
static int usable_tuning(const afhip_plan_desc& d) {
    int tuning = d.tuning;
    if (tuning > 0) {
        const int tvec = ((tuning % 10000) % 1000) / 100;
        if (tvec <= 0 || d.n_cells % tvec != 0) tuning = 0;          // a vector arm needs rows that are multiples of it
    }
    return tuning;
}

// ---- 4. histogram partition ----
// The float32 / float64 checks below are one template over the input type T: std::fma / std::floor on T are fmaf / floorf for
// float and fma / floor for double, the very operations the kernel executes on its input precision.
// arithmetic edges: E[g] = lo0 + g * w must come out EXACTLY, in the input precision and by the very fma the
// kernel executes, for every bin of the guarded partition; the clamp points must lie inside the guard bins
template <typename T>
static bool edges_exact(const HistPartition& h, int n, double e0) {
    const double w = h.hb_w, lo0 = h.hb_lo0, gl = h.hb_gl, gh = h.hb_gh;
    const T wt = (T)w, lo0t = (T)lo0, e0t = (T)e0, glt = (T)gl, ght = (T)gh;
    bool ex = (double)wt == w && (double)lo0t == lo0 && (double)e0t == e0 && lo0t + wt == e0t;
    for (int g = 0; ex && g <= n + 1; ++g) {
        const double lo_want = g == 0 ? lo0 : h.hb_edge[g - 1];
        const double hi_want = g == n + 1 ? h.hb_edge[n] + w : h.hb_edge[g];
        ex = (double)std::fma((T)g, wt, lo0t) == lo_want && (double)std::fma((T)g, wt, e0t) == hi_want;
    }
    return ex && (double)glt > lo0 && (double)glt < e0 && (double)ght > h.hb_edge[n] && (double)ght < h.hb_edge[n] + w;
}

// the one-sided guess (ha_update): the guess constant biased down by the smallest delta of a ladder for which, with the
// kernel's own fma in the input precision, every edge E[k] of the guarded partition guesses bin k - 1 and the clamp
// points guess their guard bins.  fma and floor are monotone in v, so every value of [E[t], E[t+1]) then guesses t - 1
// or t.  No delta fits (bins of a few ulps): the table form.
template <typename T>
static bool biased_guess(const HistPartition& h, int n, int k_first, double* c0b) {
    const double c1 = h.hb_c1, c0 = h.hb_c0;
    bool found = false;
    for (int k = k_first; !found && k >= 8; --k) {
        const double delta = std::ldexp(1.0, -k);
        const T c1t = (T)c1, cbt = (T)(c0 - delta);
        auto guess = [&](double v) { return (double)std::floor(std::fma((T)v, c1t, cbt)); };
        bool okd = true;
        for (int g = 1; okd && g <= n + 1; ++g) okd = guess(h.hb_edge[g - 1]) == (double)(g - 1);
        okd = okd && guess(h.hb_gl) == 0.0 && guess(h.hb_gh) == (double)(n + 1);
        if (okd) *c0b = (double)cbt;
        found = okd;
    }
    return found;
}

// Bins of UNEQUAL interior widths (afhip_cell_map.h): `m` contiguous sorted bins, six at least, all of positive width.  Bin 0 and bin
// m - 1 are END bins exactly as FEAT_END_BINS has them — any positive width, infinite included, counted on the guard bins under the
// test  L < v < U  — and the m - 2 interior bins are described by the hb_* fields as ever; only the guess differs: hb_c1 / hb_c0 guess a
// cell of hb_cells cells of half the smallest interior width, and hb_cmap sends the cell to its bin.  Found only if the map fits a byte
// index (254 cells: range over smallest width up to 127), the cells are wide enough for a guess in the input precision, and the host
// check with the kernel's own fma passes.  (Five bins stay on the per-slot kernels, which do about as much work per value there.)
template <typename Slot>
static HistPartition find_cell_map(const PlanLayout& pl, int m, const std::vector<int>& order, Slot slot) {
    HistPartition h;
    if (m < 6 || !rows_fit_32bit(pl.desc)) return h;
    for (int b = 0; b < m; ++b)
        if (!(slot(b).t1 > slot(b).t0)) return h;             // (NaN limits fail)
    const int n = m - 2;
    double E[MAX_THR + 1];
    for (int k = 0; k < n; ++k) E[k] = slot(1 + k).t0;
    E[n] = slot(n).t1;
    CellMap cm;
    // (a packed cube's values are float32)
    const bool found = pl.desc.dtype != AFHIP_F64 ? cell_map_find<float>(E, n, &cm) : cell_map_find<double>(E, n, &cm);
    if (!found) return h;
    h.hb_n = n; h.hb_c1 = cm.c1; h.hb_c0 = cm.c0;
    for (int b = 0; b < m; ++b) h.hb_bin_of_slot[order[(size_t)b]] = b - 1;      // (the lower end: -1, the upper end: n)
    for (int k = 0; k <= n; ++k) h.hb_edge[k] = E[k];
    h.hb_wide = true;
    h.hb_slot_lo = order[0]; h.hb_slot_hi = order[(size_t)m - 1];
    h.hb_cells = cm.cells;
    memcpy(h.hb_cmap, cm.map, sizeof h.hb_cmap);
    return h;
}

// contiguous equal-width partition?  (sorted by t0, t1[b] == t0[b+1], constant width) — closed, or with a WIDE END BIN on one side or
// both: bin 0 and / or bin m - 1 of any positive width, infinite included (a catch-all below / above the equal-width bins).  The
// interior bins 1 .. m - 2 (at least two) always belong to the equal-width lattice; an end bin that continues it is an ordinary bin,
// one that does not is a wide end (its width may be smaller than the lattice's too).  The candidates are tried closed form first, so a
// partition without a wide end gets exactly the result it always got.  With a wide end hb_n and every constant describe the lattice
// alone; the end slots sit on the guard bins (HistPartition::hb_wide).  A contiguous partition that none of the four candidates fits —
// interior widths that differ — is handed to find_cell_map last, so no partition found here is ever found there.
static HistPartition find_partition(const PlanLayout& pl, bool all_bins) {
    const afhip_plan_desc* desc = &pl.desc;
    HistPartition h;
    if (!(all_bins && pl.nthr >= 4)) return h;
    const int m = pl.nthr;
    std::vector<int> order((size_t)m);
    for (int i = 0; i < m; ++i) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return pl.thr[(size_t)x].t0 < pl.thr[(size_t)y].t0; });
    auto slot = [&](int b) -> const ThrSlot& { return pl.thr[(size_t)order[(size_t)b]]; };
    bool contiguous = true;
    for (int b = 0; contiguous && b + 1 < m; ++b) contiguous = slot(b).t1 == slot(b + 1).t0;
    if (!contiguous) return h;
    // the lattice: bins first .. first + n - 1 of the sorted slots
    int first = 0, n = 0;
    double e0 = 0, w = 0;
    bool ok = false;
    for (int cand = 0; !ok && cand < 4; ++cand) {
        const int lo_wide = cand & 1, hi_wide = cand >> 1;
        first = lo_wide; n = m - lo_wide - hi_wide;
        if (n < 2 || (cand && m < 4)) continue;
        e0 = slot(first).t0;
        w = slot(first).t1 - e0;
        ok = w > 0 && std::isfinite(e0) && std::isfinite(w);
        for (int b = 0; ok && b < n; ++b) {
            const ThrSlot& t = slot(first + b);
            ok = std::fabs(t.t0 - (e0 + b * w)) <= 1e-9 * w && std::fabs(t.t1 - (e0 + (b + 1) * w)) <= 1e-9 * w;
        }
        // a wide end has a positive width of its own (NaN limits fail)
        if (ok && lo_wide) ok = slot(0).t1 > slot(0).t0;
        if (ok && hi_wide) ok = slot(m - 1).t1 > slot(m - 1).t0;
    }
    // the in-kernel guess floor(v / w - e0 / w) is computed in the INPUT precision and may be off by
    // one bin at most: the bins must not be narrower than ~2^20 (f32) / 2^48 (f64) ulps of the edges
    const double emax = std::max(std::fabs(e0), std::fabs(e0 + n * w));
    // (a packed cube's values are float32: its dtype goes the float way here and below)
    const double eps = desc->dtype != AFHIP_F64 ? 1.2e-7 : 2.3e-16;
    ok = ok && emax * eps * 16.0 < w;
    if (!ok) return find_cell_map(pl, m, order, slot);
    h.hb_n = n; h.hb_c1 = 1.0 / w; h.hb_c0 = 1.0 - e0 / w;      // + 1: bin 0 is the lower guard bin
    for (int b = 0; b < m; ++b) h.hb_bin_of_slot[order[(size_t)b]] = b - first;      // (a wide lower end: -1, a wide upper end: n)
    for (int b = 0; b < n; ++b) h.hb_edge[b] = slot(first + b).t0;
    h.hb_edge[n] = slot(first + n - 1).t1;
    h.hb_wide = n < m;
    h.hb_slot_lo = order[0]; h.hb_slot_hi = order[(size_t)m - 1];
    h.hb_w = w; h.hb_lo0 = e0 - w; h.hb_gl = e0 - 0.5 * w; h.hb_gh = h.hb_edge[n] + 0.5 * w;
    const bool f32 = desc->dtype != AFHIP_F64;
    bool ex = f32 ? edges_exact<float>(h, n, e0) : edges_exact<double>(h, n, e0);
    if (ex) ex = f32 ? biased_guess<float>(h, n, 22, &h.hb_c0b) : biased_guess<double>(h, n, 50, &h.hb_c0b);
    // (these variants address a row by a 32-bit byte offset per lane)
    if (!rows_fit_32bit(*desc)) ex = false;
    h.hb_arith = ex;
    return h;
}

// ---- 5. variant choice ----
// the variant with the region-fused period ends compiled in and every other field equal (null: the menu has none).  Float kernels have
// their twins in their own menu, at their own rows in flight; packed kernels (MENU_PACKED, MENU_PACKED_SHORT) in MENU_PACKED_RF, where a
// twin may keep FEWER rows in flight than its plain kernel (gen_variants.py: PACKED_RF_SHALLOW) — every field but `depth` is matched.
// Nothing the planner or the launch derives from the plain variant depends on that field on the direct-load path, the only one packed
// cubes have: the LDS layout (lds_sine_offset) reads the depth of the LDS-DMA ring only, and the chunk table is laid in whole inner groups,
// not in bursts.  (The round fill of build_chunks asks the PLAIN kernel how many workgroups a CU holds, on every storage.)
static const Variant* twin_of(const Variant* v) {
    const bool packed = v->dtype == AFHIP_I16;
    int n = 0;
    const Variant* tab = menu_table(packed ? MENU_PACKED_RF : MENU_FLOAT, &n);
    for (int i = 0; i < n; ++i) {
        const Variant& t = tab[i];
        if (t.feat == (v->feat | FEAT_REGION_FUSED) && t.dtype == v->dtype && t.pipe == v->pipe && t.vec == v->vec && t.stat == v->stat && t.nthr == v->nthr &&
            t.kmax == v->kmax && (packed || t.depth == v->depth))
            return &t;
    }
    return nullptr;
}

// Region-fused period ends: per-cell period values that would be a noticeable share of the traffic — P K 8 bytes per cell against T elem —
// by the thresholds of rf_plan_ok (section 7, which says where they come from), for a plan that runs variant `v`.
static double rf_share(const PlanLayout& pl) {
    return (double)pl.desc.P * pl.K * 8.0 / std::max(1.0, (double)pl.desc.T * (double)elem_bytes(pl.desc.dtype));
}
static bool rf_share_ok(const PlanLayout& pl, const Variant* v) {
    const bool two_row_light = v->pair() && !v->group_form() && !(v->lean() == 1 && v->kmax == 6);
    if (!two_row_light) return rf_share(pl) >= 0.002;
    return rf_share(pl) >= (is_packed_dtype(pl.desc.dtype) ? 0.10 : 0.05);
}

// Packed cubes: what can be known BEFORE chunking of whether a plan that would run `v` takes the region-fused route — everything
// rf_plan_ok asks but the one-slot-per-period test: a twin in the library, several periods, no table-order promise, no float32 rounding of
// the final value, the share of the period values, and neither AFHIP_NO_REGION_FUSED nor AFHIP_NO_PACKED_RF.  (Up to six columns and four
// threshold slots: MENU_PACKED_RF holds no other twin.)
//   `gives_up_four`: the rows are a multiple of four and the library holds the plan's kernel at four cells per lane, which has no twin — taking
// `v` costs the plan that kernel.  The four-cell kernel is ahead over the whole stream (x0.63 ... x0.96 on the short-group forms,
// profiles/packed_short_groups.txt) and the twin saves at the period ends alone, so such a plan is a candidate
//   - from PACKED_RF_NARROW_MIN_P periods on (below eight build_chunks lays no chunk per period either; the float32 twins gain 3 - 6 % at twelve),
//   - and a short-group plan only with period values of a quarter of the cube's bytes and more: on the configs[1] shape (rows a multiple of
//     four: the two-cell twin against the four-cell kernel on the per-cell route, profiles/packed_region_fused.txt, section 2) the 6-hourly
//     monthly polynomial (share 0.13) is BEHIND at x1.01 — and ahead at x0.94 / x0.95 where both routes run two cells or one —, weekly sine_dd
//     from pairs (0.29) ahead at x0.94, daily 8-hourly and mixed-length panels (5.3) at x0.37.  The general forms are ahead at every share
//     measured (monthly polynomial, 0.024: x0.91 ... x0.94; weekly x0.88 ... x0.90; daily degree days x0.90 ... x0.92; the daily K = 5 panel x0.77).
constexpr int64_t PACKED_RF_NARROW_MIN_P = 8;
static bool packed_rf_candidate(const PlanLayout& pl, const PlanKnobs& knobs, const Variant* v, bool gives_up_four) {
    if (!v || knobs.no_region_fused || knobs.no_packed_rf || pl.desc.exact_order || pl.desc.P < 2 || pl.K > 6 || pl.nthr > 4) return false;
    for (const ColOp& c : pl.cols)
        if (c.rounding & AFHIP_ROUND_FINAL) return false;
    if (gives_up_four && (pl.desc.P < PACKED_RF_NARROW_MIN_P || (v->pair() && rf_share(pl) < 0.25))) return false;
    return twin_of(v) != nullptr && rf_share_ok(pl, v);
}

// int16- and uint16-packed cubes (AFHIP_I16, AFHIP_U16) have a menu of their own (MENU_PACKED) of general forms on the direct-load path: the
// widest row piece per lane the rows allow and the menu holds for the plan's shape — four cells (8 bytes, the light shapes only), else
// two, else one.  (Four against two cells on the light shapes is the float32 rule "8 bytes per lane" carried over; not measured on
// packed cubes yet: profiles/packed_cube.txt.)
//   The four-cell forms have no region-fused twin (the period end's scan is written for one and two cells per lane).  A plan that is a
// candidate for that route (packed_rf_candidate) therefore takes the widest of two cells and one that divides the rows, where that
// kernel has a twin; where it has none (gen_variants.py: PACKED_RF_DROPPED) the choice is the one above.  The cost: a run of such a plan that
// wants the per-cell values (`want_cells`), or whose table has no runs that fit, goes through the two-cell plain kernel instead of the
// four-cell one.  AFHIP_NO_PACKED_RF restores the choice above, widths included.
// A plan whose rows allow four cells is a candidate under the further conditions of packed_rf_candidate (`gives_up_four`).
static const Variant* choose_packed_variant(const PlanLayout& pl, const PlanKnobs& knobs) {
    const int64_t C = pl.desc.n_cells;
    const bool gives_up_four = C % 4 == 0 && find_exact_form(MENU_PACKED, AFHIP_I16, 4, pl.stat, pl.nthr, pl.K, false, false) != nullptr;
    for (int vec : {2, 1}) {
        if (C % vec != 0) continue;
        const Variant* v = find_exact_form(MENU_PACKED, AFHIP_I16, vec, pl.stat, pl.nthr, pl.K, false, false);
        if (v && packed_rf_candidate(pl, knobs, v, gives_up_four)) return v;
        if (v) break;          // (the widest of the two the rows allow and the menu holds: no narrower kernel for the sake of a twin)
    }
    for (int vec : {4, 2, 1}) {
        if (C % vec != 0) continue;
        if (const Variant* v = find_exact_form(MENU_PACKED, AFHIP_I16, vec, pl.stat, pl.nthr, pl.K, false, false)) return v;
    }
    return nullptr;
}

// ... and a menu of lean short-group forms (MENU_PACKED_SHORT) for plans whose inner groups are all two, three or four rows or mixed one to
// four: short_group_form's rules — no threshold slot, stat 1 or 2, rows under 4 GiB at two bytes an element, every column lean
// (mean | sum | min | max | sine_dd -> integer power -> sum | mean) — and the exact form of the plan's group length, sine-only where
// every column is a plain sine_dd; the widest of four, two and one cells per lane that divides the rows and that the production menu holds
// (the stat-2 six-column forms exist at two and one only).  Null — not such a plan, no such kernel (`dev` menu), or AFHIP_NO_PACKED_SHORT (the
// A/B knob of scripts/packed_short_bench.py) — leaves the plan to the general packed kernel.  AFHIP_PACKED_SHORT_VEC=1|2|4 asks for that
// width where the library holds it (the width arms of the same script).
//   Which plans take the form by default was measured, by the rule the histogram routes were held to: on the configs[1] shape held as int16, a
// class of plans (group length x one mean column / the K = 5 polynomial / min and max / four stat-2 columns / two sine_dd columns) takes it only
// if the median of its widest production width lies below the general packed kernel's minimum in the same process, the routes alternating.
// Every class does (profiles/packed_short_groups.txt, section 2: the script's whole output): two-row groups x0.42 / x0.34 / x0.41 / x0.43 and
// x0.46 for sine_dd, three-row x0.61 / x0.45 / x0.51 / x0.49, four-row x0.61 / x0.41 / x0.53 / x0.53, mixed x0.70 / x0.48 / x0.63 / x0.62 — so
// LIGHT plans take it too: packed storage has no LDS-DMA ring, and the float rule that sends light stat-1 plans there (short_group_form: min_k)
// has no packed counterpart.  The same holds on rows that take two cells per lane on both routes (x0.38 ... x0.69) and one (x0.35 ... x0.76:
// section 3).  Widths by the same rule, form by form: four cells against two x0.63 ... x0.96, two against one x0.53 ... x0.82 — all production.
static const Variant* choose_packed_short_variant(const PlanLayout& pl, const PlanKnobs& knobs) {
    if (knobs.no_packed_short) return nullptr;
    const GroupForm f = short_group_form(pl, knobs);
    if (!f.pairs || !f.lean) return nullptr;
    auto find = [&](int vec, bool arms) {
        return pl.desc.n_cells % vec == 0
                   ? find_exact_form(MENU_PACKED_SHORT, AFHIP_I16, vec, pl.stat, pl.nthr, pl.K, false, false, arms, f.glcode(), f.lean_sine ? 2 : 1)
                   : nullptr;
    };
    if (knobs.packed_short_vec)
        if (const Variant* v = find(knobs.packed_short_vec, true)) return v;
    // (a candidate for the region-fused route: two cells or one, as in choose_packed_variant and at the same cost — four cells against two
    // measured x0.63 ... x0.96 on the per-cell route, profiles/packed_short_groups.txt)
    const bool gives_up_four = find(4, false) != nullptr;
    for (int vec : {2, 1})
        if (const Variant* v = find(vec, false)) {
            if (packed_rf_candidate(pl, knobs, v, gives_up_four)) return v;
            break;
        }
    for (int vec : {4, 2, 1})
        if (const Variant* v = find(vec, false)) return v;
    return nullptr;
}

// one inner group per period and every outer `first`: the plan qualifies for the single-level (`sl`) forms
static bool is_single_level(const PlanLayout& pl) {
    const afhip_plan_desc* desc = &pl.desc;
    bool single_level = desc->P == desc->G1;
    for (int64_t p = 0; single_level && p <= desc->P; ++p) single_level = pl.ob[(size_t)p] == p;
    for (const ColOp& c : pl.cols) single_level = single_level && c.outer == OUT_FIRST;
    return single_level;
}

// The LDS-histogram forms that are matched exactly (find_exact_form): those of packed cubes (MENU_PACKED_HIST) for a closed partition
// `hist` — found with the float32 rules: the values of a packed cube are float32 — the end-bin forms (MENU_END_BINS) for a partition
// with a wide end bin (HistPartition::hb_wide) and the cell-map forms (MENU_CELL_MAP) for one whose interior widths differ, on packed and
// float cubes alike.  A closed partition on a float cube never comes here: it
// goes through choose_variant.  Either way the widest of two and one cells per lane that divides the row length and that the production
// menu holds for the plan's stat tier and storage — single-level form for single-level plans, arithmetic edges when the edges are exact,
// else the edge table.  Null: no such kernel, or the route is off.
//   Closed, packed: which widths the menu holds was measured form by form (gen_variants.py: packed_hist_menu; profiles/packed_cube.txt,
// section 6): two cells per lane for the single-level edge-table forms only.  Null sends the plan to the general form above, and so does
// AFHIP_NO_PACKED_HIST.  AFHIP_PACKED_HIST_VEC=1|2 asks for that width where the library holds it, arms included (the A/B knob of that
// section).
//   Wide: the storage's production histogram forms with FEAT_END_BINS (gen_variants.py: end_bins_menu) — one cell per lane, and for packed
// cubes two where the rows are even and the menu holds the form (the single-level edge-table forms, as in packed_hist_menu).  Null — no
// such kernel (`dev` menu), a tuning arm, or the route is off — routes the plan as if the partition had not been found.
// AFHIP_NO_END_BINS_HIST switches the route off (the A/B knob of scripts/end_bins_bench.py); packed cubes follow AFHIP_NO_PACKED_HIST too,
// but not AFHIP_PACKED_HIST_VEC.  The route is the default on every storage, by the rule the packed histogram forms were held to: on the
// configs[1] shape, thirteen 5-degree bins between two open ends, single level and two-level with a mean, its median lies below the
// earlier route's minimum in the same process — at x0.11 / x0.12 of it on packed cubes, x0.27 / x0.34 on float32, x0.52 / x0.36 on
// float64 (profiles/end_bins.txt, section 2: the whole output of scripts/end_bins_bench.py with device, build and min / median / max of
// the three routes).
//   Cell map (HistPartition::hb_cells: interior bins of unequal widths, found by find_cell_map): the edge-table end-bin forms with
// FEAT_CELL_MAP (gen_variants.py: cell_map_menu, MENU_CELL_MAP), the widest of two and one cells per lane as for the end-bin menu; never an
// arithmetic-edge form.  Null under the same conditions as the end-bin route, with AFHIP_NO_CELL_MAP_HIST as its A/B knob
// (scripts/cell_map_bench.py).  The default on every storage by the same rule — on the configs[1] shape, the eight-bin spec
// (-inf,-10] ... (35,inf) and a fourteen-bin spec of three interior widths, single level / two-level with a mean, its median lies below the
// earlier route's minimum in the same process, the two alternating: at x0.14 / x0.14 and x0.14 / x0.15 of it on packed cubes, x0.30 / x0.46 and
// x0.30 / x0.47 on float32, x0.51 / x0.45 and x0.51 / x0.42 on float64 — and six closed bins win as well (x0.14 / x0.13, x0.30 / x0.45,
// x0.51 / x0.46), so the floor of six bins (find_cell_map) holds on all three (profiles/cell_map_bins.txt, section 2: the script's whole output).
static const Variant* choose_hist_variant(const PlanLayout& pl, const HistPartition& hist, int tuning, const PlanKnobs& knobs) {
    const bool packed = is_packed_dtype(pl.desc.dtype);
    if (hist.hb_n == 0 || (packed && knobs.no_packed_hist)) return nullptr;
    if (hist.hb_cells ? (knobs.no_cell_map_hist || tuning != 0) : (hist.hb_wide ? (knobs.no_end_bins_hist || tuning != 0) : !packed)) return nullptr;
    const Menu menu = hist.hb_cells ? MENU_CELL_MAP : (hist.hb_wide ? MENU_END_BINS : MENU_PACKED_HIST);
    const int dtype = packed ? AFHIP_I16 : pl.desc.dtype;
    const bool sl = is_single_level(pl);
    auto find = [&](int vec, bool arms) {
        return pl.desc.n_cells % vec == 0 ? find_exact_form(menu, dtype, vec, pl.stat, pl.nthr, pl.K, sl, hist.hb_arith, arms) : nullptr;
    };
    if (!hist.hb_wide && knobs.packed_hist_vec)
        if (const Variant* v = find(knobs.packed_hist_vec, true)) return v;
    for (int vec : {2, 1})
        if (const Variant* v = find(vec, false)) return v;
    return nullptr;
}

// `form0` and `path0` are the short-group form and the load path the plan would take by the default rules.  Null: the menu holds
// no variant that covers the plan.
static const Variant* choose_variant(const PlanLayout& pl, const GroupForm& form0, const LoadPath& path0, const HistPartition& hist, bool all_bins,
                                     int tuning, const PlanKnobs& knobs, int cu_count) {
    const afhip_plan_desc* desc = &pl.desc;
    // specialisations the lowered plan qualifies for
    const bool single_level = is_single_level(pl);
    const LoadPath path = (hist.hb_n > 0 && tuning == 0) ? LoadPath{0, 1} : path0;   // the LDS histogram lives on the direct-load path
    const GroupForm form = on_load_path(form0, path.pipe);
    // rows in flight per lane on the direct-load path: f64 four, f32 eight — but four for f32 plans with two cells per lane on
    // grids large enough for 256-thread workgroups (the multi-column plans; see gen_variants.py)
    int depth_hint = desc->dtype == AFHIP_F64 ? 4 : 8;
    if (desc->dtype == AFHIP_F32 && path.pipe == 0 && path.vec == 2 && !form.pairs && hist.hb_n == 0 &&
        (desc->n_cells + (int64_t)WG * 2 - 1) / ((int64_t)WG * 2) >= (int64_t)cu_count)
        depth_hint = 4;
    VariantQuery q;
    q.dtype = desc->dtype; q.pipe = path.pipe; q.vec = path.vec; q.stat = pl.stat; q.nthr = pl.nthr; q.K = pl.K; q.tuning = tuning;
    q.all_bins = all_bins; q.single_level = single_level;
    q.partition = hist.hb_n > 0 && path.pipe == 0;
    q.arith = q.partition && hist.hb_arith;
    q.quads = (form.pairs && form.quad_len()) ? form.glcode() : 0;
    q.pairs = form.pairs && !form.quad_len();
    if (q.quads) depth_hint = form.glen == 3 ? 6 : 8;           // two groups per block
    q.depth_hint = depth_hint;
    q.lean = form.lean ? (form.lean_sine ? 2 : 1) : 0;
    const Variant* v = find_variant(q);
    VariantQuery untuned = q;
    untuned.tuning = 0;
    if (!v && tuning > 0) v = find_variant(untuned);   // a tuning arm is a hint: arms are compiled for the headline plan shapes only
    if (!v) {      // direct loads, one cell per lane
        VariantQuery d = untuned;
        d.pipe = 0; d.vec = 1; d.partition = hist.hb_n > 0; d.arith = hist.hb_n > 0 && hist.hb_arith;
        v = find_variant(d);
    }
    if (!v) return nullptr;
    // A single-level plan takes an `sl` variant when the menu has one (no outer accumulators: cheaper) — but those have no region-fused
    // twin, and a plan that stores one value per group, column and cell (a daily panel of several degree-day columns) then writes and
    // re-reads period values worth a sizeable share of the cube.  From 5 % on the general two-level variant (outer = first) with its twin
    // is taken instead; packed bin counts (16-byte records, gathered directly) stay where they are.
    if (v->sl() && !v->tki() && tuning == 0 && !desc->exact_order && !knobs.no_region_fused &&
        (double)desc->P * pl.K * 8.0 >= 0.05 * (double)desc->T * (double)elem_bytes(desc->dtype)) {
        VariantQuery two = untuned;
        two.all_bins = two.single_level = two.partition = two.arith = false;
        const Variant* v2 = find_variant(two);
        if (v2 && v2->pipe == 0 && !v2->tki() && !v2->hb() && twin_of(v2)) v = v2;
    }
    return v;
}

// ---- 6. chunking ----
size_t plan_lds_bytes(const PlanLayout* pl) {
    const Variant& v = *pl->variant;
    if (v.hb()) return lds_hist_bytes(pl->hb_n + 2, v.vec, pl->wg) + (feat_has(v.feat, FEAT_CELL_MAP) ? (size_t)CELL_MAP_BYTES : 0);      // (the cell map, behind the counters)
    return lds_sine_offset(v.pipe, pl->wg / 64, v.depth) + (pl->has_sine ? (size_t)feat_sine_bytes(v.feat) : 0);      // the variant's sine table, behind the ring
}

// Chunking.  target_len = time steps a workgroup should stream; a long period is cut on
// inner-group boundaries into pieces (each emits a partial), short consecutive periods are
// packed into one chunk (each emits its own final value).
static int lay_chunks(PlanLayout* pl, int64_t want_chunks);

static int build_chunks(PlanLayout* pl, int vec, const PlanKnobs& knobs, const DeviceFacts& dev) {
    const int64_t P = pl->desc.P, C = pl->desc.n_cells;
    // single-wave workgroups when 256-thread tiles cannot give every CU a few workgroups — and on large grids too, unless every
    // workgroup copies a sine table into LDS first (pair-mode sine_dd at 64 threads: 3.23 -> 5.80 ms).  The bare streaming read of
    // this access shape is fastest in single-wave workgroups (scripts/probe/read_bw.hip: 7.02 against 6.69 TB/s at four rows in
    // flight, profiles/r03_read_ceiling.txt) and the plans follow it by less: configs[1] f64 3.142 -> 3.131 ms, f32 1.713 -> 1.693,
    // C1 f32 1.577 -> 1.558, the reference's benchmark shape 5.336 -> 5.281 (same box, arms alternated; 128 threads: 3.234).
    pl->wg = ((C + (int64_t)WG * vec - 1) / ((int64_t)WG * vec) < (int64_t)dev.cu_count || !pl->has_sine) ? 64 : WG;
    // the LDS-histogram kernel: single-wave workgroups and MANY time chunks.  It is short of bytes in flight (waves park 65 % of
    // their cycles on memory at 4.2 waves per SIMD, VALU and LDS far from busy: profiles/r03_c4_bound_pmc.txt), and the more,
    // smaller workgroups the grid offers the fuller the CUs stay: configs[3] f32 3.15 ms (7 chunks of 256 threads) -> 2.84 ms
    // (126 chunks of 64), f64 5.86 -> 5.58 (profiles/r03_sweep_chunks_depth.txt).  Round 1 had measured 4-wave workgroups
    // ahead — at the few chunks of that time.
    const bool hist = pl->variant && pl->variant->hb();
    if (hist) pl->wg = 64;
    if (knobs.force_wg) pl->wg = knobs.force_wg;   // experiment knob
    pl->tiles = (C + (int64_t)pl->wg * vec - 1) / ((int64_t)pl->wg * vec);
    // aim for ~4 workgroups per CU over the whole grid, never streaming fewer than 64 steps
    int per_cu = 4;      // measured (profiles/r01_sweep_chunks.txt, r03_sweep_chunks_depth.txt): the fewer time chunks the better once every CU has ~4 workgroups
    if (hist) per_cu = 96;   // ... except for the histogram kernel (above)
    if (knobs.wgs_per_cu) per_cu = knobs.wgs_per_cu;   // experiment knob
    const int64_t want_wgs = (int64_t)dev.cu_count * per_cu * (WG / pl->wg);
    int64_t want_chunks = std::max<int64_t>(1, (want_wgs + pl->tiles - 1) / pl->tiles);
    // Plans with several output periods: up to one time chunk per period.  Cutting ON period boundaries adds no slot and no traffic
    // (the "fewer chunks are better" of round 1 was measured at P = 1, where every cut adds a slot), and the period-end stores are
    // what such plans pay for: with the stores compiled out the configs[1] plan runs P = 12 and P = 73 exactly as fast as P = 1
    // (3.14 ms), with them 3.69 and 4.30 — 150 MB of stores for 0.55 ms, box-dependent (0.22 ms on another box).  The more chunks, the
    // fewer period ends a workgroup carries in the middle of its stream: P = 365 5.24 -> 4.94 ms, P = 73 3.76 -> 3.46, weekly f32
    // 1.72 -> 1.67, the reference's own benchmark shape 5.64 -> 5.53 (profiles/r03_period_end_stores.txt).  lay_chunks still
    // packs periods shorter than 64 steps together; the histogram kernel keeps its own rule.
    // Plans that already get eight chunks or more keep them (configs[2]'s shape, 14 chunks for 40 years: 40 measured 0.5 % behind).
    bool period_chunks = false;
    if (P > 1 && !hist && want_chunks < 8 && !knobs.wgs_per_cu && !knobs.no_period_chunks) {
        const int64_t wg_cap = 262144;                              // workgroups a period-chunked launch may have
        const int64_t by_period = std::min<int64_t>(P, std::max<int64_t>(1, wg_cap / std::max<int64_t>(pl->tiles, 1)));
        // (a handful of period chunks makes a handful of occupancy rounds with a costly last one: P = 4 measured 2-4 % behind one chunk)
        if (by_period >= 8) { want_chunks = by_period; period_chunks = true; }
    }
    int rc = lay_chunks(pl, want_chunks);
    if (rc) return rc;
    // Rounds.  A CU holds `resident` workgroups of this variant at once; a grid of more workgroups than the chip holds runs in
    // "rounds", and a last round that is mostly empty is paid in full: the reference's own benchmark shape (global 0.25 deg,
    // 2,028 tiles as ONE chunk against 1,536 resident workgroups = 1.32 rounds) ran at 0.65 of the HBM peak, as three chunks
    // (3.96 rounds) at 0.79 (profiles/r03_ref_shape_arms.txt).  When the grid does not fit the chip at once, take the chunk
    // count (of the next few) whose last round is fullest; a grid that fits keeps the fewest chunks, which measured best.
    // (period-aligned chunks are many and short: their last round weighs little, and the search below would cut periods to fill it)
    if (!period_chunks && !knobs.no_round_fill && !knobs.wgs_per_cu) {
        const int64_t capacity = (int64_t)dev.resident_wgs(pl->variant->fn, pl->wg, plan_lds_bytes(pl)) * dev.cu_count;
        auto fill = [&](int64_t total) { const int64_t rounds = (total + capacity - 1) / capacity; return (double)total / (double)(rounds * capacity); };
        int64_t total = pl->tiles * (int64_t)pl->chunks.size();
        if (capacity > 0 && total > capacity && fill(total) < 0.92) {
            int64_t best_c = want_chunks;
            double best = fill(total);
            size_t last_n = pl->chunks.size();
            for (int64_t c = want_chunks + 1; c <= want_chunks + 12 && best < 0.92; ++c) {
                if ((rc = lay_chunks(pl, c))) return rc;
                if (pl->chunks.size() == last_n) continue;         // (period boundaries: not every count exists)
                last_n = pl->chunks.size();
                const double f = fill(pl->tiles * (int64_t)pl->chunks.size());
                if (f > best + 1e-9) { best = f; best_c = c; }
            }
            if ((rc = lay_chunks(pl, best_c))) return rc;
        }
    }
    return AFHIP_OK;
}

// Chunk table for ~want_chunks time chunks (see build_chunks).
static int lay_chunks(PlanLayout* pl, int64_t want_chunks) {
    const auto& ib = pl->ib;
    const auto& ob = pl->ob;
    const int64_t G1 = pl->desc.G1, P = pl->desc.P, T = pl->desc.T;
    const int64_t target_len = std::max<int64_t>(64, T / std::max<int64_t>(want_chunks, 1));
    // splitting a period adds partial traffic (16 B per extra slot, column and cell, write +
    // read); keep it under ~5 % of the cube: extra_slots*K*16 <= 0.05*T*elem.  (2 % starved the
    // CONUS-window f32 plan of workgroups: 9 chunks 0.229 ms, 22 chunks 0.151 ms.)
    const int64_t elem = elem_bytes(pl->desc.dtype);
    const double split_frac = 0.05;
    int64_t split_budget = std::max<int64_t>(1, (int64_t)(split_frac * (double)T * (double)elem / (16.0 * std::max(1, pl->K))));
    const bool any_first = std::any_of(pl->cols.begin(), pl->cols.end(), [](const ColOp& c) { return c.outer == OUT_FIRST; });
    const bool may_split = !pl->desc.exact_order && !any_first;

    pl->chunks.clear();
    pl->emit.assign((size_t)std::max<int64_t>(G1, 1), 0);
    pl->slot_ptr.assign((size_t)P + 1, 0);
    int64_t slot = 0;

    auto steps_of = [&](int64_t p) { return ib[(size_t)ob[(size_t)p + 1]] - ib[(size_t)ob[(size_t)p]]; };
    auto groups_of = [&](int64_t p) { return ob[(size_t)p + 1] - ob[(size_t)p]; };
    auto splittable = [&](int64_t p) {
        return may_split && split_budget > 0 && groups_of(p) >= 2 && steps_of(p) >= 2 * target_len;
    };
    auto push_chunk = [&](int64_t g_lo, int64_t g_hi, int64_t slot_base) {
        ChunkDesc c{};
        c.k_lo = ib[(size_t)g_lo]; c.k_hi = ib[(size_t)g_hi];
        c.g_lo = (int32_t)g_lo; c.g_hi = (int32_t)g_hi; c.slot_base = (int32_t)slot_base;
        pl->chunks.push_back(c);
    };

    int64_t p = 0;
    while (p < P) {
        const int64_t g0 = ob[(size_t)p], g1 = ob[(size_t)p + 1];
        if (g1 == g0) {  // empty resample bin: no slot, the combine kernel writes NaN
            pl->slot_ptr[(size_t)p] = (int32_t)slot;
            ++p;
            continue;
        }
        if (splittable(p)) {
            const int64_t steps = steps_of(p);
            const int64_t pieces = std::max<int64_t>(2, std::min<int64_t>({steps / target_len, g1 - g0, split_budget + 1}));
            pl->slot_ptr[(size_t)p] = (int32_t)slot;
            int64_t g = g0, made = 0;
            for (int64_t i = 1; i <= pieces && g < g1; ++i) {
                int64_t ge;
                if (i == pieces) {
                    ge = g1;
                } else {
                    const int64_t k_goal = ib[(size_t)g0] + (steps * i) / pieces;
                    ge = (int64_t)(std::lower_bound(ib.begin() + g + 1, ib.begin() + g1, k_goal) - ib.begin());
                    ge = std::min(ge, g1);
                }
                if (ge <= g) continue;
                push_chunk(g, ge, slot);
                pl->emit[(size_t)ge - 1] = 1;
                ++slot; ++made;
                g = ge;
            }
            split_budget -= std::max<int64_t>(0, made - 1);
            ++p;
            continue;
        }
        // pack whole periods until the chunk holds ~target_len steps
        const int64_t cg0 = g0, slot_base = slot;
        int64_t acc_steps = 0, cg1 = g0;
        bool first = true;
        while (p < P) {
            const int64_t a0 = ob[(size_t)p], a1 = ob[(size_t)p + 1];
            const int64_t st = steps_of(p);
            if (!first && (acc_steps + st > target_len || splittable(p))) break;
            pl->slot_ptr[(size_t)p] = (int32_t)slot;
            if (a1 > a0) { pl->emit[(size_t)a1 - 1] = 1; ++slot; cg1 = a1; }
            acc_steps += st;
            first = false;
            ++p;
        }
        push_chunk(cg0, cg1, slot_base);
    }
    pl->slot_ptr[(size_t)P] = (int32_t)slot;
    pl->n_slots = slot;
    if (pl->chunks.size() > 65535)
        return fail(AFHIP_E_UNSUPPORTED, "plan needs %zu chunks (> 65535 grid.y)", pl->chunks.size());
    return AFHIP_OK;
}

// ---- 7. region-fused eligibility (after chunking: it reads the slots of the periods) ----
// Region-fused period ends (FusedArgs::rf_w): the twin variant, if the menu has one, and what the plan itself must satisfy —
// two-level columns without float32 rounding of the final value (the period value must enter the weighted sum as it leaves
// the accumulator; an outer mean's division by the period's group count is applied to the region sums, k_rf_reduce), at most one slot per period (shared validity needs the whole period's value), several periods
// (with one the stores sit at the kernel's end and cost nothing: the headline stays on the route it was measured on).
static bool rf_plan_ok(const PlanLayout& pl, const PlanKnobs& knobs) {
    const afhip_plan_desc* desc = &pl.desc;
    const Variant* v = pl.variant;
    bool ok = pl.variant_rf != nullptr && !desc->exact_order && desc->P >= 2 && !knobs.no_region_fused;
    if (is_packed_dtype(desc->dtype) && knobs.no_packed_rf) ok = false;      // (the A/B knob of scripts/packed_rf_bench.py)
    for (const ColOp& c : pl.cols) ok = ok && !(c.rounding & AFHIP_ROUND_FINAL);      // (identity outers too: a daily panel of daily means)
    for (int64_t p = 0; ok && p < desc->P; ++p) ok = pl.slot_ptr[(size_t)p + 1] - pl.slot_ptr[(size_t)p] <= 1;
    // ... and per-cell period values that would be a noticeable share of the traffic: P K 8 bytes per cell against T elem.  Below
    // ~0.2 % there is nothing to win and the emit still costs: configs[2]'s shape (40 annual values of 2 columns from 350,640
    // hourly steps: 0.05 %) measured 0.25 % behind, the one-period headline (0.06 %) 0.6 %; the shapes that gain sit at 0.5 % and up.
    // Which forms gain was measured, not derived (profiles/r03_region_fused.txt: an occupancy rule could not tell them apart): float64
    // forms and float32 forms without threshold slots gain 3 - 50 % from two periods on; the lean four-row forms and the six-column
    // lean pair form likewise (6-hourly monthly polynomial: step 0.97 against 1.13 - 1.33 ms).
    // Round 4 (the scan form of the period end; twins for threshold-only plans and every short-group form; profiles/r04_region_fused_scan.txt):
    // the float32-with-a-threshold-slot forms are level from 12 periods and ahead from there, a degree-day column alone gains 6 % at
    // 12 and 52 periods and 22-25 % on a daily panel — one rule for all of them: period values of 0.2 % of the cube and more.  The
    // two-row forms other than the six-column lean one (sine_dd from (tmin, tmax) pairs: a period end every few rows) pay only where
    // the per-cell route's own traffic decides: monthly 4.44 against 3.77 ms (behind), weekly 5.80 against 6.20, daily 17.7 against
    // 21.5 — from period values of 5 % of the cube.
    //   Packed cubes (profiles/packed_region_fused.txt, sections 2 and 3: scripts/packed_rf_bench.py on the configs[1] shape held as int16, the
    // twin's median against the per-cell route's minimum in one process, on rows that take two cells per lane on both routes / one): the
    // same rule holds at 0.2 % — monthly polynomial (share 0.024) x0.95 ... x0.99, weekly x0.89 ... x0.94, daily degree days x0.83 / x0.86, the
    // daily K = 5 panel x0.75 / x0.63, 6-hourly monthly polynomial x0.94 / x0.95, daily 8-hourly and mixed-length panels x0.37 ... x0.43.  The
    // light two-row forms: the same jobs are twice the share at two bytes an element, and the threshold doubles with them — sine_dd from pairs
    // monthly (0.067) is BEHIND at x1.05 / x1.04, weekly (0.29) ahead at x0.80 / x0.83, daily (2.0) at x0.48 / x0.50: from period values of 10 %
    // of the cube.
    if (ok) ok = rf_share_ok(pl, v);
    return ok;
}

// ---- 8. group table, packed-count format, workspace sizes ----
static std::vector<int64_t> group_table(const PlanLayout& pl) {
    const int64_t G1 = pl.desc.G1;
    std::vector<int64_t> gtab(2 * ((size_t)G1 + 2), 0);
    for (int64_t g = 0; g < G1; ++g) {
        const int64_t len = pl.ib[(size_t)g + 1] - pl.ib[(size_t)g];
        const double inv = len > 0 ? 1.0 / (double)len : 0.0;     // correctly rounded: div_by() then equals s / n exactly
        int64_t bits;
        memcpy(&bits, &inv, 8);
        gtab[2 * (size_t)g] = (pl.ib[(size_t)g + 1] << 1) | (pl.emit[(size_t)g] ? 1 : 0);
        gtab[2 * (size_t)g + 1] = bits;
    }
    return gtab;
}

// packed counts: integer-bin single-level variant, every column a plain bin count, no period longer than a
// 16-bit counter holds (0xFFFF is the NaN mark).  nw = 0: the plan is not packed.
static PackFmt packed_format(const PlanLayout& pl) {
    const int64_t K = pl.desc.K;
    PackFmt pk{};
    bool packed = pl.variant->tki() && pl.variant->sl() && K <= 16;
    for (const ColOp& c : pl.cols)
        packed = packed && c.src == SRC_THR && c.tf == TF_NONE && c.rounding == 0 && c.outer == OUT_FIRST;
    int64_t maxlen = 0;
    for (int64_t g = 0; g < pl.desc.G1; ++g) maxlen = std::max(maxlen, pl.ib[(size_t)g + 1] - pl.ib[(size_t)g]);
    packed = packed && maxlen < 65535;
    if (!packed) return pk;
    // the narrowest field that holds the longest period's count and keeps all ones free for NaN; 16-byte records when
    // K such fields fit two words (daily data, annual bins: 13 x 9 bits), else 16-bit fields in 32 bytes
    int bw = 1;
    while (((int64_t)1 << bw) - 1 <= maxlen) ++bw;
    int f = 64 / bw;
    pk.nw = 2;
    if (K > 2 * f) { bw = 16; f = 4; pk.nw = 4; }
    pk.mask = (uint32_t)(((uint64_t)1 << bw) - 1);
    for (int j = 0; j < MAX_COLS; ++j) { pk.word[j] = (uint8_t)(j / f); pk.shift[j] = (uint8_t)((j % f) * bw); }
    return pk;
}

static void workspace_sizes(PlanLayout* pl) {
    const int64_t C = pl->desc.n_cells, K = pl->desc.K, P = pl->desc.P;
    auto a256 = [](int64_t b) { return (b + 255) / 256 * 256; };
    pl->ws_partial = pl->packed ? a256(std::max<int64_t>(pl->n_slots, 1) * C * pl->pk.nw * 8)
                                : a256(std::max<int64_t>(pl->n_slots, 1) * K * C * 8);
    pl->ws_panel = a256(C * (K + 1) * std::max<int64_t>(P, 1) * 8);
}

// ---- the planner ----
static int validate_desc(const afhip_plan_desc* d) {
    if (!d) return fail(AFHIP_E_INVALID, "plan_create: desc is NULL");
    if (d->T < 0 || d->n_cells <= 0 || d->K <= 0 || d->G1 < 0 || d->P < 0)
        return fail(AFHIP_E_INVALID, "plan_create: bad sizes (T=%lld n_cells=%lld K=%d G1=%lld P=%lld)",
                    (long long)d->T, (long long)d->n_cells, d->K, (long long)d->G1, (long long)d->P);
    if (d->dtype != AFHIP_F32 && d->dtype != AFHIP_F64 && !is_packed_dtype(d->dtype))
        return fail(AFHIP_E_INVALID, "plan_create: dtype must be AFHIP_F32, AFHIP_F64, AFHIP_I16 or AFHIP_U16");
    if (!d->inner_bounds || !d->outer_bounds || !d->columns) return fail(AFHIP_E_INVALID, "plan_create: NULL table");
    if (d->inner_bounds[0] != 0 || d->inner_bounds[d->G1] != d->T)
        return fail(AFHIP_E_INVALID, "plan_create: inner_bounds must run from 0 to T");
    for (int64_t g = 0; g < d->G1; ++g)
        if (d->inner_bounds[g + 1] < d->inner_bounds[g]) return fail(AFHIP_E_INVALID, "plan_create: inner_bounds not monotone (time index must be monotonic increasing)");
    if (d->outer_bounds[0] != 0 || d->outer_bounds[d->P] != d->G1)
        return fail(AFHIP_E_INVALID, "plan_create: outer_bounds must run from 0 to G1");
    for (int64_t p = 0; p < d->P; ++p)
        if (d->outer_bounds[p + 1] < d->outer_bounds[p]) return fail(AFHIP_E_INVALID, "plan_create: outer_bounds not monotone");
    if (d->G1 > INT32_MAX - 2) return fail(AFHIP_E_INVALID, "plan_create: too many inner groups");
    return AFHIP_OK;
}

int build_plan(const afhip_plan_desc* desc, const DeviceFacts& dev, PlanLayout* pl) {
    int rc = validate_desc(desc);
    if (rc) return rc;
    const PlanKnobs knobs = read_knobs();
    static_cast<RunKnobs&>(*pl) = knobs;
    pl->desc = *desc;
    pl->ib.assign(desc->inner_bounds, desc->inner_bounds + desc->G1 + 1);
    pl->ob.assign(desc->outer_bounds, desc->outer_bounds + desc->P + 1);
    pl->columns.assign(desc->columns, desc->columns + desc->K);
    pl->desc.inner_bounds = nullptr; pl->desc.outer_bounds = nullptr; pl->desc.columns = nullptr;
    if ((rc = lower_columns(pl))) return rc;

    // int16 and uint16 storage alike (the kernels take the signedness from the bound packing).  Their menus hold no tuning arm that
    // `tuning` names; of the short-group forms the lean ones; region-fused twins at two cells and at one cell per lane (MENU_PACKED_RF).
    const bool packed = is_packed_dtype(desc->dtype);
    const int tuning = packed ? 0 : usable_tuning(pl->desc);
    bool all_bins = pl->nthr > 0;
    for (const ThrSlot& t : pl->thr) all_bins = all_bins && t.nan_poisons == 0;
    // A plan of four or more contiguous, equal-width, strict bins (on packed storage by the float32 rules) — or of six or more whose interior
    // widths differ (find_cell_map: hb_wide with a cell map) — takes an LDS-histogram form,
    // chunked with single-wave workgroups and many chunks and, single-level, with packed count records and the count gather
    // (packed_format).  A float cube's closed partition finds its form in choose_variant, which may also leave the partition unused;
    // packed cubes and partitions with a wide end bin have menus of exact forms: that form or none — no kernel without FEAT_END_BINS ever
    // sees a partition with a wide end, and the general packed kernels see none at all — so without one the plan routes as if the
    // partition had not been found.
    HistPartition hist = find_partition(*pl, all_bins);
    pl->variant = nullptr;
    if (packed || hist.hb_wide) {
        pl->variant = choose_hist_variant(*pl, hist, tuning, knobs);
        if (!pl->variant) hist = HistPartition{};
    }
    static_cast<HistPartition&>(*pl) = hist;
    if (!pl->variant && packed) {
        // the lean short-group forms, else the packed menu of general forms: no packed counts (packed_format finds no integer-bin
        // form); the spatial stage is the slot gather or the table-order sums
        pl->variant = choose_packed_short_variant(*pl, knobs);
        if (!pl->variant) pl->variant = choose_packed_variant(*pl, knobs);
    } else if (!pl->variant) {
        const GroupForm form = short_group_form(*pl, knobs);
        const LoadPath path = load_path(*pl, form.pairs);
        pl->variant = choose_variant(*pl, form, path, hist, all_bins, tuning, knobs, dev.cu_count);
    }
    if (!pl->variant)
        return packed ? fail(AFHIP_E_UNSUPPORTED, "no packed kernel variant for stat=%d slots=%d columns=%d", pl->stat, pl->nthr, pl->K)
                      : fail(AFHIP_E_UNSUPPORTED, "no kernel variant for dtype=%d stat=%d slots=%d columns=%d", desc->dtype, pl->stat, pl->nthr, pl->K);
    if ((rc = build_chunks(pl, pl->variant->vec, knobs, dev))) return rc;
    pl->variant_rf = twin_of(pl->variant);      // (null: the storage's menu of twins holds none for this kernel, and rf_plan_ok is false)
    pl->rf_plan_ok = rf_plan_ok(*pl, knobs);
    pl->gtab = group_table(*pl);
    pl->pk = packed_format(*pl);
    pl->packed = pl->pk.nw != 0;
    workspace_sizes(pl);
    return AFHIP_OK;
}

}  // namespace afhip
