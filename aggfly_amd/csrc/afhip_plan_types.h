// afhip_plan_types.h — what the host planner (afhip_planner.cpp) and the device code (afhip_kernels.h) share: launch constants,
// the column / slot / chunk records that FusedArgs copies by value, the feature bits of k_fused_temporal and its LDS layout.  Plain C++: no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace afhip {

constexpr int WG = 256;          // 4 wavefronts of 64
constexpr int MAX_THR = 16;      // threshold slots evaluated on raw data per pass
constexpr int MAX_COLS = 16;     // output columns per pass
constexpr int HB_TABLE_BYTES = 2 * (MAX_THR + 2) * 16;    // LDS edge tables of the histogram path (576 B)

// inner-source kinds (what a column reads at the end of an inner group)
enum : int { SRC_MEAN = 0, SRC_SUM = 1, SRC_MIN = 2, SRC_MAX = 3, SRC_NANMEAN = 4, SRC_THR = 5, SRC_SINE = 6 };
enum : int { TF_NONE = 0, TF_POWI = 1, TF_POW = 2, TF_HINGE = 3, TF_INTER = 4 };
enum : int { OUT_FIRST = 0, OUT_SUM = 1, OUT_MEAN = 2, OUT_MIN = 3, OUT_MAX = 4, OUT_DD = 5, OUT_BINS = 6 };

// One threshold slot on raw data: contribution = (t0 < v && v < t1) ? fma(A, v, B) : 0.
//   dd, base = t0:  inside the window v - t0 > 0, so |v - base| = fma(+1, v, -t0)
//   dd, base = t1:  inside the window v - t1 < 0, so |v - base| = fma(-1, v, +t1)
//   bins:           fma(0, v, 1) = 1
// One rounding, identical to the reference's av = v - base; if av < 0: av = -av
// (nb_kernels.py:169-177) and c += 1.0 (nb_kernels.py:190-196).
// t0f / t1f are t0 rounded down / t1 rounded up to float: for a float v,
// (double)v > t0  <=>  v > t0f  and  (double)v < t1  <=>  v < t1f, so f32 cubes compare in f32.
// packed-count record format (FusedArgs::packed): nw = 0 -> not packed
struct PackFmt {
    int32_t nw;                      // 64-bit words per (slot, cell): 2 or 4
    uint32_t mask;                   // all ones of a field = NaN
    uint8_t word[MAX_COLS], shift[MAX_COLS];
};

struct ThrSlot {
    double t0, t1, A, B;
    float t0f, t1f;
    int32_t nan_poisons;  // dd: a NaN in the window makes the group NaN; bins: it does not
    int32_t pad;
};

struct ColOp {
    int32_t src, src_idx;      // SRC_*; slot index for SRC_THR
    int32_t tf, tf_iarg;       // TF_*; integer exponent for TF_POWI
    int32_t outer, skind;      // OUT_*; sine_dd kind flag (0 cooling, 1 heating)
    int32_t rounding, inter_f32;   // AFHIP_ROUND_* bits (float32 intermediates like the reference); 1: `inter` holds float32
    const void* inter;         // TF_INTER: the second cube [G1][C] (one value per inner group and cell), else null
    double s0, s1;             // sine_dd thresholds
    double s0x2, s1x2;         // 2 * s0, 2 * s1 (exact): the cooling form's 2 thr - tmax - tmin starts from them
    float s0dn, s0up, s1dn, s1up;  // s0 / s1 rounded down / up to float: for float tmin, tmax   tmin < s <=> tmin < up,  s < tmax <=> tmax > dn
    double swidth, swidth2;        // s1 - s0, 2 (s1 - s0)
    double tf_arg;             // exponent (TF_POW) or knot (TF_HINGE)
    double o0, o1, obase;      // outer dd/bins thresholds
};

// How a 16-bit-packed cube (AFHIP_I16, AFHIP_U16) becomes float32 values — the layout of afhip_packing (include/aggfly_hip.h), copied
// by value into FusedArgs.  f = (float)q, then n_pairs times  f = f * mul[i];  f = f + add[i]  with every operation rounded to float32
// (no fma), then NaN where q == fill.  A pair half the chain does not have is sent as its exact identity — mul 1.0f, add -0.0f
// (x + -0 == x for every x, the sign of zero included) — so the result is bit for bit that of the operations the chain does have.
// is_unsigned: the 16 stored bits are uint16 (q widens by zero extension, fill is 0..65535).  The public struct calls the field `pad`:
// the library writes it from the plan's dtype / the entry point's name and never reads the caller's.
struct PackArgs {
    int32_t n_pairs, has_fill, fill, is_unsigned;
    float mul[3], add[3];
};
constexpr int MAX_PACK_PAIRS = 3;

struct ChunkDesc {
    int64_t k_lo, k_hi;        // time steps [k_lo, k_hi)
    int32_t g_lo, g_hi;        // inner groups [g_lo, g_hi); k_lo == ib[g_lo], k_hi == ib[g_hi]
    int32_t slot_base, pad;
};

// LDS bytes of the two sine_dd tables (afhip_sine.h: the acos table of sine_theta, the P2 table of sine_pair_g)
constexpr int SINE_ROWS = 184;                  // rows per half: k <= 181 for u <= 0.70711; the last rows are guards
constexpr int SINE_TAB_BYTES = 2 * SINE_ROWS * 32;
constexpr int SINE_P2_N = 512;                                   // = AFHIP_SINE_P2_N of the generated table
constexpr int SINE_P2_BYTES = (SINE_P2_N + 1) * 32 + 32;         // (+ a pad row: multiple of 64 bytes)

// ---------------------------------------------------------------------------------------
// The feature bits of k_fused_temporal's template parameter FEAT: what each one compiles in.  The one definition — the kernel,
// the variant table, the planner and the launcher all read it; gen_variants.py's table is held equal by static_asserts in the
// generated variants_table.hip.
// ---------------------------------------------------------------------------------------
enum : int {
    // single-sine degree days (needs STAT >= 2).  Bulky once inlined per column, like the next bit: only the variants that need
    // them carry them
    FEAT_SINE = 1,
    // the general transforms: pow() with a non-integer exponent, and `inter` (Dataset.interact, dataset.py:483-518,547-563: the
    // inner value times the matching element of a second cube)
    FEAT_GENERAL_TF = 2,
    // non-temporal (nt) cache policy on the streaming loads
    FEAT_NT = 4,
    // every threshold slot is a bin count -> 32-bit integer counters (one v_addc per slot and element instead of fma + select +
    // f64 add)
    FEAT_INT_BINS = 8,
    // single-level plan (every inner group is an output period, every column passes its inner value through): no outer
    // accumulators at all
    FEAT_SINGLE_LEVEL = 16,
    // the bins are a contiguous equal-width partition -> per-lane histogram in LDS.  One fma + floor in the INPUT precision
    // guesses the bin (off by one at most, host-checked); the two edges around the guess come from an LDS table and four exact
    // compares move the guess up / down or reject a value that sits on an edge (strict inequalities, like the reference); one
    // ds_add_u32 bumps the lane's private counter.  A guard bin on either side absorbs out-of-range values, so there is no range
    // test and no data-dependent branch.  ~13 VALU + 2 LDS ops per element instead of 3 VALU per bin.
    FEAT_HIST = 32,
    // histogram with arithmetic edges — exactly representable equal-width edges (5 degC bins from -20 ...): the edge pair of the
    // guessed bin is computed (2 fma) instead of read from the LDS table, which takes an LDS round trip out of every element's
    // dependent chain; a value on an edge is recognised by equality
    FEAT_ARITH_EDGES = 64,
    // short-group mode: every inner group holds exactly TWO rows ((tmin, tmax) pairs per day, configs[4]) unless one of the three
    // length bits below says otherwise.  A block of DEPTH rows is DEPTH / 2 whole groups — all of them in flight at once instead
    // of one group's two rows — and a group's statistics are min / max / sum of the pair, taken in the input precision, without
    // the per-row accumulators
    FEAT_SHORT_GROUP = 128,
    // short-group mode with the LEAN group end: every column is   mean | sum | min | max | sine_dd  ->  (nothing | integer power)
    // ->  sum | mean,   without float32 rounding (configs[4]'s sine_dd -> sum; the daily mean of (tmin, tmax) and its polynomial).
    // The group end is then the column's value, its power chain and one add — no per-group walk through the column records'
    // source / transform / reducer switches; the records are loop-invariant kernel arguments and stay in scalar registers; a NaN
    // pair is remembered in a lane mask (scalar OR) and applied when the period's sum leaves the kernel, since NaN is sticky under
    // + anyway
    FEAT_LEAN = 256,
    // ... and every column is a plain sine_dd (no power), at most two of them: nothing but the closed forms in the group end
    FEAT_LEAN_SINE = 512,
    // the lean short-group form for inner groups of exactly FOUR rows (6-hourly data).  The sum runs in time order
    // ((u0 + u1) + u2) + u3, the mean is s / 4 = s * 0.25 exactly, min / max are taken in the input precision; sine_dd columns use
    // the general closed forms (tavg is not the mid-range of four steps), so these variants read the acos table
    FEAT_FOUR_ROW = 1024,
    // region-fused period ends (FusedArgs::rf_w).  A twin of the plain variant: the staging code at the period end raises the
    // register count by ~7 (one wave per SIMD less on the float32 two-cell forms), so only plans that take the route run it; with
    // rf_w == null it behaves like its twin
    FEAT_REGION_FUSED = 2048,
    // ... of exactly THREE rows (8-hourly data): the sum runs (u0 + u1) + u2, the mean is the correctly rounded s / 3 (div_by with
    // the correctly rounded reciprocal: bit-identical to the reference's division), otherwise like four rows
    FEAT_THREE_ROW = 4096,
    // ... of MIXED lengths one to four rows (a 6-hourly series with missing steps, a 12-hourly one joined to a 6-hourly one):
    // every group owns four row registers and fills as many as it is long; its length is a scalar read from the group table, the
    // loads and the statistics' tail rows sit under scalar branches on it, the mean is div_by's correctly rounded s / n (n = 2, 4:
    // exact anyway).  Otherwise the four-row form
    FEAT_MIXED = 8192,
    // histogram (FEAT_HIST only) whose partition has a WIDE END BIN on one side or both — (L, E[0]) and / or (E[n], U) of any positive
    // width, infinite included, around the equal-width lattice E[0..n].  The guard bins are the end bins: a value is counted only
    // if it also satisfies  L < v < U  (two compares in the input precision against the end slots' own t0f / t1f; NaN fails both),
    // and an end slot reads its guard counter (hb_bin_of_slot = -1 / hb_n).  Clamp, guess, repair and "a value on an edge is in no
    // bin" are the closed form's
    FEAT_END_BINS = 16384,
    // histogram with end bins (FEAT_HIST | FEAT_END_BINS, never FEAT_ARITH_EDGES) whose INTERIOR bins have unequal widths: the fma
    // guesses a CELL of a lattice of half the smallest interior width, and one byte read from a cell -> bin map in LDS (FusedArgs::
    // hb_cmap, copied behind the counters at kernel start) turns it into the guessed bin.  Everything after the guess — edge table,
    // repair by +-1, "a value on an edge is in no bin", the outer limits, the counters — is the end-bin form's (afhip_cell_map.h has
    // the construction and the host check that the guess is one bin off at most)
    FEAT_CELL_MAP = 32768,
};

// what follows from the bits
constexpr bool feat_has(int feat, int bits) { return (feat & bits) != 0; }
// rows a short-group variant gives each group (k_fused_temporal: GL)
constexpr int feat_group_rows(int feat) { return feat_has(feat, FEAT_FOUR_ROW | FEAT_MIXED) ? 4 : (feat_has(feat, FEAT_THREE_ROW) ? 3 : 2); }
// lean group end: 0 none, 1 lean, 2 its sine-only form
constexpr int feat_lean_level(int feat) { return feat_has(feat, FEAT_LEAN_SINE) ? 2 : (feat_has(feat, FEAT_LEAN) ? 1 : 0); }
// group-length rule of a short-group variant: 0 two rows (or not a short-group variant), 1 four, 2 three, 3 mixed one to four
constexpr int feat_group_form(int feat) { return feat_has(feat, FEAT_FOUR_ROW) ? 1 : (feat_has(feat, FEAT_THREE_ROW) ? 2 : (feat_has(feat, FEAT_MIXED) ? 3 : 0)); }
// sine_dd reads the P2 table of sine_pair_g (tavg is the mid-range: two-row groups only), otherwise the acos table of sine_theta
constexpr bool feat_sine_p2(int feat) { return feat_has(feat, FEAT_SHORT_GROUP) && feat_group_form(feat) == 0; }
constexpr int feat_sine_bytes(int feat) { return feat_sine_p2(feat) ? SINE_P2_BYTES : SINE_TAB_BYTES; }

// The kernel's dynamic LDS, front to back: the LDS-DMA ring (PIPE 1: one block of DEPTH rows of 1 KiB per wave), then the sine
// table of a plan with a sine_dd column; histogram variants (direct loads, no sine_dd) hold their edge tables and counters there
// instead; the parking blocks of a region-fused launch come last (FusedArgs::rf_lds_off).
constexpr size_t lds_ring_bytes_per_wave(int depth) { return (size_t)depth * 1024; }
constexpr size_t lds_sine_offset(int pipe, int waves, int depth) { return pipe == 1 ? (size_t)waves * lds_ring_bytes_per_wave(depth) : (size_t)0; }
// (FEAT_CELL_MAP: + the 256-byte cell map, behind the counters — plan_lds_bytes)
constexpr size_t lds_hist_bytes(int bins, int vec, int wg) { return (size_t)HB_TABLE_BYTES + (size_t)bins * vec * wg * 4; }    // counters [bins * vec][wg]; bins = hb_n + 2 with the guards
constexpr int rf_lane_bytes(int vec) { return vec * 16 + 16; }     // a lane's parking block: its cells' weight pairs + its two lane words (a multiple of 16: read and written in 16-byte pieces)

}  // namespace afhip
