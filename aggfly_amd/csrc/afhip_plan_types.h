// afhip_plan_types.h — what the host planner (afhip_planner.cpp) and the device code (afhip_kernels.h) share: launch constants,
// the column / slot / chunk records that FusedArgs copies by value, and the LDS sizes of the sine tables.  Plain C++: no HIP.
#pragma once
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

}  // namespace afhip
