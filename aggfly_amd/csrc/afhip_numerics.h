// afhip_numerics.h — device arithmetic helpers of k_fused_temporal (afhip_kernels.h): integer powers by a double-double chain, f64 division / reciprocal without the
// library's scaling code, operand-pinned fma / max / min forms
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace afhip {

// ---------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double nan64() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ double inf64() { return __longlong_as_double(0x7ff0000000000000LL); }

// A volatile empty asm cannot be speculated, so a block that starts with it stays behind its branch.
#define KEEP_BRANCH() asm volatile("")

// min(max(x, -2^1023), 2^1023) IN PLACE: NaN and +-inf become finite (v_max returns its other operand for a NaN), every |x| <= 2^1023
// stays as it is.  The bound is built in VCC inside the block — a constant kept in a scalar register pair across the time loop cost
// the kernels two SGPRs and thirteen of them 34 more scalar spills — so: no new VGPR, no new SGPR, two SALU + two VALU.
__device__ __forceinline__ double clamp_finite(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("s_mov_b32 vcc_lo, 0\n\ts_mov_b32 vcc_hi, 0x7fe00000\n\tv_max_f64 %0, %0, -vcc\n\tv_min_f64 %0, %0, vcc" : "+v"(x) : : "vcc");
    return x;
#else
    return x != x ? -0x1p1023 : (x > 0x1p1023 ? 0x1p1023 : (x < -0x1p1023 ? -0x1p1023 : x));
#endif
}
// The last step of powi_dd_vec's chain (below), hi + lo — but once the product has overflowed, the error term is no error of anything: hi = +-inf comes with
// lo = fma(inf, x, -inf) = NaN or an infinity of the other sign, and hi + lo would be NaN where np.power gives +-inf.  The term is
// made finite in place (inf + finite = inf).  (A v_cmp_class on hi and a select — between hi and hi + lo, or on lo — kept two more
// VGPRs alive in 343 / 441 of the 529 kernels and cost 18 / 36 of them a wave per SIMD; profiles/special_values.txt.)
__device__ __forceinline__ double powi_finish(double hi, double lo) { return hi + clamp_finite(lo); }
// ... with the chain's sign.  hi + lo has hi's sign wherever it is not zero (|lo| is a few ulps of hi); where it is zero it is +0 unless
// both are -0, and hi's sign is the power's.  So hi's sign bit is OR-ed in: two VALU on the high dword, no compare, no select, nothing
// kept alive.  The mask is a literal of the v_and_b32 itself: as a copysign the compiler parks 0x7fffffff in a scalar register for the
// whole kernel, which cost one variant its eighth wave (profiles/numerics_exact.txt).  That is one compiler's register allocation:
// __builtin_copysign(x, hi) computes the same value on every (x, hi) the chain produces and is the form to go back to, resource lines
// permitting, should a toolchain reject or mis-schedule the assembly.  (An OR, not a copysign: the two differ where x < 0 <= hi, which
// the chain cannot produce; the host branch below is the same OR.)
__device__ __forceinline__ double or_sign(double x, double hi) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t hh = (uint32_t)((uint64_t)__double_as_longlong(hi) >> 32);
    uint32_t s;
    asm("v_and_b32 %0, 0x80000000, %1" : "=v"(s) : "v"(hh));
    return __longlong_as_double((long long)((uint64_t)__double_as_longlong(x) | ((uint64_t)s << 32)));
#else
    uint64_t xb, hb;
    __builtin_memcpy(&xb, &x, 8);
    __builtin_memcpy(&hb, &hi, 8);
    xb |= hb & 0x8000000000000000ull;
    __builtin_memcpy(&x, &xb, 8);
    return x;
#endif
}

// x**e for a small integer e, evaluated as a double-double product chain so that the
// result is the correctly rounded power in all but ~1e-14 of cases — what libm's pow()
// behind np.power (dataset.py:543) returns.  Plain repeated multiplication differs from
// np.power in the last bit for 26-35 % of inputs at e = 3, 4.
// The exponent is wave-uniform: one scalar loop drives the N independent chains of a lane.
//
// The pair (hi, lo) is NOT renormalised between steps: (hi + lo) x = p + (err + lo x) with p = RN(hi x), err = hi x - p exactly
// (one fma) and the small term rounded once (a second fma) — |lo| stays within a few ulps of hi for every exponent lowered to this
// form (|e| <= 64), so its rounding errors are of order 2^-106 and only the final hi + lo rounds at 2^-53.  Three instructions per
// step, two for the first (lo = 0), instead of the six of a renormalising step: x^3 6 instructions, x^4 9 (were 13 and 19).
// Zeros: a power that underflows is the +-0 of its product chain — hi — where hi + lo may be -0 + +0 = +0, and under a negative
// exponent that sign is the sign of an infinity ((-0)^-3 and (-1e-200)^-3 are -inf).  The result takes hi's sign bit (or_sign, above) in every form
// that divides or promises np.power's signed zeros (NEG, ZERO_SIGN: k_transform's chain on a scaled mantissa runs with NEG off).
//
// What the chain ON x ITSELF does not reach (tests/numerics_cases.py holds every exponent to exact rational arithmetic):
// "err = hi x - p exactly" needs err representable, so a power below 2^-969 = 2^(-1022 + 53) in magnitude, whose error terms are
// subnormal or lost, is within one ulp (one step, 2^-1074, below 2^-1022) of the exact power instead of correctly rounded; and a
// negative exponent takes the reciprocal of the positive power, whatever became of that: +-0 where it overflowed though the exact
// power is a subnormal, the reciprocal of a product with few bits left where it was subnormal.  The fused kernels keep that
// (powi_scaled_vec in all of them cost 17 variants a wave per SIMD and one 208 bytes of scratch: profiles/numerics_exact.txt);
// k_transform does not (powi_scaled_vec, below).
template <int N, bool NEG = true, bool ZERO_SIGN = false>
__device__ __forceinline__ void powi_dd_vec(double (&x)[N], int e) {
    if (e == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = 1.0;
        return;
    }
    const int n = e < 0 ? -e : e;
    if (n == 2) {                       // the chain's first step is RN(x * x) exactly: one multiply
        KEEP_BRANCH();
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = x[i] * x[i];
    } else if (n > 2) {
        double hi[N], lo[N];
#pragma unroll
        for (int i = 0; i < N; ++i) { hi[i] = x[i] * x[i]; lo[i] = __fma_rn(x[i], x[i], -hi[i]); }
        auto step = [&]() {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const double p = hi[i] * x[i];
                const double err = __fma_rn(hi[i], x[i], -p);
                lo[i] = __fma_rn(lo[i], x[i], err);
                hi[i] = p;
            }
        };
        step();                         // n >= 3; the cube and the fourth power (polynomials) are straight-line code: a loop
        if (n > 3) {                    // carries (hi, lo) through register copies
            KEEP_BRANCH();
            step();
            for (int it = 4; it < n; ++it) step();
        }
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = powi_finish(hi[i], lo[i]);
        if constexpr (NEG || ZERO_SIGN) {
#pragma unroll
            for (int i = 0; i < N; ++i) x[i] = or_sign(x[i], hi[i]);
        }
    }
    if constexpr (NEG) {                // (the lean short-group forms take non-negative exponents only: no division code in them)
        if (e < 0) {
            KEEP_BRANCH();
#pragma unroll
            for (int i = 0; i < N; ++i) x[i] = 1.0 / x[i];
        }
    }
}

// frexp as two instructions, without the library's special-case code: v_frexp_mant_f64 / v_frexp_exp_i32_f64 split a finite non-zero
// x (subnormals included) into f in +-[0.5, 1) and k with x = f 2^k, and return (x, 0) for x = +-0, +-inf and NaN.
__device__ __forceinline__ double frexp_mant(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_frexp_mant(x);
#else
    int k;
    return (x == 0.0 || x != x || x - x != 0.0) ? x : frexp(x, &k);
#endif
}
__device__ __forceinline__ int frexp_exp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_frexp_exp(x);
#else
    int k = 0;
    if (!(x == 0.0 || x != x || x - x != 0.0)) (void)frexp(x, &k);
    return k;
#endif
}
// The library's pow(x, y), except where x = +-2^m and m y is an integer: that power is +-2^(m y) exactly, by v_ldexp_f64 — the
// library's pow is within an ulp or two and gave the neighbour of 2^130 for 4^65 (tests/test_gpu_numerics.py: the lowering boundary).
// m y is formed without a rounding (the fma's remainder is zero) or the library's value stands; a negative x needs an integer y,
// whose parity gives the sign; +-0, +-inf and NaN have no mantissa of +-0.5 and keep the library's answers.  k_transform's form.
__device__ __forceinline__ double pow_exact_pow2(double x, double y) {
    double r = pow(x, y);
    const double f = frexp_mant(x);
    if (f == 0.5 || f == -0.5) {
        const double m = (double)(frexp_exp(x) - 1);
        const double my = m * y;
        const bool whole = my == floor(my) && __fma_rn(m, y, -my) == 0.0 && fabs(my) < 4096.0;
        if (whole && (x > 0.0 || y == floor(y))) {
            const bool neg = x < 0.0 && 0.5 * y != floor(0.5 * y);          // an odd integer y (from 2^53 on every double is even)
            r = ldexp(neg ? -1.0 : 1.0, (int)my);
        }
    }
    return r;
}

// x**e as powi_dd_vec<N, true, true> gives it, for every x: for |e| >= 3 and e = -2 the chain runs on frexp's mantissa f — every
// product in [2^-64, 1), every error term normal or zero, nothing overflows — and x^e = f^e 2^(k e) by one v_ldexp_f64, which is exact
// where the result is normal, rounds once more where it is subnormal (within one step, 2^-1074, of the exact power) and saturates to
// +-inf / +-0.  So a positive power is correctly rounded down to 2^-1022, (2^20)^-52 is 2^-1040 instead of the reciprocal of an
// infinity, and a negative power is within one ulp whatever the size of the positive one.  Four more instructions per element and an
// int register each: k_transform's form, a plain HBM stream with VALU to spare.  x^2 and x^-1 stay single IEEE operations.
template <int N>
__device__ __forceinline__ void powi_scaled_vec(double (&x)[N], int e) {
    const int n = e < 0 ? -e : e;
    if (n < 2 || e == 2) {
        powi_dd_vec<N, true, true>(x, e);
        return;
    }
    int k[N];
#pragma unroll
    for (int i = 0; i < N; ++i) { k[i] = frexp_exp(x[i]) * e; x[i] = frexp_mant(x[i]); }
    powi_dd_vec<N, false, true>(x, n);
    if (e < 0) {
        KEEP_BRANCH();
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = 1.0 / x[i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = ldexp(x[i], k[i]);
}
__device__ __forceinline__ double powi_dd(double x, int e) {
    double v[1] = {x};
    powi_dd_vec<1>(v, e);
    return v[0];
}

// ---- f64 division / square root without the library's scaling and special-case code ----
// 1/x for normal x: v_rcp_f64 (measured 2^-24.4 on gfx950, scripts/probe/rcp_rsq_probe.py) + one Newton step: <= 10 ulp
// (2.2e-15).  Enough for sine_arc's quotients: their error only matters next to |x| = 1, where the closed forms are
// ill-conditioned by themselves.
__device__ __forceinline__ double rcp_newton1(double x) {
    const double y = __builtin_amdgcn_rcp(x);
    const double e = __fma_rn(-x, y, 1.0);
    return __fma_rn(y, e, y);
}
// rcp_newton1 for a window's range: a SUBNORMAL range (a window of +- the smallest subnormals: below 2^-1022) has no finite
// reciprocal seed — v_rcp_f64 gives inf, the Newton step NaN, and sine_dd was NaN where the reference's division gives a value
// of the order of the range.  min(., 2^1022) leaves the reciprocal of every normal range as it is (<= 2^1022; doubled for the
// heating form it stays finite) and takes inf / NaN to 2^1022: the quotient z then keeps its sign and |z| <= 1, so the arc is
// finite and, like the exact one, below four times the range (< 9e-308) in size.  One v_min_f64, the bound built in VCC (clamp_finite).
__device__ __forceinline__ double rcp_range(double x) {
    double y = rcp_newton1(x);
#if defined(__HIP_DEVICE_COMPILE__)
    asm("s_mov_b32 vcc_lo, 0\n\ts_mov_b32 vcc_hi, 0x7fd00000\n\tv_min_f64 %0, %0, vcc" : "+v"(y) : : "vcc");
#else
    y = (y < 0x1p1022) ? y : 0x1p1022;
#endif
    return y;
}
// a / b given y ~ 1/b (Markstein): q0 = a*y, r = a - b*q0 exactly (fma), q = q0 + r*y.  With y the
// CORRECTLY rounded reciprocal (the host's 1.0/n for a group length n) q is the correctly rounded
// quotient — bit-identical to a true division — wherever |a / b| >= 2^-1022; a SUBNORMAL quotient is
// within one step (2^-1074) of it: r is exact, but q0 + r*y then rounds a value that is not a / b, and
// on an exact tie (2856 * 2^-1074 / 48 = 59.5 steps) the rounded y decides the direction instead of
// ties-to-even.  Checked against exact rational arithmetic over group lengths 1 .. 48 in
// tests/test_numerics_host.py (the emulated text) and tests/test_gpu_numerics.py (the kernels);
// DESIGN.md §5.  With a faithful y it is within 1 ulp.  v_div_fixup restores the IEEE results for
// inf / NaN / zero operands.
__device__ __forceinline__ double div_by_finite(double a, double b, double y) {   // finite a, normal b
    const double q0 = a * y;
    const double r = __fma_rn(-q0, b, a);
    return __fma_rn(r, y, q0);
}
__device__ __forceinline__ double div_by(double a, double b, double y) {
    return __builtin_amdgcn_div_fixup(div_by_finite(a, b, y), b, a);
}
// d = a * b + c as ONE three-address v_fma_f64 with the (wave-uniform) factor b in a scalar register pair and the addend in a
// vector register: hipcc otherwise emits v_mov_b64 + v_fmac_f64 (the two-address form clobbers its addend).
__device__ __forceinline__ double fma_vsv(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(b), "v"(c));
    return d;
#else
    return __builtin_fma(a, b, c);
#endif
}
// a * b + c with the addend in scalar registers (three-address form: the compiler's v_fmac needs a v_mov of the constant first)
__device__ __forceinline__ double fma_vvs(double a, double b, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    double d;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c));
    return d;
#else
    return __builtin_fma(a, b, c);
#endif
}
// (k << n) + base in one instruction
__device__ __forceinline__ uint32_t lshl_add(uint32_t base, uint32_t k, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t d;
    asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(d) : "v"(k), "n"(n), "v"(base));
    return d;
#else
    return (k << n) + base;
#endif
}
// max(x, 0) / max(-x, 0) as one v_max_f64: the builtin first canonicalises an operand it cannot prove quiet (v_max x, x);
// a NaN operand gives 0 either way (callers replace the value of a NaN window afterwards)
__device__ __forceinline__ double max0(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double d;
    asm("v_max_f64 %0, %1, 0" : "=v"(d) : "v"(x));
    return d;
#else
    return x > 0.0 ? x : 0.0;
#endif
}
// min(x, c) with the wave-uniform c in a scalar register pair, one instruction (no canonicalising v_max in front)
__device__ __forceinline__ double min_vs(double x, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
    double d;
    asm("v_min_f64 %0, %1, %2" : "=v"(d) : "v"(x), "s"(c));
    return d;
#else
    return x < c ? x : c;
#endif
}
__device__ __forceinline__ double max0_neg(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double d;
    asm("v_max_f64 %0, -%1, 0" : "=v"(d) : "v"(x));
    return d;
#else
    return -x > 0.0 ? -x : 0.0;
#endif
}

}  // namespace afhip
