// const_div.hpp -- x / d for a divisor that does not change from call to call, without the ~11-instruction IEEE
// division sequence:
//     q0 = x * r;  e = fma(-d, q0, x);  q = fma(e, r, q0)        with r = RN(1 / d).
// Whether q is the correctly rounded quotient depends on d and on the range of x, so every user keeps a guard in front
// of it and redoes the work with true divisions when the guard trips; tools/verify_const_div.c proves the ranges by
// trying every dividend.
//
//   * Stage 2 (k_haar_select32.hip), d = sqrtf(2), sqrtf(32), sqrtf(128): ALL 2^32 inputs checked; q equals the
//     correctly rounded quotient bit for bit whenever 2^-105 <= |x| < inf (and for +0; -0 gives +0, which no later
//     step can tell apart).  DivGuard records what a line met:
//       - every dividend: min over t = 2 |x|bits - 1 (one shift-add per value, one min3 per pair); zero wraps to
//         0xFFFFFFFF and never trips it, anything in (0, 2^-100) does;
//       - the 16 values a line starts from: max over |x|bits <= 2^126.  Later dividends are sums and differences of
//         quotients, at most 4x the largest input after four levels, so they stay finite.
//   * Stage 1 (k_rows_pruned.hip), the band means: d is a small integer, x a sum of squares (+0, positive finite or
//     +inf, never NaN).  For the divisors listed in band_div_proven.inc +0 and every dividend bit pattern in
//     [kBandDivLo, kBandDivHi] give the correctly rounded quotient (profiles/const_div_bands.txt is the tool's output
//     the list is generated from, tools/gen_band_div_table.py the generator).  Odd divisors and powers of two are
//     exact down to the smallest denormal; the other even ones fail where the quotient is denormal, and +inf fails
//     for every divisor (inf - inf).  The guard is DivGuard's minimum on the low side and one comparison against
//     the largest finite float on the high side.  Any other divisor keeps the true division.
#pragma once
#include <cstdint>

namespace lbad {

constexpr uint32_t kFastDivLo = 0x0D800000u;   // 2^-100
constexpr uint32_t kFastDivHi = 0x7E800000u;   // 2^126

// band means: +0 and dividends in [kBandDivLo, kBandDivHi] are proven for the divisors of band_div_proven.inc
constexpr uint32_t kBandDivLo = kFastDivLo;
constexpr uint32_t kBandDivHi = 0x7F7FFFFFu;   // the largest finite float

// integer divisors for which tools/verify_const_div.c found the short form exact on [kBandDivLo, kBandDivHi]
inline bool band_div_proven(float d) {
    static const uint32_t proven[] = {
#include "band_div_proven.inc"
    };
    for (uint32_t v : proven)
        if (d == (float)v) return true;
    return false;
}

#ifdef __HIPCC__
struct DivGuard {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    __device__ __forceinline__ void dividends(float a, float b) {
        lo = min(lo, min((__float_as_uint(a) << 1) - 1u, (__float_as_uint(b) << 1) - 1u));
    }
    __device__ __forceinline__ void inputs(float a, float b) {
        hi = max(hi, max(__float_as_uint(a) & 0x7fffffffu, __float_as_uint(b) & 0x7fffffffu));
    }
    __device__ __forceinline__ bool bad() const { return lo < 2u * kFastDivLo - 1u || hi > kFastDivHi; }
};

template <bool FAST>
__device__ __forceinline__ float div_c(float x, float d, float r) {
    if constexpr (FAST) {
        const float q0 = __fmul_rn(x, r);
        const float e = __fmaf_rn(-d, q0, x);
        return __fmaf_rn(e, r, q0);
    } else {
        return __fdiv_rn(x, d);
    }
}
#endif

}  // namespace lbad
