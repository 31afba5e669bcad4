// shadow_scale_plan.h -- the host arithmetic of the int8 filter shadow's COMMON scale ("One common scale"):
// when a load keeps one scale s_c for every row of the shadow instead of the reference's per-row scales, and when rows written
// later (nvdb_hip_insert_rows, nvdb_hip_ivf_add_rows) let the fact stand.  Plain C++ with no HIP call in it, so that the sanitizer
// build of tests/shadow_scale_plan_check.cpp compiles the very code the entry points run (as insert_plan.h, compact_plan.h).
//
// The fact "every entry of the shadow's scale array equals s_c" lets the flat search run the filter build whose first-stage test
// compares raw accumulator bits (shadow_i8c_kernel, kernels_filter_i8s.h) against shadow_cs_bits_bar below.  The search stays exact under either rule: the band is
// ||q|| x resid_max with resid_max measured under the rule that wrote the rows.  The rule below only keeps the band from widening
// by more than SHADOW_CS_MARGIN.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define NVDB_CS_HD __host__ __device__
#else
#define NVDB_CS_HD
#endif

namespace nvdbhip {

constexpr int SHADOW_CS_ACC_BIAS = 0x4B000000;     // the int8 kernels' accumulator bias (the bits of 2^23 as a float)
constexpr int SHADOW_CS_H_MAX = 8384000;           // |H| <= 128 * 65500: the hi plane's L1 bound (prep_q8_kernel keeps it)

// The common-scale shadow may cost at most this much more residual than the per-row shadow.  The filter's band is linear in
// resid_max and a launch's survivors grow with the band: doubling the band cost the bench line 7.7 % (round 6), the cheaper test
// can save at most 5.8 % of a pass, so a quarter more band (about 2 %) is where the trade stops paying.
constexpr float SHADOW_CS_MARGIN = 0.25f;

// s_c must be a scale the kernels' arithmetic is exact about: positive, finite, and so that H * s_c (|H| < 2^23) neither
// overflows nor leaves the normal range for H != 0.  s_c = 0 (a corpus of zeros) and NaN fail here.
inline bool shadow_cs_scale_ok(float s_c) { return s_c >= 1e-30f && s_c <= 1e30f; }

struct ShadowScaleFact {
  bool common = false;                             // every entry of the shadow's scale array equals s_c
  float s_c = 0.f;                                 // the common scale (0: none)
  float resid_row = 0.f, resid_common = 0.f;       // resid_max the load measured under the per-row rule / under s_c (0: not measured)
};

// Does the load TRY the common scale?  opt: option shadow_common_scale (0 = off, anything else = automatic); bad: a row holds a
// non-finite element (the load builds no shadow at all then); s_c: the largest per-row reference scale.
inline bool shadow_cs_try(int64_t opt, bool bad, float s_c) { return opt != 0 && !bad && shadow_cs_scale_ok(s_c); }

// ... and does it KEEP it, the rows requantised under s_c having given resid_common?  An outlier row that quantises well under
// its own scale makes every other row quantise worse under s_c: resid_common leaves the margin and the load goes back to the
// per-row rule.  (An outlier that already sets the per-row resid_max costs the band nothing more and is kept.)  A NaN on either
// side fails the comparison.
inline bool shadow_cs_keep(float resid_row, float resid_common, bool bad_common) {
  return !bad_common && resid_row >= 0.f && resid_common <= resid_row * (1.0f + SHADOW_CS_MARGIN);
}

// Rows written after the load were quantised under f.s_c; new_scale_max is the largest reference scale among them.  A row above
// s_c has clipped: the caller requantises the new rows per row and the fact falls (the old rows stay as they are -- a valid
// per-row-scale shadow whose scales happen to be equal).  Returns whether the fact still stands.
inline bool shadow_cs_after_write(ShadowScaleFact& f, float new_scale_max) {
  if (f.common && !(new_scale_max <= f.s_c)) f.common = false;
  return f.common;
}

// The first-stage bar in the bits domain.  A value is logged iff fl(float(H) * s_c) >= t1q (shadow_i8c_kernel's rare_log, kernels_filter_i8s.h; float(H) is exact, |H| < 2^23).
// With r = t1q / s_c (real numbers, s_c > 0) and fl(H s_c) = H s_c (1 + e), |e| <= 2^-24 (s_c in [1e-30, 1e30]: no overflow, and
// H s_c is normal for H != 0):
//   r > 0:  a logged H is positive and H >= r / (1 + e) >= r (1 - 2^-24);
//   r < 0:  a logged H is >= 0, or negative with |H| <= |r| / (1 + e) <= |r| (1 + 2^-23), that is H >= r (1 + 2^-23);
//   r = 0:  a logged H is >= 0.
// Every case gives H >= r -+ r 2^-22 - 1 with room for the double division's own rounding (2^-53), so Hb = floor(r (1 -+ 2^-22)) - 1
// never exceeds a logged H: the bar is conservative toward "flag", by at most 3 + |r| 2^-22 <= 5 steps of H.  The accumulator of H
// holds the int32 SHADOW_CS_ACC_BIAS + H (kernels_filter.h: I8_ACC_BIAS, the bits of 2^23); for |H| < 2^23 that is the bit pattern of a positive normal float -- 2^23 + H for H >= 0 and
// 2^23 + H / 2 for H < 0 (one binade down, spacing 1/2: still one pattern per H) -- and positive floats order as their patterns
// do.  So "H >= Hb" is "bits as float >= (SHADOW_CS_ACC_BIAS + Hb) as float", exactly, for negative H as for positive.  |H| <= 128 *
// I8_HI_L1_MAX = 8384000: an Hb above that flags nothing (+inf), one below -8384000, t1q = -inf and a NaN t1q flag everything
// (a NaN bar logs nothing in rare_log, as in the per-row build, whose flag is false for it).
NVDB_CS_HD inline float shadow_cs_bits_bar(float t1q, float s_c) {
  const double r = static_cast<double>(t1q) / static_cast<double>(s_c);
  const double hb = __builtin_floor(r * (r > 0.0 ? 1.0 - 0x1p-22 : 1.0 + 0x1p-22)) - 1.0;
  if (hb > static_cast<double>(SHADOW_CS_H_MAX)) return __builtin_huge_valf();
  const int Hb = hb >= -static_cast<double>(SHADOW_CS_H_MAX) - 1.0 ? static_cast<int>(hb) : -SHADOW_CS_H_MAX - 1;      // (a NaN fails the comparison: flag everything)
  return __builtin_bit_cast(float, SHADOW_CS_ACC_BIAS + Hb);
}

}  // namespace nvdbhip
