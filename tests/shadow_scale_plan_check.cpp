// shadow_scale_plan_check.cpp -- the rule of the int8 filter shadow's common scale (nano-vectordb_amd/csrc/shadow_scale_plan.h, the
// code the load and the insertion run) as a stand-alone program for AddressSanitizer / UBSan.  The quantiser here is the host
// restatement of shadow_q8_kernel (scale = max|x| / 127 per row, or one common scale; rint, clamp +-127; residual norm): it feeds
// the rule what a load would measure on small corpora built to land on either side of it.
#include "shadow_scale_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace nvdbhip;

namespace {

struct Measured { float resid = 0.f, scale_max = 0.f; bool bad = false; };

// common == 0: every row under its own reference scale
Measured quantise(const std::vector<std::vector<float>>& rows, float common) {
  Measured m;
  for (const auto& row : rows) {
    float mx = 0.f;
    for (float x : row) mx = std::fmax(mx, std::fabs(x));
    if (!(mx < 3.0e38f)) m.bad = true;
    m.scale_max = std::fmax(m.scale_max, mx / 127.f);
    const float scale = common > 0.f ? common : mx > 0.f ? mx / 127.f : 1.f;
    const float inv = 1.0f / scale;
    float ss = 0.f;
    for (float x : row) {
      const float qv = std::fmin(std::fmax(std::rint(x * inv), -127.f), 127.f);
      const float d = x - qv * scale;
      ss = std::fma(d, d, ss);
    }
    if (!(ss == ss)) m.bad = true;
    m.resid = std::fmax(m.resid, std::sqrt(ss) * 1.0001f);
  }
  return m;
}

// what a load does (nvdb_corpus.cpp): reduction pass, try, keep
ShadowScaleFact load(const std::vector<std::vector<float>>& rows, int64_t opt, float& resid_in_force) {
  ShadowScaleFact f;
  const Measured row = quantise(rows, 0.f);
  f.resid_row = row.resid; f.s_c = row.scale_max;
  resid_in_force = row.resid;
  if (shadow_cs_try(opt, row.bad, f.s_c)) {
    const Measured com = quantise(rows, f.s_c);
    f.resid_common = com.resid;
    f.common = shadow_cs_keep(f.resid_row, f.resid_common, com.bad);
    if (f.common) resid_in_force = com.resid;
  }
  return f;
}

std::vector<float> noise_row(uint32_t seed, int dim, float amp) {
  std::vector<float> r(dim);
  uint32_t s = seed * 2654435761u + 12345u;
  for (int c = 0; c < dim; ++c) { s = s * 1664525u + 1013904223u; r[c] = amp * (static_cast<float>(s >> 8) / 8388608.f - 1.f); }
  return r;
}

// ---- the bits-domain bar (shadow_cs_bits_bar) against the kernel's exact test float(H) * s_c >= t1q ---------------------------
// as the kernel sees an accumulator: the int32 BIAS + H read as a float
float acc_as_float(int H) { return __builtin_bit_cast(float, SHADOW_CS_ACC_BIAS + H); }
bool logged(int H, float s_c, float t1q) { volatile float p = static_cast<float>(H) * s_c; return p >= t1q; }   // rare_log's test, rounded once to fp32

// every H of [lo, hi]: a logged H must be flagged (bar + shift; shift = 0 is the bar itself); returns the flagged H that are not logged
// or -1 when a logged H is missed
int sweep(float t1q, float s_c, int lo, int hi, int step, int shift) {
  float bar = shadow_cs_bits_bar(t1q, s_c);
  if (shift && bar < 3.0e38f) bar = __builtin_bit_cast(float, __builtin_bit_cast(int, bar) + shift);
  int extra = 0;
  for (long long H = lo; H <= hi; H += step) {
    const bool flag = acc_as_float(static_cast<int>(H)) >= bar, hit = logged(static_cast<int>(H), s_c, t1q);
    if (hit && !flag) return -1;
    if (flag && !hit) ++extra;
  }
  return extra;
}

int fails = 0;
void expect(bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++fails; } else std::printf("checked %s\n", what); }

}  // namespace

int main() {
  const int dim = 256;
  float resid = 0.f;
  // rows of one kind: the common scale costs next to nothing and is kept; the option turns it off
  std::vector<std::vector<float>> equal;
  for (uint32_t r = 0; r < 64; ++r) equal.push_back(noise_row(r, dim, 1.f));
  ShadowScaleFact f = load(equal, -1, resid);
  expect(f.common && f.s_c > 0.f && f.resid_common <= f.resid_row * (1.f + SHADOW_CS_MARGIN) && resid == f.resid_common, "equal rows keep the common scale");
  ShadowScaleFact off = load(equal, 0, resid);
  expect(!off.common && off.resid_common == 0.f && resid == off.resid_row, "option 0 keeps the per-row rule");
  // one outlier row, 10x longer, that quantises exactly under its own scale: everything else pays under s_c -> declined
  std::vector<std::vector<float>> outlier = equal;
  outlier.push_back(std::vector<float>(dim, 10.f));
  for (int c = 0; c < dim; c += 2) outlier.back()[c] = -10.f;
  f = load(outlier, -1, resid);
  expect(!f.common && f.resid_common > f.resid_row * (1.f + SHADOW_CS_MARGIN) && resid == f.resid_row, "an outlier row that widens the residual is declined");
  // an outlier of the same kind as the rest already sets the per-row residual: kept, the band does not widen
  std::vector<std::vector<float>> dense = equal;
  dense.push_back(noise_row(1000, dim, 10.f));
  f = load(dense, -1, resid);
  expect(f.common && f.resid_common <= f.resid_row * (1.f + SHADOW_CS_MARGIN), "an outlier that already sets the per-row residual is kept");
  // a corpus of zeros: s_c = 0 fails shadow_cs_scale_ok
  std::vector<std::vector<float>> zeros(8, std::vector<float>(dim, 0.f));
  f = load(zeros, -1, resid);
  expect(!f.common && f.s_c == 0.f && !shadow_cs_scale_ok(0.f), "a corpus of zeros keeps the per-row rule");
  // zero rows among others are no obstacle
  std::vector<std::vector<float>> some_zero = equal;
  some_zero.push_back(std::vector<float>(dim, 0.f));
  f = load(some_zero, -1, resid);
  expect(f.common, "zero rows among others keep the common scale");
  // non-finite elements: inf, NaN
  for (float v : {std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()}) {
    std::vector<std::vector<float>> bad = equal;
    bad[3][7] = v;
    f = load(bad, -1, resid);
    expect(!f.common, "a non-finite element keeps the per-row rule (the load builds no shadow)");
  }
  expect(!shadow_cs_scale_ok(std::numeric_limits<float>::quiet_NaN()) && !shadow_cs_scale_ok(std::numeric_limits<float>::infinity()) &&
         !shadow_cs_scale_ok(1e-31f) && !shadow_cs_scale_ok(1e31f) && !shadow_cs_scale_ok(-1.f) && shadow_cs_scale_ok(1e-30f) && shadow_cs_scale_ok(1.f),
         "the range of scales the bits-domain bar is exact about");
  expect(!shadow_cs_keep(1.f, std::numeric_limits<float>::quiet_NaN(), false) && !shadow_cs_keep(std::numeric_limits<float>::quiet_NaN(), 1.f, false) &&
         !shadow_cs_keep(1.f, 1.f, true) && shadow_cs_keep(1.f, 1.25f, false) && !shadow_cs_keep(1.f, 1.2501f, false) && shadow_cs_keep(0.f, 0.f, false),
         "keep: NaN and a bad pass fail, the margin is inclusive");
  // insertion: a row at or below s_c leaves the fact, one above clears it for good
  f = load(equal, -1, resid);
  const float s_c = f.s_c;
  expect(shadow_cs_after_write(f, s_c * 0.5f) && f.common, "an inserted row below s_c leaves the fact");
  expect(shadow_cs_after_write(f, s_c) && f.common, "an inserted row at s_c leaves the fact");
  expect(!shadow_cs_after_write(f, std::nextafter(s_c, 2.f * s_c)) && !f.common && f.s_c == s_c, "an inserted row above s_c clears the fact");
  expect(!shadow_cs_after_write(f, s_c * 0.5f) && !f.common, "a cleared fact stays cleared");
  f = load(equal, -1, resid);
  expect(!shadow_cs_after_write(f, std::numeric_limits<float>::quiet_NaN()) && !f.common, "a NaN scale among the new rows clears the fact");
  // the residual of the rows the insertion quantised under s_c joins resid_max as before: a row under s_c has at most the
  // rounding error of a full-range row
  {
    std::vector<std::vector<float>> small{noise_row(77, dim, 0.01f)};
    const Measured m = quantise(small, s_c);
    expect(m.resid <= 0.5f * s_c * std::sqrt(static_cast<float>(dim)) * 1.001f, "a small row under s_c: residual within half a step per element");
  }
  // the bar: H swept +-48 around it (every H), and the whole range of H at a stride, for bars at H0 x s_c and a few ulps to either side
  // -- positive, negative (where the accumulator reads 2^23 + H / 2: half spacing), zero, at the binade edge 2^22, at the ends of the
  // range of H and of s_c -- and for t1q = +-0, +-inf, NaN, huge and tiny.  shift > 0 is the self-check: a bar a few steps of H
  // too high must be caught by this very sweep.
  {
    const float scales[] = {1e-30f, 3.3e-10f, 0.125f / 127.f, 0.37f, 1.0f, 777.7f, 1e30f};
    const int centres[] = {0, 1, 2, 3, 100, 12345, 65536, 4194303, 4194304, 4194305, 8383999, SHADOW_CS_H_MAX};
    bool ok = true, tight = true;
    int caught = 0, mutants = 0;
    long long cases = 0;
    for (float s_c : scales)
      for (int c : centres)
        for (int sign : {1, -1}) {
          const int H0 = sign * c;
          float t = static_cast<float>(H0) * s_c;
          for (int u = 0; u < 4; ++u) t = std::nextafter(t, -std::numeric_limits<float>::infinity());
          for (int u = -4; u <= 4; ++u, t = std::nextafter(t, std::numeric_limits<float>::infinity())) {
            const int lo = std::max(H0 - 48, -SHADOW_CS_H_MAX), hi = std::min(H0 + 48, SHADOW_CS_H_MAX);
            const int near = sweep(t, s_c, lo, hi, 1, 0), far = sweep(t, s_c, -SHADOW_CS_H_MAX, SHADOW_CS_H_MAX, 4099, 0);
            ++cases;
            if (near < 0 || far < 0) { ok = false; std::printf("  missed: t1q %a s_c %a H0 %d\n", t, s_c, H0); }
            if (near > 6) { tight = false; std::printf("  loose: t1q %a s_c %a H0 %d: %d flagged beyond the logged\n", t, s_c, H0, near); }
            if (H0 > -SHADOW_CS_H_MAX + 64 && H0 < SHADOW_CS_H_MAX - 64) { ++mutants; if (sweep(t, s_c, lo, hi, 1, 8) < 0) ++caught; }
          }
        }
    expect(ok && cases == 7 * 12 * 2 * 9, "bits-domain bar: every logged H is flagged (positive, negative, zero bars; both ends of H and s_c)");
    expect(tight, "bits-domain bar: at most 6 flagged values below the first logged one");
    expect(mutants > 1000 && caught == mutants, "self-check: a bar 8 steps of H too high is caught by the same sweep, every time");
    bool special = true;
    for (float s_c : scales) {
      const float inf = std::numeric_limits<float>::infinity();
      for (float t : {0.f, -0.f, 1e-38f, -1e-38f, 1e-45f, -1e-45f, 3e38f, -3e38f, inf, -inf})
        if (sweep(t, s_c, -SHADOW_CS_H_MAX, SHADOW_CS_H_MAX, 997, 0) < 0 || sweep(t, s_c, -64, 64, 1, 0) < 0) { special = false; std::printf("  missed: t1q %a s_c %a\n", t, s_c); }
      // +inf bar for an unreachable t1q, "flag everything" for -inf and NaN (NaN logs nothing: any flag is conservative)
      if (!(shadow_cs_bits_bar(inf, s_c) == inf)) special = false;
      for (float t : {-inf, std::numeric_limits<float>::quiet_NaN()})
        if (!(acc_as_float(-SHADOW_CS_H_MAX) >= shadow_cs_bits_bar(t, s_c))) special = false;
    }
    expect(special, "bits-domain bar: zero, subnormal, huge, infinite and NaN t1q");
    // the order the kernel relies on: one pattern per H, ascending, across H = 0 and the binade edge
    bool mono = true;
    for (int H : {-SHADOW_CS_H_MAX, -4194305, -4194304, -4194303, -2, -1, 0, 1, 4194303, 4194304, SHADOW_CS_H_MAX - 1})
      if (!(acc_as_float(H) < acc_as_float(H + 1))) mono = false;
    expect(mono && acc_as_float(-1) == 8388607.5f && acc_as_float(1) == 8388609.f, "biased accumulators order as H does (negative H at half spacing)");
  }
  if (fails) { std::printf("%d FAILED\n", fails); return 1; }
  std::printf("OK\n");
  return 0;
}
