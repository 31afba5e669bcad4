// parts_anyk_plan_check.cpp -- the host-side arithmetic of the probe search for any k (nano-vectordb_amd/csrc/parts_anyk_plan.h, the
// code the library's entry points run) against naive loops, with exactly sized heap buffers: built with
// -fsanitize=address,undefined by tests/test_cabi_parts_anyk_cpu.py, a read past a block list or a write past a plan's arrays
// stops the program.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "parts_anyk_plan.h"

using namespace nvdbhip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// the slab of (k, len): a power of two, >= 2, >= min(k, len), the smallest such; long beyond PA_LDS_KEYS
static void check_slab(uint32_t k, uint32_t len) {
  const uint64_t want = k < len ? k : len, K2 = pa_slab_len(k, len);
  if (want == 0) CHECK(K2 == 0);
  else {
    CHECK(K2 >= 2 && K2 >= want && (K2 & (K2 - 1)) == 0);
    CHECK(K2 == 2 || K2 / 2 < want);
    CHECK(K2 == rp_slab_len(want));
  }
  CHECK(pa_slab_is_long(K2) == (want > PA_LDS_KEYS));
  std::printf("slab k=%u len=%u checked\n", k, len);
}

// a sub-batch's plan against the definitions
static void check_plan(const std::vector<uint64_t>& blocks, uint32_t k) {
  const uint32_t b = static_cast<uint32_t>(blocks.size());
  uint64_t* block = new uint64_t[b];
  for (uint32_t i = 0; i < b; ++i) block[i] = blocks[i];
  PaPlan p;
  CHECK(pa_plan(block, b, k, p));
  CHECK(p.slab_off.size() == static_cast<size_t>(b) * 2);
  uint64_t widest = 1, lds = 2, keys = 0;
  uint32_t nlong = 0;
  for (uint32_t i = 0; i < b; ++i) {
    const uint64_t K2 = pa_slab_len(k, static_cast<uint32_t>(block[i]));
    widest = std::max<uint64_t>(widest, std::min<uint64_t>(k, block[i]));
    if (pa_slab_is_long(K2)) { ++nlong; keys += K2; CHECK(p.slab_off[2 * i] != PA_NO_SLAB || p.slab_off[2 * i + 1] != PA_NO_SLAB); }
    else { lds = std::max(lds, K2); CHECK(p.slab_off[2 * i] == PA_NO_SLAB && p.slab_off[2 * i + 1] == PA_NO_SLAB); }
  }
  CHECK(p.out_k == widest && p.lds_keys == lds && p.lds_keys <= PA_LDS_KEYS && p.slab_keys == keys && p.longs.size() == nlong);
  // the long lists: ordered by length, then by query; slabs adjacent, disjoint, inside slab_keys; the per-query offsets agree
  uint64_t at = 0;
  for (size_t i = 0; i < p.longs.size(); ++i) {
    const PaLong& l = p.longs[i];
    const uint64_t off = (static_cast<uint64_t>(l.off_hi) << 32) | l.off_lo;
    CHECK(l.q < b && l.K2 == pa_slab_len(k, static_cast<uint32_t>(block[l.q])) && off == at);
    CHECK(p.slab_off[2 * l.q] == l.off_lo && p.slab_off[2 * l.q + 1] == l.off_hi);
    if (i) CHECK(p.longs[i - 1].K2 < l.K2 || (p.longs[i - 1].K2 == l.K2 && p.longs[i - 1].q < l.q));
    at += l.K2;
  }
  CHECK(at == p.slab_keys);
  delete[] block;
  std::printf("plan b=%u k=%u: out_k %u, lds_keys %u, %u long lists, %llu keys checked\n", b, k, p.out_k, p.lds_keys, nlong,
              static_cast<unsigned long long>(p.slab_keys));
}

// the cut against its three bounds
static void check_cut(const std::vector<uint64_t>& blocks, uint32_t k, uint64_t budget, const char* what) {
  const uint32_t nq = static_cast<uint32_t>(blocks.size());
  uint64_t* block = new uint64_t[nq];
  for (uint32_t i = 0; i < nq; ++i) block[i] = blocks[i];
  uint32_t q0 = 0, cuts = 0;
  while (q0 < nq) {
    const uint32_t q1 = pa_cut(block, nq, q0, k, budget);
    CHECK(q1 > q0 && q1 <= nq);
    if (q1 == q0) break;
    uint64_t sum = 0, slabs = 0, widest = 0;
    for (uint32_t q = q0; q < q1; ++q) {
      sum += block[q];
      const uint64_t K2 = pa_slab_len(k, static_cast<uint32_t>(block[q]));
      if (pa_slab_is_long(K2)) slabs += K2;
      widest = std::max<uint64_t>(widest, std::min<uint64_t>(k, block[q]));
    }
    CHECK(sum < RP_MAX_ENTRIES);
    if (q1 - q0 > 1) CHECK(sum <= budget && slabs <= budget && widest * (q1 - q0) <= budget);
    if (q1 < nq) {                                  // ... and the next query would have broken one of them
      const uint64_t K2 = pa_slab_len(k, static_cast<uint32_t>(std::min<uint64_t>(block[q1], 0xFFFFFFFFull)));
      const uint64_t w = std::max<uint64_t>(widest, std::min<uint64_t>(k, block[q1]));
      CHECK(block[q1] >= RP_MAX_ENTRIES - sum || sum + block[q1] > budget || slabs + (pa_slab_is_long(K2) ? K2 : 0) > budget || w * (q1 - q0 + 1) > budget);
    }
    q0 = q1;
    ++cuts;
  }
  CHECK(pa_cut(block, nq, nq, k, budget) == nq);
  delete[] block;
  std::printf("cut %s: %u sub-batches checked\n", what, cuts);
}

int main() {
  for (uint32_t k : {1u, 65u, 100u, 8192u, 8193u, 30001u, 0xFFFFFFFFu})
    for (uint32_t len : {0u, 1u, 64u, 8192u, 8193u, 20000u, 0xFFFFFFFEu}) check_slab(k, len);
  check_plan({0, 1, 63, 20000, 128, 9000, 20000, 16384, 16385}, 100);          // nothing long
  check_plan({0, 1, 63, 20000, 128, 9000, 20000, 16384, 16385}, 8192);
  check_plan({0, 1, 63, 20000, 128, 9000, 20000, 16384, 16385}, 8193);         // five long lists of 16384 keys
  check_plan({0, 1, 63, 20000, 128, 9000, 20000, 16384, 16385}, 30001);        // long lists of 16384 (9000, 16384) and 32768 keys (20000 twice, 16385)
  check_plan({0, 0, 0}, 100);
  check_plan({5}, 0xFFFFFFFFu);
  {                                                  // 2^32 keys in one slab: refused
    uint64_t* block = new uint64_t[1]{0xFFFFFFF0ull};
    PaPlan p;
    CHECK(!pa_plan(block, 1, 0x80000001u, p));
    CHECK(pa_plan(block, 1, 0x80000000u, p) && p.longs.size() == 1 && p.longs[0].K2 == 0x80000000u);
    delete[] block;
    std::printf("plan 2^31 results checked\n");
  }
  check_cut(std::vector<uint64_t>(70, 20000), 100, 65536, "three queries per sub-batch");
  check_cut(std::vector<uint64_t>(70, 20000), 30001, 65536, "long slabs bound it");
  check_cut(std::vector<uint64_t>(70, 20000), 100, 1, "one query per sub-batch");
  check_cut({0, 0, 5, 0, 70000, 3, 3, 3}, 65, 100, "empty blocks and one over the budget");
  check_cut(std::vector<uint64_t>(1000, 200), 150, 2000, "the output bounds it");
  check_cut({0xFFFFFFF0ull, 0x10ull, 0xFFFFFFFEull, 1, 1}, 100, ~0ull, "2^32 entries");
  {
    uint64_t* block = new uint64_t[2]{0xFFFFFFFFull, 1};
    CHECK(pa_cut(block, 2, 0, 100, ~0ull) == 0);     // one query's block alone reaches the limit: no progress
    CHECK(pa_cut(block, 2, 1, 100, ~0ull) == 2);
    delete[] block;
    std::printf("cut no progress checked\n");
  }
  std::printf(failures ? "%d FAILED\n" : "OK\n", failures);
  return failures ? 1 : 0;
}
