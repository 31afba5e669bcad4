// parts_worklist.h -- the host-side work list of the probe path (nvdb_partitions.cpp describes it; every pass of the probe search,
// the partition range scan, the probe search for any k and the masked flat bootstrap is built here): the probe table's
// de-duplication, the counting sort by partition, groups, segments, classes and candidate slots, and the layout of the image the
// kernels read.  Plain C++ with no HIP and no context in it: the sanitizer build of tests/parts_worklist_check.cpp compiles the
// code the library runs.  A function that can fail returns the reason (nullptr: fine); the caller names the call and the status.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace nvdbhip {

constexpr uint32_t PART_WAVES = 8;             // waves per workgroup (two per SIMD: one hides the other's LDS latency)
constexpr uint32_t PART_QW_MAX = 4;            // queries per wave -> groups of at most PART_WAVES * 4 queries
constexpr uint32_t PART_SEG_ROWS = 2048;       // a partition is cut into segments of at most this many rows

// one workgroup's work; qoff indexes qidx[], doff indexes dst[] (both: one entry per query of the group)
struct PartItem { uint32_t row_lo, row_hi, qoff, doff, nqg, pad; };

// host scratch of the list builder, reused across calls.  After pw_probes: uniq / ucount.  After pw_worklist: qidx (per probed
// partition, the ascending queries that probe it), dst (per item and query of its group, the first candidate slot), cbeg (nq + 1:
// the queries' blocks of the candidate buffer) and items by class of group size (0: <= PART_WAVES queries, 1: <= 2 * PART_WAVES, 2: more).
struct PartScratch {
  std::vector<uint32_t> uniq, ucount, pcount, pstart, cursor, qidx, dst, cbeg, psum;
  std::vector<PartItem> items[3];
};

struct PartList { uint32_t npairs = 0; uint64_t total = 0, rows_read = 0; size_t nitems = 0; };

// The probe table of a call ([nq][nprobe]), checked and de-duplicated into uniq / ucount: 0xFFFFFFFF slots dropped, a partition
// named twice counted once.  rows_union (optional, nq entries): the rows of every query's probed union.
inline const char* pw_probes(PartScratch& ps, const uint64_t* off, uint32_t nparts, uint32_t nq, const uint32_t* probe, uint32_t nprobe, uint64_t* rows_union) {
  ps.uniq.resize(static_cast<size_t>(nq) * nprobe);
  ps.ucount.assign(nq, 0);
  for (uint32_t q = 0; q < nq; ++q) {
    uint32_t* u = ps.uniq.data() + static_cast<size_t>(q) * nprobe;
    uint32_t m = 0;
    for (uint32_t j = 0; j < nprobe; ++j) {
      const uint32_t p = probe[static_cast<size_t>(q) * nprobe + j];
      if (p == 0xFFFFFFFFu) continue;
      if (p >= nparts) return "probe entry names a partition >= nparts";
      u[m++] = p;
    }
    std::sort(u, u + m);
    m = static_cast<uint32_t>(std::unique(u, u + m) - u);
    ps.ucount[q] = m;
    if (rows_union) {
      uint64_t rows = 0;
      for (uint32_t j = 0; j < m; ++j) rows += off[u[j] + 1] - off[u[j]];
      rows_union[q] = rows;
    }
  }
  return nullptr;
}

// The work list of queries q0 .. q0 + nq of that table (numbered from 0 inside the list): the counting sort by partition, query
// groups of at most qg_max queries, segments of at most PART_SEG_ROWS rows, classes by group size.  slot_cap: an (item, query)
// gets min(slot_cap, segment rows) candidate slots (the top-k search: k; the range scan: no cap).
inline const char* pw_worklist(PartScratch& ps, const uint64_t* off, uint32_t nparts, uint32_t q0, uint32_t nq, uint32_t nprobe, uint32_t qg_max, uint32_t slot_cap,
                               PartList& wl) {
  // 1. the de-duplicated probes of queries q0 .. q0 + nq (pw_probes): per-partition query counts
  const uint32_t* uniq = ps.uniq.data() + static_cast<size_t>(q0) * nprobe;
  const uint32_t* ucount = ps.ucount.data() + q0;
  ps.pcount.assign(nparts, 0);
  for (uint32_t q = 0; q < nq; ++q)
    for (uint32_t j = 0; j < ucount[q]; ++j) ++ps.pcount[uniq[static_cast<size_t>(q) * nprobe + j]];
  // 2. counting sort: the queries of every partition, ascending
  ps.pstart.assign(nparts + 1, 0);
  for (uint32_t p = 0; p < nparts; ++p) ps.pstart[p + 1] = ps.pstart[p] + ps.pcount[p];
  const uint32_t npairs = ps.pstart[nparts];
  ps.qidx.resize(npairs);
  ps.cursor.assign(ps.pstart.begin(), ps.pstart.end() - 1);
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t* u = uniq + static_cast<size_t>(q) * nprobe;
    for (uint32_t j = 0; j < ucount[q]; ++j) ps.qidx[ps.cursor[u[j]]++] = q;
  }
  // 3. candidate slots a probe of partition p costs a query; the queries' blocks
  auto nseg_of = [](uint64_t size) { return static_cast<uint32_t>((size + PART_SEG_ROWS - 1) / PART_SEG_ROWS); };
  ps.psum.assign(nparts, 0);
  for (uint32_t p = 0; p < nparts; ++p) {
    const uint64_t size = off[p + 1] - off[p];
    if (!ps.pcount[p] || !size) continue;
    const uint32_t nseg = nseg_of(size);
    uint64_t sum = 0;
    for (uint32_t sg = 0; sg < nseg; ++sg) sum += std::min<uint64_t>(slot_cap, size * (sg + 1) / nseg - size * sg / nseg);
    ps.psum[p] = static_cast<uint32_t>(sum);
  }
  ps.cbeg.assign(nq + 1, 0);
  uint64_t total = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t* u = uniq + static_cast<size_t>(q) * nprobe;
    for (uint32_t j = 0; j < ucount[q]; ++j) total += ps.psum[u[j]];
    if (total >= 0xFFFFFFFFull) return "more than 2^32 candidate slots in one call (split the batch)";
    ps.cbeg[q + 1] = static_cast<uint32_t>(total);
  }
  // 4. work items, by class of group size
  for (auto& v : ps.items) v.clear();
  ps.dst.clear();
  ps.cursor.assign(ps.cbeg.begin(), ps.cbeg.end() - 1);
  uint64_t rows_read = 0;
  for (uint32_t p = 0; p < nparts; ++p) {
    const uint64_t size = off[p + 1] - off[p];
    const uint32_t cnt = ps.pcount[p];
    if (!cnt || !size) continue;
    const uint32_t nseg = nseg_of(size);
    for (uint32_t g0 = 0; g0 < cnt; g0 += qg_max) {
      const uint32_t nqg = std::min(qg_max, cnt - g0);
      const int cl = nqg <= PART_WAVES ? 0 : (nqg <= 2 * PART_WAVES ? 1 : 2);
      for (uint32_t sg = 0; sg < nseg; ++sg) {
        const uint32_t lo = static_cast<uint32_t>(off[p] + size * sg / nseg), hi = static_cast<uint32_t>(off[p] + size * (sg + 1) / nseg);
        ps.items[cl].push_back(PartItem{lo, hi, ps.pstart[p] + g0, static_cast<uint32_t>(ps.dst.size()), nqg, 0u});
        const uint32_t slot = std::min<uint32_t>(slot_cap, hi - lo);
        for (uint32_t g = 0; g < nqg; ++g) { uint32_t& cur = ps.cursor[ps.qidx[ps.pstart[p] + g0 + g]]; ps.dst.push_back(cur); cur += slot; }
        rows_read += hi - lo;
      }
    }
  }
  wl.npairs = npairs;
  wl.total = total;
  wl.rows_read = rows_read;
  wl.nitems = ps.items[0].size() + ps.items[1].size() + ps.items[2].size();
  return nullptr;
}

// The image of a work list, in 32-bit words: [items (classes 2, 1, 0) | qidx | dst | cbeg | masked: mask_of | extra].  Every field
// is the first word of its part; a part ends where the next begins, the image at `words`.
struct PartLayout { size_t items = 0, qidx = 0, dst = 0, cbeg = 0, mask_of = 0, extra = 0, words = 0; };

inline PartLayout pw_layout(const PartScratch& ps, const PartList& wl, uint32_t nq, bool masked, uint32_t extra_words) {
  PartLayout l;
  l.qidx = wl.nitems * (sizeof(PartItem) / 4);
  l.dst = l.qidx + wl.npairs;
  l.cbeg = l.dst + ps.dst.size();
  l.mask_of = l.cbeg + nq + 1;
  l.extra = l.mask_of + (masked ? nq : 0);
  l.words = l.extra + extra_words;
  return l;
}

// ... written to w[0 .. l.words).  mask_of (nq entries) is read in a masked layout only; nullptr there: plane 0 for every query
inline void pw_write_image(const PartScratch& ps, const PartLayout& l, const uint32_t* mask_of, const uint32_t* extra, uint32_t* w) {
  uint32_t* it = w + l.items;
  for (int cl = 2; cl >= 0; --cl) {                                     // the widest groups first: the longest items start early
    if (!ps.items[cl].empty()) std::memcpy(it, ps.items[cl].data(), ps.items[cl].size() * sizeof(PartItem));
    it += ps.items[cl].size() * (sizeof(PartItem) / 4);
  }
  if (l.dst > l.qidx) std::memcpy(w + l.qidx, ps.qidx.data(), (l.dst - l.qidx) * 4);
  if (l.cbeg > l.dst) std::memcpy(w + l.dst, ps.dst.data(), (l.cbeg - l.dst) * 4);
  std::memcpy(w + l.cbeg, ps.cbeg.data(), (l.mask_of - l.cbeg) * 4);
  for (size_t q = 0; q < l.extra - l.mask_of; ++q) w[l.mask_of + q] = mask_of ? mask_of[q] : 0u;
  if (l.words > l.extra) std::memcpy(w + l.extra, extra, (l.words - l.extra) * 4);
}

}  // namespace nvdbhip
