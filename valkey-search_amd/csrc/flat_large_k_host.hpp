// flat_large_k_host.hpp -- the host half of the one-pass FLAT search for k > 1024 (flat_large_k.hip, FlatIndex::search_large_k):
// the sizes both halves agree on, the chunk plan and the finish rule over a hand-back.  No HIP in here: the rules are tested
// by a plain host program under sanitizers (tests/helpers/san_flat_large_k_main.cc).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace vk {

// Entries the device hands back per query: the k-th key's tie group may reach past k, so the list has room for `slack` more.
// A float distance takes 2^32 values and real data ties at the k-th place by a handful of entries at most; what does tie by
// the thousand is an index of duplicates, and that query goes to the paged path (which orders a tie group by label in the
// scan).  The slack is paid in hand-back bytes (12 per slot, downloaded whole), so it follows k at a quarter and never
// drops below one page of the paged path.
inline uint64_t large_k_slack(uint64_t k) { return std::max<uint64_t>(1024, k / 4); }
inline uint64_t large_k_cap(uint64_t k) { return k + large_k_slack(k); }

// bytes one slot of the hand-back takes: distance bits + label
constexpr uint64_t kLargeKSlotBytes = 12;
// queries one chunk may hold at most: the y dimension of the select and emit grids
constexpr uint64_t kLargeKMaxChunkQueries = 65535;

// The chunk plan.  ld = floats between two queries' rows of the distance buffer (count rounded up to 64 floats, so every row
// starts on a 256-byte boundary).  The path is taken only when ONE query's row of distances fits the budget (fits); a chunk
// then holds as many queries as the budget pays for, a query costing its row of distances plus its hand-back list -- at least
// one, at most nq and the grid's limit, and a multiple of 8 once it reaches 8 (the distance kernel serves up to 8 queries per
// row tile: a chunk of 15 would read the table for 8 + 7).
struct LargeKPlan {
  bool fits = false;
  uint64_t ld = 0;        // floats
  uint64_t chunk_q = 0;   // queries per chunk (the last chunk may hold fewer)
  uint64_t chunks = 0;
};
inline LargeKPlan large_k_plan(uint64_t nq, uint64_t count, uint64_t k, uint64_t budget_bytes) {
  LargeKPlan p;
  p.ld = (count + 63) & ~(uint64_t)63;
  if (nq == 0 || count == 0 || p.ld * 4 > budget_bytes) return p;
  p.fits = true;
  const uint64_t per_q = p.ld * 4 + large_k_cap(k) * kLargeKSlotBytes;
  uint64_t c = std::max<uint64_t>(1, budget_bytes / per_q);
  c = std::min(c, std::min(nq, kLargeKMaxChunkQueries));
  if (c >= 8) c &= ~(uint64_t)7;
  p.chunk_q = c;
  p.chunks = (nq + c - 1) / c;
  return p;
}

// order-preserving u32 of a non-NaN float, -0 and +0 sharing a key: merge_key of flat_scan.hip
inline uint32_t large_k_key(uint32_t bits) {
  if (bits == 0x80000000u) bits = 0;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// The finish rule: the hand-back's n entries (distance bits, label) in any order -> the first min(k, n) of them by (float
// compare with -0 == +0, then label), the stored bits kept.  No NaN is ever handed back.  Returns the number written.
inline uint64_t large_k_finish(const uint32_t *bits, const uint64_t *labels, uint64_t n, uint64_t k, float *out_dist, uint64_t *out_label) {
  struct E { uint32_t key, bits; uint64_t label; };
  std::vector<E> v(n);
  for (uint64_t i = 0; i < n; ++i) v[i] = E{large_k_key(bits[i]), bits[i], labels[i]};
  std::sort(v.begin(), v.end(), [](const E &a, const E &b) { return a.key != b.key ? a.key < b.key : a.label < b.label; });
  const uint64_t m = std::min(k, n);
  for (uint64_t i = 0; i < m; ++i) {
    memcpy(out_dist + i, &v[i].bits, 4);
    out_label[i] = v[i].label;
  }
  return m;
}

}  // namespace vk
