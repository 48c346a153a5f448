// san_flat_large_k_main.cc -- TEST INFRASTRUCTURE (tests/test_flat_large_k_host_cpu.py): a stand-alone program over
// csrc/flat_large_k_host.hpp, built with -fsanitize=address,undefined.  The header makes no HIP call.
//
//   plans   random (nq, count, k, budget): the chunk plan holds its contract -- ld >= count and a multiple of 64; the path is
//           taken exactly when one row of distances fits the budget; the chunks cover every query exactly once; a chunk is never
//           empty, never beyond the grid's limit, a multiple of 8 once it reaches 8, and -- unless one query alone is already
//           beyond it -- its distances and hand-back fit the budget
//   worlds  random hand-backs with ties, +0 / -0 and short lists: large_k_finish against std::partial_sort over the full list
//           by (float compare, label); the stored distance bits are kept; nothing is written behind min(k, n)
// Usage: san_flat_large_k <seed> <plans> <worlds>; prints "plans=.. worlds=.. short=.. zeros=.. bad=..".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "flat_large_k_host.hpp"

namespace {

int g_bad = 0;
#define CHECK(cond, what)                                        \
  do {                                                           \
    if (!(cond)) {                                               \
      if (g_bad < 20) fprintf(stderr, "FAILED: %s (line %d)\n", what, __LINE__); \
      ++g_bad;                                                   \
    }                                                            \
  } while (0)

void check_plan(uint64_t nq, uint64_t count, uint64_t k, uint64_t budget) {
  const vk::LargeKPlan p = vk::large_k_plan(nq, count, k, budget);
  CHECK(p.ld >= count && p.ld % 64 == 0 && p.ld < count + 64, "ld");
  CHECK(p.fits == (nq != 0 && count != 0 && p.ld * 4 <= budget), "fits");
  if (!p.fits) {
    CHECK(p.chunk_q == 0 && p.chunks == 0, "no plan when it does not fit");
    return;
  }
  CHECK(p.chunk_q >= 1 && p.chunk_q <= nq && p.chunk_q <= vk::kLargeKMaxChunkQueries, "chunk size");
  CHECK(p.chunk_q < 8 || p.chunk_q % 8 == 0, "multiple of 8");
  CHECK((p.chunks - 1) * p.chunk_q < nq && p.chunks * p.chunk_q >= nq, "the chunks cover the queries once");
  const uint64_t per_q = p.ld * 4 + vk::large_k_cap(k) * vk::kLargeKSlotBytes;
  CHECK(p.chunk_q == 1 || p.chunk_q * per_q <= budget, "a chunk of several queries fits the budget");
  // not needlessly small: one more group of queries would not have fitted (or there are no more queries, or the grid's limit)
  uint64_t most = nq < vk::kLargeKMaxChunkQueries ? nq : vk::kLargeKMaxChunkQueries;
  while (most > 1 && most * per_q > budget) --most;   // (the largest chunk the limits admit, found the slow way)
  CHECK(p.chunk_q <= most && (most < 8 ? p.chunk_q == most : p.chunk_q + 8 > most), "chunk not needlessly small");
}

struct Entry { float d; uint32_t bits; uint64_t label; };

}  // namespace

int main(int argc, char **argv) {
  const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const uint64_t plans = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1000;
  const uint64_t worlds = argc > 3 ? strtoull(argv[3], nullptr, 10) : 1000;
  std::mt19937_64 rng(seed);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };

  CHECK(vk::large_k_cap(1025) == 2049 && vk::large_k_cap(4096) == 5120 && vk::large_k_cap(100000) == 125000, "cap");
  for (uint64_t i = 0; i < plans; ++i) {
    const uint64_t nq = i % 17 == 0 ? pick(0, 2) : i % 5 == 0 ? pick(1, 200000) : pick(1, 64);
    const uint64_t count = i % 19 == 0 ? pick(0, 3) : i % 3 == 0 ? pick(1, 20000000) : pick(1, 70000);
    const uint64_t k = pick(1025, 100000);
    const uint64_t ld4 = ((count + 63) & ~63ull) * 4;
    uint64_t budget;
    switch (i % 4) {
      case 0: budget = pick(0, 2 * ld4 + 8); break;                           // around one row of distances
      case 1: budget = ld4 + pick(0, 40) * (ld4 + vk::large_k_cap(k) * 12); break;   // a few queries
      case 2: budget = 1ull << 30; break;
      default: budget = pick(0, 1ull << 36); break;
    }
    check_plan(nq, count, k, budget);
    check_plan(nq, count, k, ld4);          // exactly one row of distances
    if (ld4) check_plan(nq, count, k, ld4 - 1);
  }

  uint64_t n_short = 0, n_zeros = 0;
  for (uint64_t w = 0; w < worlds; ++w) {
    const uint64_t k = pick(1, 300);
    const uint64_t n = w % 7 == 0 ? pick(0, k) : pick(k, k + 400);   // short lists, and lists with a tie group behind k
    const uint64_t distinct = pick(1, 12);                           // a handful of distances: ties everywhere
    std::vector<uint32_t> bits(n);
    std::vector<uint64_t> labels(n);
    std::vector<Entry> all(n);
    for (uint64_t i = 0; i < n; ++i) {
      float d;
      const uint64_t c = rng() % (distinct + 3);
      if (c == distinct) d = 0.0f;
      else if (c == distinct + 1) d = -0.0f;
      else if (c == distinct + 2) d = INFINITY;
      else d = (float)((int64_t)c - 5) * 0.25f;
      memcpy(&bits[i], &d, 4);
      labels[i] = (rng() << 20) | i;                                 // distinct labels
      all[i] = Entry{d, bits[i], labels[i]};
      n_zeros += d == 0.0f;
    }
    n_short += n < k;
    const uint64_t m = std::min(k, n);
    std::partial_sort(all.begin(), all.begin() + m, all.end(),
                      [](const Entry &a, const Entry &b) { return a.d < b.d || (a.d == b.d && a.label < b.label); });
    std::vector<float> od(k + 2, 12345.0f);
    std::vector<uint64_t> ol(k + 2, 777);
    const uint64_t got = vk::large_k_finish(bits.data(), labels.data(), n, k, od.data(), ol.data());
    CHECK(got == m, "min(k, n) entries");
    for (uint64_t i = 0; i < m && i < got; ++i) {
      uint32_t b;
      memcpy(&b, &od[i], 4);
      CHECK(ol[i] == all[i].label && b == all[i].bits, "entry");
    }
    for (uint64_t i = m; i < k + 2; ++i) CHECK(od[i] == 12345.0f && ol[i] == 777, "nothing behind the answer");
  }
  printf("plans=%llu worlds=%llu short=%llu zeros=%llu bad=%d\n", (unsigned long long)plans, (unsigned long long)worlds,
         (unsigned long long)n_short, (unsigned long long)n_zeros, g_bad);
  return g_bad ? 1 : 0;
}
