// san_flat_large_k_sort_main.cc -- TEST INFRASTRUCTURE (tests/test_flat_large_k_sort_host_cpu.py): a stand-alone program over
// csrc/flat_large_k_host.hpp (no HIP call in it) and include/vk_index.h, built with -fsanitize=address,undefined.  The pass
// count of the device sort at the edges of its tile, the chunk plan with the sort's buffers counted, the new struct's size.
#include <stdio.h>

#include <random>

#include "flat_large_k_host.hpp"
#include "vk_index.h"

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "FAILED: %s (line %d)\n", #cond, __LINE__); ++g_bad; } } while (0)

int main() {
  const uint64_t T = vk::kLargeKSortTile;
  CHECK(T == 4096 && vk::large_k_sort_passes(1) == 0 && vk::large_k_sort_passes(T) == 0 && vk::large_k_sort_passes(T + 1) == 1);
  CHECK(vk::large_k_sort_passes(2 * T) == 1 && vk::large_k_sort_passes(2 * T + 1) == 2 && vk::large_k_sort_passes(0xFFFFFFFFull) == 20);
  for (uint64_t cap = 1; cap < 70 * T; cap += 997) {   // runs of T << passes span cap, runs of half that do not
    const uint32_t p = vk::large_k_sort_passes(cap);
    CHECK((T << p) >= cap && (p == 0 || (T << (p - 1)) < cap));
  }
  CHECK(sizeof(vk_flat_large_k_sort_stats) == 64 && sizeof(vk_flat_large_k_stats) == 56);
  std::mt19937_64 rng(16);
  auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
  for (int i = 0; i < 4000; ++i) {
    const uint64_t nq = pick(0, i % 5 ? 64 : 200000), count = pick(0, i % 3 ? 70000 : 20000000), k = pick(1025, 100000);
    const uint64_t per_q = ((count + 63) & ~63ull) * 4 + (2 * vk::large_k_cap(k) + k) * 12;
    const uint64_t budget = i % 2 ? pick(0, 40) * per_q + pick(0, per_q) : pick(0, 1ull << 36);
    const vk::LargeKPlan p = vk::large_k_plan_sorted(nq, count, k, budget), plain = vk::large_k_plan(nq, count, k, budget);
    CHECK(p.fits == plain.fits && p.ld == plain.ld && p.chunk_q <= plain.chunk_q);   // the same door, never more queries per chunk
    if (!p.fits) continue;
    CHECK(p.chunk_q >= 1 && p.chunk_q <= nq && p.chunk_q <= vk::kLargeKMaxChunkQueries && (p.chunk_q < 8 || p.chunk_q % 8 == 0));
    CHECK((p.chunks - 1) * p.chunk_q < nq && p.chunks * p.chunk_q >= nq);
    CHECK(p.chunk_q == 1 || p.chunk_q * per_q <= budget);   // the budget is honoured, but never below one query
  }
  printf("bad=%d\n", g_bad);
  return g_bad ? 1 : 0;
}
