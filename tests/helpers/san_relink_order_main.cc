// The order of hnsw_relink_kernel's counting sort (csrc/hnsw_relink_order.hpp) under -fsanitize=address,undefined, on the
// host: for every case the ranks relink_rank gives to i = 0..total-1 must be a permutation of 0..total-1, the entries in
// rank order must ascend by (key, id, position) with every NaN behind every number, and where a case holds no NaN and no
// repeated (distance, id) pair the order must be the one of `d < d' || (d == d' && id < id')` -- what the kernel ranked by
// before.  Usage: prog <seed> <rounds>; prints cases=<n> bad=<mismatches>.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "hnsw_relink_order.hpp"

using namespace vk;

namespace {

float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}

uint64_t g_cases = 0, g_bad = 0, g_plain = 0;

void fail(const char *what, const char *why, size_t total) {
  ++g_bad;
  if (g_bad <= 20) printf("BAD %s (total=%zu): %s\n", what, total, why);
}

void check(const char *what, const std::vector<float> &d, const std::vector<uint32_t> &id) {
  ++g_cases;
  const uint32_t total = (uint32_t)d.size();
  std::vector<float> d_exact(d);          // exactly total elements each: a read past the end is a sanitizer report
  std::vector<uint32_t> id_exact(id);
  std::vector<int64_t> at(total, -1);     // at[rank] = i
  for (uint32_t i = 0; i < total; ++i) {
    const uint32_t r = relink_rank(d_exact.data(), id_exact.data(), total, i);
    if (r >= total) return fail(what, "rank out of range", total);
    if (at[r] != -1) return fail(what, "two entries share a rank", total);
    at[r] = i;
  }
  for (uint32_t r = 0; r < total; ++r)
    if (at[r] < 0) return fail(what, "a slot is never written", total);
  bool nan = false, plain = true;
  std::set<std::pair<uint32_t, uint32_t>> seen;   // (distance bits with -0 as +0, id)
  for (uint32_t r = 0; r < total; ++r) {
    const float f = d[at[r]];
    if (f != f) nan = true;
    else if (nan) return fail(what, "a number behind a NaN", total);
    uint32_t u;
    memcpy(&u, &f, 4);
    if (u == 0x80000000u) u = 0;
    if (f != f || !seen.insert({u, id[at[r]]}).second) plain = false;
    if (r == 0) continue;
    const uint32_t a = (uint32_t)at[r - 1], b = (uint32_t)at[r];
    if (!relink_before(relink_order_key(d[a]), id[a], a, relink_order_key(d[b]), id[b], b)) return fail(what, "not ascending", total);
    if (d[a] == d[a] && d[b] == d[b] && d[a] > d[b]) return fail(what, "float order broken", total);
  }
  if (!plain) return;
  ++g_plain;
  // today's inputs: the order of the comparison the kernel used before
  std::vector<uint32_t> want(total);
  for (uint32_t i = 0; i < total; ++i) want[i] = i;
  std::sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return d[a] < d[b] || (d[a] == d[b] && id[a] < id[b]); });
  for (uint32_t r = 0; r < total; ++r)
    if (want[r] != (uint32_t)at[r]) return fail(what, "differs from the (distance, id) order", total);
}

}  // namespace

int main(int argc, char **argv) {
  const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const int rounds = argc > 2 ? atoi(argv[2]) : 50;
  std::mt19937_64 rng(seed);
  const float inf = INFINITY, qnan = from_bits(0x7FC00000u), neg_nan = from_bits(0xFFC00001u), snan = from_bits(0x7F800001u);
  const std::vector<uint32_t> totals = {1, 2, 3, 17, 63, 64, 65, 255, 256};

  // the key itself: order, +-0, NaN last
  const float ladder[] = {-inf, -3.0e38f, -1.0f, from_bits(0x80000001u), -0.0f, from_bits(0x00000001u), 1.0f, 3.0e38f, inf};
  for (size_t i = 0; i + 1 < sizeof(ladder) / sizeof(ladder[0]); ++i)
    if (!(relink_order_key(ladder[i]) < relink_order_key(ladder[i + 1]))) fail("key", "ladder not ascending", i);
  if (relink_order_key(-0.0f) != relink_order_key(0.0f)) fail("key", "-0 and +0 differ", 0);
  for (float n : {qnan, neg_nan, snan, from_bits(0xFFFFFFFFu)})
    if (relink_order_key(n) != 0xFFFFFFFFu || !(relink_order_key(inf) < relink_order_key(n))) fail("key", "NaN not last", 0);

  for (int round = 0; round < rounds; ++round) {
    for (uint32_t total : totals) {
      std::vector<float> d(total);
      std::vector<uint32_t> id(total);
      auto distinct_ids = [&] {
        for (uint32_t i = 0; i < total; ++i) id[i] = i * 7 + 3;
        std::shuffle(id.begin(), id.end(), rng);
      };
      std::normal_distribution<float> normal;
      // random distances, distinct ids
      distinct_ids();
      for (float &f : d) f = normal(rng);
      check("random", d, id);
      // few distinct distances: ties everywhere, decided by id
      for (float &f : d) f = (float)(int)(rng() % 3) - 1.0f;
      check("ties", d, id);
      // all equal
      for (float &f : d) f = 0.25f;
      check("all equal", d, id);
      // all NaN, of both signs
      for (uint32_t i = 0; i < total; ++i) d[i] = (i & 1) ? neg_nan : qnan;
      check("all NaN", d, id);
      // NaN mixed in
      for (float &f : d) f = (rng() % 4 == 0) ? ((rng() & 1) ? qnan : neg_nan) : normal(rng);
      check("NaN mixed in", d, id);
      // +-0 among small numbers
      for (float &f : d) { const int c = (int)(rng() % 4); f = c == 0 ? 0.0f : c == 1 ? -0.0f : c == 2 ? -1.0e-30f : 1.0e-30f; }
      check("+-0", d, id);
      // +-inf
      for (float &f : d) { const int c = (int)(rng() % 4); f = c == 0 ? inf : c == 1 ? -inf : normal(rng); }
      check("+-inf", d, id);
      // duplicated (distance, id) pairs: ids drawn from a few, distances from a few
      for (uint32_t i = 0; i < total; ++i) { id[i] = (uint32_t)(rng() % 4); d[i] = (float)(int)(rng() % 2); }
      check("duplicates", d, id);
      // everything one (distance, id) pair; and one NaN pair
      for (uint32_t i = 0; i < total; ++i) { id[i] = 9; d[i] = 1.5f; }
      check("one pair", d, id);
      for (float &f : d) f = qnan;
      check("one NaN pair", d, id);
      // the whole bit space
      distinct_ids();
      for (float &f : d) f = from_bits((uint32_t)rng());
      check("bits", d, id);
    }
  }
  printf("cases=%llu plain=%llu bad=%llu\n", (unsigned long long)g_cases, (unsigned long long)g_plain, (unsigned long long)g_bad);
  return g_bad ? 1 : 0;
}
