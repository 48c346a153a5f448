// san_prefilter_handle_main.cc -- TEST INFRASTRUCTURE (tests/test_prefilter_handle_host_cpu.py): the host half of the exact
// kNN from a filter handle (csrc/prefilter_handle_host.hpp) under -fsanitize=address,undefined, with plain host memory.
//
// Random worlds: an ascending, duplicate-free label list spread over 1 to 8 shards, distances with few distinct values (ties
// everywhere, +-0), k in {1, 2, 10, 64, 1000}.  Per shard the plain model of the select kernel (prefilter_select_model) gives
// the hand-back over the shard's part of the list -- or the fallback mark, when more entries tie than the cap holds; the
// candidates carry their labels; handle_union + handle_finish must equal the reference's heap rule over the whole list, and
// the k smallest by (distance, label).  Run splitting: random handle tables against a plain scan.
//   usage: san_prefilter_handle_main <seed> <worlds>
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "prefilter_handle_host.hpp"

using namespace vk;

int main(int argc, char **argv) {
  const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1;
  const int worlds = argc > 2 ? atoi(argv[2]) : 1000;
  std::mt19937_64 rng(seed);
  const uint64_t ks[] = {1, 2, 10, 64, 1000};
  long bad = 0, fell = 0, answered = 0;
  for (int w = 0; w < worlds; ++w) {
    const uint64_t n = rng() % 3000, k = ks[rng() % 5], cap = prefilter_cap(k), S = 1 + rng() % 8, nq = 1 + rng() % 4;
    const int distinct = 3 + (int)(rng() % 48);
    std::vector<uint64_t> labels(n);
    uint64_t next = rng() % 5;
    for (uint64_t i = 0; i < n; ++i) { labels[i] = next; next += 1 + rng() % 7; }
    std::vector<uint32_t> shard(n);
    for (uint64_t i = 0; i < n; ++i) shard[i] = (uint32_t)(rng() % S);
    std::vector<HandleCands> parts(S);
    for (auto &p : parts) p.reset(nq, false);
    std::vector<std::vector<float>> dist(nq, std::vector<float>(n));
    for (uint64_t q = 0; q < nq; ++q) {
      for (uint64_t i = 0; i < n; ++i) {
        const int v = (int)(rng() % (uint64_t)distinct);
        dist[q][i] = v == 0 ? (rng() % 2 ? 0.0f : -0.0f) : (float)(v - distinct / 2) * 0.25f;
      }
      for (uint64_t s = 0; s < S; ++s) {
        std::vector<float> d;
        std::vector<uint64_t> l;
        for (uint64_t i = 0; i < n; ++i)
          if (shard[i] == s) { d.push_back(dist[q][i]); l.push_back(labels[i]); }
        std::vector<uint32_t> idx;
        const uint32_t count = prefilter_select_model(d.data(), d.size(), k, cap, &idx);
        if (prefilter_is_fallback(count, cap)) {
          parts[s].fallback[q] = 1;
        } else {
          for (uint32_t i : idx) parts[s].items.push_back(HandleCand{l[i], d[i]});
        }
        parts[s].begin[q + 1] = parts[s].items.size();
      }
    }
    HandleCands all;
    handle_union(parts, nq, &all);
    std::vector<uint64_t> which;
    handle_fallback_queries(all, 100, 100 + nq, &which);
    uint64_t marks = 0;
    for (uint64_t q = 0; q < nq; ++q) marks += all.fallback[q];
    if (which.size() != marks) ++bad;
    for (uint64_t q = 0; q < nq; ++q) {
      if (all.fallback[q]) { ++fell; continue; }
      ++answered;
      std::vector<float> od(k), rd(k);
      std::vector<uint64_t> ol(k), rl(k);
      uint64_t on = 0, rn = 0;
      handle_finish(all.items.data() + all.begin[q], all.begin[q + 1] - all.begin[q], k, od.data(), ol.data(), &on);
      prefilter_heap_rule(dist[q].data(), labels.data(), n, k, rd.data(), rl.data(), &rn);
      bool same = on == rn;
      for (uint64_t i = 0; same && i < on; ++i) same = ol[i] == rl[i] && od[i] == rd[i];
      // ... and the k smallest by (distance, label)
      std::vector<std::pair<float, uint64_t>> sorted(n);
      for (uint64_t i = 0; i < n; ++i) sorted[i] = {dist[q][i], labels[i]};
      std::sort(sorted.begin(), sorted.end());
      for (uint64_t i = 0; same && i < on; ++i) same = sorted[i].second == ol[i] && sorted[i].first == od[i];
      if (!same) ++bad;
    }
    // run splitting
    const uint64_t tq = rng() % 40;
    std::vector<const void *> tab(tq);
    static const int handles[3] = {0, 0, 0};
    for (uint64_t q = 0; q < tq; ++q) tab[q] = &handles[rng() % 3];
    std::vector<std::pair<uint64_t, uint64_t>> runs;
    handle_runs(tab.data(), tq, &runs);
    uint64_t at = 0;
    for (const auto &r : runs) {
      if (r.first != at || r.second <= r.first || r.second > tq) { ++bad; break; }
      for (uint64_t q = r.first; q < r.second; ++q)
        if (tab[q] != tab[r.first]) ++bad;
      if (r.second < tq && tab[r.second] == tab[r.first]) ++bad;
      at = r.second;
    }
    if (at != tq) ++bad;
  }
  printf("worlds=%d answered=%ld fell=%ld bad=%ld\n", worlds, answered, fell, bad);
  return bad ? 1 : 0;
}
