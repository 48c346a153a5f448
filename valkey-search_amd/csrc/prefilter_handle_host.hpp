// prefilter_handle_host.hpp -- the host half of the exact kNN from a filter handle (vk_index_search_filter_exact_batch):
// run splitting, the union of a sharded index's shards, the answer from the candidates, the fallback's bookkeeping.  No HIP
// call in here: tests/helpers/san_prefilter_handle_main.cc drives it with plain host memory under the sanitizers.
//
// The list a handle stands for is ascending and duplicate-free, so the reference's heap rule over it (prefilter_host.hpp:
// fill to k, replace the top only on a strictly smaller distance) keeps, among equal distances, the smaller labels: its
// answer is the k smallest by (distance, label).  The candidates of a query arrive with their LABELS instead of positions in
// a caller's array -- there is no such array on the host -- and label order is list order, so the rule runs over them sorted
// by label.  Any superset of {distance <= T} gives the same heap (prefilter_host.hpp has the argument), which is why a
// sharded index may take the union of its shards' candidates.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "prefilter_host.hpp"

namespace vk {

struct HandleCand {
  uint64_t label;
  float dist;
};
struct HandleCands {
  std::vector<uint64_t> begin;       // [nq + 1] into items
  std::vector<HandleCand> items;     // per query in label order
  std::vector<uint8_t> fallback;     // [nq] 1 = the query goes to the list path (its items are meaningless)
  void reset(uint64_t nq, bool all_fallback) {
    begin.assign(nq + 1, 0);
    items.clear();
    fallback.assign(nq, all_fallback ? 1 : 0);
  }
};

// consecutive queries with the same handle: [first, last) pairs covering 0 .. nq in order
inline void handle_runs(const void *const *tab, uint64_t nq, std::vector<std::pair<uint64_t, uint64_t>> *runs) {
  runs->clear();
  for (uint64_t q = 0; q < nq;) {
    uint64_t e = q + 1;
    while (e < nq && tab[e] == tab[q]) ++e;
    runs->emplace_back(q, e);
    q = e;
  }
}

// A sharded index: per query the union of its shards' candidates, back in label order (a label lives on one shard, so the
// union has no duplicates); a query that any shard hands over is handed over.
inline void handle_union(const std::vector<HandleCands> &parts, uint64_t nq, HandleCands *out) {
  out->reset(nq, false);
  for (uint64_t q = 0; q < nq; ++q) {
    const size_t first = out->items.size();
    for (const HandleCands &p : parts) {
      if (p.fallback[q]) { out->fallback[q] = 1; continue; }
      out->items.insert(out->items.end(), p.items.begin() + (std::ptrdiff_t)p.begin[q], p.items.begin() + (std::ptrdiff_t)p.begin[q + 1]);
    }
    if (out->fallback[q]) out->items.resize(first);
    else std::sort(out->items.begin() + (std::ptrdiff_t)first, out->items.end(), [](const HandleCand &a, const HandleCand &b) { return a.label < b.label; });
    out->begin[q + 1] = out->items.size();
  }
}

// The answer of one query from its candidates (label order): the heap rule, entries past the count (+inf, UINT64_MAX).
inline void handle_finish(const HandleCand *c, uint64_t n, uint64_t k, float *out_dist, uint64_t *out_label, uint64_t *out_n) {
  std::vector<float> d(n);
  std::vector<uint64_t> l(n);
  for (uint64_t i = 0; i < n; ++i) { d[i] = c[i].dist; l[i] = c[i].label; }
  prefilter_heap_rule(d.data(), l.data(), n, k, out_dist, out_label, out_n);
}

// The queries of run [q0, q1) that take the list path, in order.
inline void handle_fallback_queries(const HandleCands &c, uint64_t q0, uint64_t q1, std::vector<uint64_t> *which) {
  which->clear();
  for (uint64_t q = q0; q < q1; ++q)
    if (c.fallback[q - q0]) which->push_back(q);
}

}  // namespace vk
