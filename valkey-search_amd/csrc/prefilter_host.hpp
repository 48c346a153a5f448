// prefilter_host.hpp -- the host half of the batched pre-filter search (vk_index_search_labels_batch).  No HIP call in
// here: tests/helpers/san_prefilter_select_main.cc drives it with plain host memory under the sanitizers.
//
// The reference's pre-filter branch (search.cc:457-481 -> vector_base.cc:509-530) runs a heap of k over the keys IN THE
// CALLER'S ORDER: fill to k, then a key replaces the heap top only when its distance is strictly smaller.  The device stage
// (prefilter_select.hip) does not run that rule; it hands back, per query, every entry at or below T = the k-th smallest
// distance of the list (the list's maximum when it has fewer than k entries), in list order, and the host runs the rule
// over those few entries.
//
// Why that is exact.  The rule's answer depends only on the entries with distance <= T and their relative order:
//   * after i entries the heap's distances are the min(i, k) smallest seen so far;
//   * an entry above T is only ever evicted by, or refused in favour of, something smaller, and it never displaces an
//     entry <= T (an entry <= T is refused or evicted only while k entries <= T that came before it are in the heap);
//   * an entry <= T meets a heap that is not full, or a top above T, exactly when the run over the <= T subsequence alone
//     would have had room for it.
// So the rule over ANY superset of {distance <= T}, in list order, ends with the same heap.  Two things rest on this: the
// device may hand back more than k entries (ties at T; up to `cap`, beyond which the query takes the old path), and a
// sharded index may take the union of its shards' candidates (each shard's T is at or above the global one).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <queue>
#include <utility>
#include <vector>

namespace vk {

// what the device stage covers: k up to kPrefilterMaxK, and per query k + kPrefilterSlack handed-back entries
constexpr uint64_t kPrefilterMaxK = 4096;
constexpr uint64_t kPrefilterSlack = 64;
inline uint64_t prefilter_cap(uint64_t k) { return k <= kPrefilterMaxK ? k + kPrefilterSlack : 0; }
// scratch bounds of one device pass (a batch is cut into chunks of queries): distances, staged queries, hand-back
constexpr uint64_t kPrefilterChunkEntries = 1ull << 24;   // x 4 B
constexpr uint64_t kPrefilterChunkBytes = 64ull << 20;
constexpr uint32_t kPrefilterCountNaN = 0xFFFFFFFFu;      // the select kernel's count word of a segment that holds a NaN

// vector_base.cc:509-530: fill to k, then a key replaces the heap top only when its distance is strictly smaller (ties
// keep what is already there); labels[i] == UINT64_MAX = unknown key, skipped.  Output ascending by (distance, label).
inline void prefilter_heap_rule(const float *dist, const uint64_t *labels, uint64_t n, uint64_t k, float *out_dist,
                                uint64_t *out_label, uint64_t *out_n) {
  std::priority_queue<std::pair<float, uint64_t>> results;
  for (uint64_t i = 0; i < n; ++i) {
    if (labels[i] == ~0ull) continue;  // unknown key: ComputeDistanceFromRecord failed
    if (results.size() < k) {
      results.emplace(dist[i], labels[i]);
    } else if (k && dist[i] < results.top().first) {
      results.pop();
      results.emplace(dist[i], labels[i]);
    }
  }
  uint64_t m = results.size();
  *out_n = m;
  while (m) {
    --m;
    out_dist[m] = results.top().first;
    out_label[m] = results.top().second;
    results.pop();
  }
}

// order-preserving f32 -> u32 of the select kernel (merge_key of flat_scan.hip: -0 and +0 share a key, as they compare equal)
inline uint32_t prefilter_key(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- the lists of a batch, resolved to row slots -------------------------------------------------------------------
// One resolve per DISTINCT list: a shared list (list_begin == nullptr) is resolved once, whatever nq is.  Unknown labels
// are dropped; the survivors keep their position in the caller's label array (`pos`, absolute).
struct PrefilterResolved {
  bool shared = false;
  uint64_t nq = 0;
  std::vector<uint32_t> slot;    // surviving entries, list after list
  std::vector<uint64_t> pos;     // [slot.size()] index into the caller's labels
  std::vector<uint64_t> begin;   // shared: {0, m}; otherwise nq + 1 offsets into slot / pos
};

template <class Lookup>   // bool lookup(uint64_t label, uint32_t *slot)
void prefilter_resolve(const uint64_t *labels, const uint64_t *list_begin, uint64_t n_labels, uint64_t nq, Lookup &&lookup,
                       PrefilterResolved *r) {
  r->shared = list_begin == nullptr;
  r->nq = nq;
  r->slot.clear();
  r->pos.clear();
  r->begin.assign(1, 0);
  const uint64_t lists = r->shared ? 1 : nq;
  for (uint64_t l = 0; l < lists; ++l) {
    const uint64_t lo = r->shared ? 0 : list_begin[l], hi = r->shared ? n_labels : list_begin[l + 1];
    for (uint64_t i = lo; i < hi; ++i) {
      uint32_t s;
      if (!lookup(labels[i], &s)) continue;
      r->slot.push_back(s);
      r->pos.push_back(i);
    }
    r->begin.push_back(r->slot.size());
  }
}
inline uint64_t prefilter_seg_lo(const PrefilterResolved &r, uint64_t q) { return r.shared ? 0 : r.begin[q]; }
inline uint64_t prefilter_seg_len(const PrefilterResolved &r, uint64_t q) { return r.shared ? r.begin[1] : r.begin[q + 1] - r.begin[q]; }

// ---- candidates ------------------------------------------------------------------------------------------------------
struct PrefilterCand {
  uint64_t pos;   // position in the caller's label array
  float dist;
};
struct PrefilterCands {
  std::vector<uint64_t> begin;        // [nq + 1] into items
  std::vector<PrefilterCand> items;   // per query in position order
  std::vector<uint8_t> fallback;      // [nq] 1 = the query goes to the per-query path (its items are meaningless)
  void reset(uint64_t nq, bool all_fallback) {
    begin.assign(nq + 1, 0);
    items.clear();
    fallback.assign(nq, all_fallback ? 1 : 0);
  }
};

// The fallback decision on the select kernel's count word: a NaN in the segment, or more entries at or below T than the
// hand-back holds.
inline bool prefilter_is_fallback(uint32_t count, uint64_t cap) { return count == kPrefilterCountNaN || count > cap; }

// A plain model of what the select kernel emits for one segment of n distances: T by the same binary descent over the
// keys (the largest T with count(key < T) < k; all ones when n < k), then, front to back, the index of every entry with
// key <= T -- at most cap of them stored, all of them counted.  Returns the count word.
inline uint32_t prefilter_select_model(const float *dist, uint64_t n, uint64_t k, uint64_t cap, std::vector<uint32_t> *idx) {
  idx->clear();
  for (uint64_t i = 0; i < n; ++i)
    if (dist[i] != dist[i]) return kPrefilterCountNaN;
  uint32_t T = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t c = T | (1u << bit);
    uint64_t below = 0;
    for (uint64_t i = 0; i < n; ++i) below += prefilter_key(dist[i]) < c;
    if (below < k) T = c;
  }
  uint32_t count = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (prefilter_key(dist[i]) > T) continue;
    if (count < cap) idx->push_back((uint32_t)i);
    ++count;
  }
  return count;
}

// A sharded index: the union of its shards' candidates per query, back in position order; a query that any shard hands
// over is handed over.  parts[s] covers the same nq queries; positions are already the caller's.
inline void prefilter_union(const std::vector<PrefilterCands> &parts, uint64_t nq, PrefilterCands *out) {
  out->reset(nq, false);
  for (uint64_t q = 0; q < nq; ++q) {
    const size_t first = out->items.size();
    for (const PrefilterCands &p : parts) {
      if (p.fallback.empty()) continue;   // (a shard that holds no key of the batch)
      if (p.fallback[q]) { out->fallback[q] = 1; continue; }
      out->items.insert(out->items.end(), p.items.begin() + p.begin[q], p.items.begin() + p.begin[q + 1]);
    }
    if (out->fallback[q]) out->items.resize(first);
    else std::sort(out->items.begin() + first, out->items.end(), [](const PrefilterCand &a, const PrefilterCand &b) { return a.pos < b.pos; });
    out->begin[q + 1] = out->items.size();
  }
}

// The answer of one query from its candidates: the heap rule over them in position order, labels from the caller's list.
inline void prefilter_finish(const PrefilterCand *c, uint64_t n, const uint64_t *labels, uint64_t k, float *out_dist, uint64_t *out_label,
                             uint64_t *out_n) {
  std::vector<float> d(n);
  std::vector<uint64_t> l(n);
  for (uint64_t i = 0; i < n; ++i) { d[i] = c[i].dist; l[i] = labels[c[i].pos]; }
  prefilter_heap_rule(d.data(), l.data(), n, k, out_dist, out_label, out_n);
}

}  // namespace vk
