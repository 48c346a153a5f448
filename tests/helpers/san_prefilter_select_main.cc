// The host half of the batched pre-filter search (csrc/prefilter_host.hpp) under -fsanitize=address,undefined: random key
// lists full of ties, "select as the kernel does (the header's model), then the heap rule over the hand-back" against the
// heap rule over the whole list -- for one device and for the union of 1 to 8 shards.  Usage: prog <seed> <lists>;
// prints bad=<mismatches>.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "prefilter_host.hpp"

using namespace vk;

namespace {

struct Answer {
  std::vector<float> d;
  std::vector<uint64_t> l;
  uint64_t n = 0;
  bool operator==(const Answer &o) const {
    if (n != o.n) return false;
    for (uint64_t i = 0; i < n; ++i)
      if (memcmp(&d[i], &o.d[i], 4) != 0 || l[i] != o.l[i]) return false;
    return true;
  }
};

Answer whole_list(const std::vector<float> &dist, const std::vector<uint64_t> &lab, uint64_t k) {
  Answer a;
  a.d.resize(k + 1);
  a.l.resize(k + 1);
  prefilter_heap_rule(dist.data(), lab.data(), dist.size(), k, a.d.data(), a.l.data(), &a.n);
  return a;
}

// what prefilter_device_stage does with the kernel's output, with the model in the kernel's place: the known entries of
// the list `part` (indices into the caller's list, ascending) are one segment
bool device_stage_model(const std::vector<float> &dist, const std::vector<uint64_t> &lab, const std::vector<uint64_t> &part, uint64_t k,
                        uint64_t cap, PrefilterCands *out) {
  PrefilterResolved r;
  std::vector<uint64_t> sub;
  for (uint64_t p : part) sub.push_back(lab[p]);
  prefilter_resolve(sub.data(), nullptr, sub.size(), 1, [&](uint64_t label, uint32_t *slot) {
    *slot = (uint32_t)(label & 0xFFFF);
    return label != ~0ull;   // (~0 plays the unknown key)
  }, &r);
  std::vector<float> seg;
  for (uint64_t p : r.pos) seg.push_back(dist[part[p]]);
  std::vector<uint32_t> idx;
  const uint32_t count = prefilter_select_model(seg.data(), seg.size(), k, cap, &idx);
  out->reset(1, false);
  if (prefilter_is_fallback(count, cap)) {
    out->fallback[0] = 1;
    return false;
  }
  if (count != idx.size()) { printf("model: count %u but %zu stored\n", count, idx.size()); exit(2); }
  for (uint32_t i : idx) out->items.push_back(PrefilterCand{part[r.pos[i]], seg[i]});
  out->begin[1] = out->items.size();
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
  const uint64_t lists = argc > 2 ? strtoull(argv[2], nullptr, 10) : 20000;
  std::mt19937_64 rng(seed);
  const uint64_t ks[] = {1, 2, 10, 64, 1000};
  uint64_t bad = 0, answered = 0, fell = 0, sharded_fell = 0, with_nan = 0;
  for (uint64_t it = 0; it < lists; ++it) {
    // lengths 0 .. 3000, short ones more often (the edges around k); 3 .. 50 distinct distances; duplicate labels; +-0;
    // every 16th list all equal; unknown keys mixed in
    const uint64_t n = (it % 4 == 0) ? rng() % 3001 : (it % 4 == 1) ? rng() % 80 : (it % 4 == 2) ? rng() % 1200 : rng() % 300;
    const uint64_t k = ks[rng() % 5];
    const uint64_t cap = (it % 7 == 0) ? k + rng() % 4 : prefilter_cap(k);   // (small slacks too: the fallback edge)
    const uint32_t n_vals = 3 + (uint32_t)(rng() % 48);
    std::vector<float> vals(n_vals);
    for (float &v : vals) v = (float)((int)(rng() % 41) - 20) * 0.25f;
    vals[0] = 0.0f;
    vals[1] = -0.0f;
    if (it % 5 == 0) vals[2] = INFINITY;
    const bool all_equal = it % 16 == 3;
    const bool nan = it % 97 == 5 && n > 0;
    // a key's distance belongs to its row: a label that appears twice brings the same distance twice
    std::vector<float> of_label(n / 2 + 1);
    for (float &v : of_label) v = all_equal ? vals[2 % n_vals] : vals[rng() % n_vals];
    if (nan) { of_label[rng() % of_label.size()] = NAN; }
    std::vector<float> dist(n);
    std::vector<uint64_t> lab(n);
    bool nan_in = false;
    for (uint64_t i = 0; i < n; ++i) {
      lab[i] = rng() % 9 == 0 ? ~0ull : rng() % (n / 2 + 1);   // duplicates everywhere
      dist[i] = lab[i] == ~0ull ? -1000.0f : of_label[lab[i]];  // (unknown keys never reach the device: any value)
      nan_in |= dist[i] != dist[i];
    }
    with_nan += nan_in;
    const Answer want = whole_list(dist, lab, k);

    // one device
    std::vector<uint64_t> all(n);
    for (uint64_t i = 0; i < n; ++i) all[i] = i;
    PrefilterCands one;
    if (device_stage_model(dist, lab, all, k, cap, &one)) {
      ++answered;
      Answer got;
      got.d.resize(k + 1);
      got.l.resize(k + 1);
      prefilter_finish(one.items.data(), one.items.size(), lab.data(), k, got.d.data(), got.l.data(), &got.n);
      if (one.items.size() > cap) ++bad;
      for (size_t i = 1; i < one.items.size(); ++i) bad += one.items[i - 1].pos >= one.items[i].pos;   // list order
      if (!(got == want)) {
        ++bad;
        if (bad < 10) printf("mismatch: list %llu n %llu k %llu cap %llu\n", (unsigned long long)it, (unsigned long long)n, (unsigned long long)k, (unsigned long long)cap);
      }
    } else {
      ++fell;
      // the decision itself: a NaN among the known keys, or more entries at or below the k-th smallest than cap
      std::vector<float> kd;
      bool has_nan = false;
      for (uint64_t i = 0; i < n; ++i)
        if (lab[i] != ~0ull) { kd.push_back(dist[i]); has_nan |= dist[i] != dist[i]; }
      if (!has_nan) {
        std::vector<float> s = kd;
        std::sort(s.begin(), s.end());
        const float T = s.empty() ? 0.f : s[std::min<uint64_t>(k, s.size()) - 1];
        uint64_t c = 0;
        for (float v : kd) c += v <= T;
        if (c <= cap) ++bad;   // fell back although the hand-back had room
      }
    }

    // 1 .. 8 shards: every key to a shard (by label, as a route table does), each shard's stage with the same k, the union
    const uint64_t S = 1 + rng() % 8;
    std::vector<std::vector<uint64_t>> part(S);
    const bool one_shard = it % 11 == 0;
    for (uint64_t i = 0; i < n; ++i) part[one_shard ? S - 1 : (lab[i] * 2654435761ull >> 7) % S].push_back(i);
    std::vector<PrefilterCands> parts(S);
    for (uint64_t s = 0; s < S; ++s) {
      if (part[s].empty()) continue;   // (left empty: the shard holds no key)
      device_stage_model(dist, lab, part[s], k, cap, &parts[s]);
    }
    PrefilterCands uni;
    prefilter_union(parts, 1, &uni);
    if (uni.fallback[0]) {
      ++sharded_fell;
    } else {
      Answer got;
      got.d.resize(k + 1);
      got.l.resize(k + 1);
      prefilter_finish(uni.items.data() + uni.begin[0], uni.begin[1] - uni.begin[0], lab.data(), k, got.d.data(), got.l.data(), &got.n);
      for (uint64_t i = uni.begin[0] + 1; i < uni.begin[1]; ++i) bad += uni.items[i - 1].pos >= uni.items[i].pos;
      if (!(got == want)) {
        ++bad;
        if (bad < 10) printf("sharded mismatch: list %llu n %llu k %llu shards %llu\n", (unsigned long long)it, (unsigned long long)n, (unsigned long long)k, (unsigned long long)S);
      }
    }
  }
  // (a run that answered nothing, or never fell back, checked nothing)
  if (lists >= 1000 && (answered == 0 || fell == 0 || sharded_fell == 0 || with_nan == 0)) ++bad;
  printf("lists=%llu answered=%llu fallback=%llu sharded_fallback=%llu nan=%llu bad=%llu\n", (unsigned long long)lists, (unsigned long long)answered,
         (unsigned long long)fell, (unsigned long long)sharded_fell, (unsigned long long)with_nan, (unsigned long long)bad);
  return bad ? 1 : 0;
}
