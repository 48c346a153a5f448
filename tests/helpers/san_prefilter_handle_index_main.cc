// san_prefilter_handle_index_main.cc -- TEST INFRASTRUCTURE (tests/test_prefilter_handle_host_cpu.py): the host half of
// vk_index_search_filter_exact_batch under ASAN / UBSAN, host only.
//
// The REAL Index::search_filter_exact_batch and filter_read_labels (csrc/prefilter_handle.cc), the real
// Index::search_labels_batch behind the fallback (csrc/prefilter_batch.cc), index_common.cc and filter_set.cc are linked
// against the virtual HIP layer (hip_virtual.cc) and host models of the kernels they reach: the filter builds and
// launch_filter_expand, which read and write THROUGH the device pointers the host code handed them.  The index is a fake:
// its handle_candidates marks none, all or some of a run's queries "take the list path" (a query carries its mark in its
// third component) and hands back, for the others, every known label of the filter with its distance, in label order -- a
// superset of what the select kernel hands back, which the heap rule is exact over; its prefilter_candidates (reached only
// through the fallback) does the same over the downloaded list.  Random handle tables over four filters (one empty, one
// full, one whose labels are all unknown), nq 0 - 40, k 1 / 5 / 64: every answer must be prefilter_heap_rule's over the
// filter's ascending list, the padding (+inf, UINT64_MAX), and batches / queries / runs / fallback_queries /
// downloaded_runs exactly what the marks say.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>

#include "hip_virtual.hpp"
#include "index.hpp"

namespace vk {
// ---- filter_build.hip and filter_expand.hip as host models on the virtual streams
uint32_t filter_set_ids_blocks(uint64_t n) { return n ? 1 : 0; }
uint32_t filter_set_runs_blocks(uint64_t n) { return n ? 1 : 0; }
uint32_t filter_combine_blocks(uint64_t) { return 1; }
hipError_t launch_filter_set_ids(uint64_t *bits, uint64_t nbits, const uint64_t *d_ids, uint64_t n, unsigned long long *d_partial, hipStream_t s) {
  hipv::launch(s, "filter_set_ids_kernel", {{bits, (size_t)((nbits + 63) / 64 + 1) * 8, "bits"}, {d_ids, (size_t)n * 8, "ids"}, {d_partial, 8, "partial"}}, [=] {
    unsigned long long on = 0;
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t id = d_ids[i];
      if (id >= nbits) continue;
      const uint64_t b = 1ull << (id & 63);
      if (!(bits[id >> 6] & b)) { bits[id >> 6] |= b; ++on; }
    }
    d_partial[0] = on;
  });
  return hipSuccess;
}
hipError_t launch_filter_set_runs(uint64_t *, uint64_t, const uint64_t *, uint64_t, unsigned long long *, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_filter_popcount(const uint64_t *bits, uint64_t words, unsigned long long *d_out, hipStream_t s) {
  hipv::launch(s, "filter_popcount_kernel", {{bits, (size_t)words * 8, "bits"}, {d_out, 8, "count"}}, [=] {
    for (uint64_t i = 0; i < words; ++i) *d_out += (unsigned long long)__builtin_popcountll(bits[i]);
  });
  return hipSuccess;
}
hipError_t launch_filter_combine(uint64_t *, const uint64_t *, const uint64_t *, uint64_t, uint32_t, unsigned long long *, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_filter_combine_batch(const uint64_t *, uint32_t, uint64_t, unsigned long long *, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_filter_delta_copy(const uint64_t *, uint32_t, uint64_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_filter_delta_apply(const uint64_t *, const uint64_t *, uint64_t, int, unsigned long long *, hipStream_t) { return hipErrorNotSupported; }

uint32_t filter_expand_tiles(uint64_t nbits) { return (uint32_t)((((nbits + 63) >> 6) + 1023) / 1024); }
hipError_t launch_filter_expand(const uint64_t *bits, uint64_t nbits, uint64_t cap, uint64_t *labels, unsigned long long *total,
                                unsigned long long *tile_off, hipStream_t s) {
  const size_t tiles = filter_expand_tiles(nbits);
  hipv::launch(s, "filter_expand_kernels", {{bits, (size_t)((nbits + 63) / 64) * 8, "bits"}, {labels, (size_t)cap * 8, "labels"}, {total, 8, "total"},
                                            {tile_off, tiles * 8, "tile_off"}}, [=] {
    unsigned long long n = 0;
    for (size_t t = 0; t < tiles; ++t) tile_off[t] = 0xA5A5A5A5A5A5A5A5ull;   // (scratch: written, never read by the host)
    for (uint64_t b = 0; b < nbits; ++b)
      if ((bits[b >> 6] >> (b & 63)) & 1) {
        if (n < cap) labels[n] = b;
        ++n;
      }
    *total = n;
  });
  return hipSuccess;
}
// the device stage and the single call's path: linked, never reached from a fake index
uint32_t prefilter_tiles(uint64_t entries) { return (uint32_t)((entries + 63) / 64); }
uint32_t label_map_key_tiles(uint64_t keys) { return (uint32_t)((keys + 255) / 256); }
hipError_t launch_prefilter_distance(const PrefilterDistArgs &, bool, bool, hipStream_t) { abort(); }
hipError_t launch_prefilter_select(const PrefilterSelectArgs &, hipStream_t) { abort(); }
hipError_t launch_label_map_resolve(const LabelMapResolveArgs &, hipStream_t) { abort(); }
hipError_t launch_filter_gather_labels(const uint32_t *, const uint2 *, const uint32_t *, const uint64_t *, uint32_t, uint32_t, uint32_t, uint64_t *,
                                       hipStream_t) { abort(); }
Status Index::search_labels(const float *, uint64_t, const uint64_t *, uint64_t, float *, uint64_t *, uint64_t *) { abort(); }
}  // namespace vk

namespace {

constexpr uint64_t kDim = 4;
bool known(uint64_t label) { return label % 5 != 3 && label < 100000; }
float fake_distance(const float *q, uint64_t label) { return (float)((label * 37 + (uint64_t)q[0] * 11) % 23) + q[1]; }   // few values: ties

struct HandleIndex final : vk::Index {
  explicit HandleIndex(const vk_index_params &p) : Index(p) {}
  uint64_t stage_calls = 0, list_batches = 0;
  vk::Status handle_candidates(const float *queries, uint64_t nq, uint64_t, const vk::FilterSet &f, vk::HandleCands *out) override {
    ++stage_calls;
    std::vector<uint64_t> bits(f.words() + 1);
    VK_TRY(f.read(bits.data(), bits.size()));
    out->reset(nq, false);
    for (uint64_t q = 0; q < nq; ++q) {
      const float *qv = queries + q * kDim;
      if (qv[2] != 0.f) {
        out->fallback[q] = 1;
      } else {
        for (uint64_t b = 0; b < f.nbits(); ++b)
          if (((bits[b >> 6] >> (b & 63)) & 1) && known(b)) out->items.push_back(vk::HandleCand{b, fake_distance(qv, b)});
      }
      out->begin[q + 1] = out->items.size();
    }
    return vk::Status::Ok();
  }
  vk::Status prefilter_candidates(const float *queries, uint64_t nq, uint64_t, const uint64_t *labels, const uint64_t *list_begin, uint64_t n_labels,
                                  vk::PrefilterCands *out) override {
    ++list_batches;
    if (list_begin) abort();   // the fallback sends the run's shared list
    out->reset(nq, false);
    for (uint64_t q = 0; q < nq; ++q) {
      for (uint64_t i = 0; i < n_labels; ++i)
        if (known(labels[i])) out->items.push_back(vk::PrefilterCand{i, fake_distance(queries + q * kDim, labels[i])});
      out->begin[q + 1] = out->items.size();
    }
    return vk::Status::Ok();
  }
  vk::Status search(const vk::SearchRequest &, float *, uint64_t *, uint64_t *) override { return vk::Status::Ok(); }
  vk::Status add(uint64_t, const float *) override { return vk::Status::Ok(); }
  vk::Status add_batch(const uint64_t *, const float *, uint64_t) override { return vk::Status::Ok(); }
  vk::Status remove(uint64_t) override { return vk::Status::Ok(); }
  vk::Status resize(uint64_t) override { return vk::Status::Ok(); }
  vk::Status set_ef(uint32_t) override { return vk::Status::Ok(); }
  vk::Status flush() override { return vk::Status::Ok(); }
  vk::Status search_device(const vk::SearchRequest &, float *, uint64_t *, uint32_t *, hipStream_t) override { return vk::Status::Ok(); }
  vk::Status label_distances(const float *, const uint64_t *, uint64_t, float *, uint8_t *) override { return vk::Status::Ok(); }
  vk::Status distance(uint64_t, const float *, float *) override { return vk::Status::Ok(); }
  vk::Status get_row(uint64_t, float *) override { return vk::Status::Ok(); }
  vk::Status contains(uint64_t, bool *) override { return vk::Status::Ok(); }
  vk::Status stats(vk_index_stats *) override { return vk::Status::Ok(); }
  vk::Status device_rows(uint64_t, void **, uint64_t *) override { return vk::Status::Ok(); }
  vk::Status commit_device_rows(uint64_t, const uint64_t *) override { return vk::Status::Ok(); }
  vk::Status save(vk_write_chunk_fn, void *) override { return vk::Status::Ok(); }
  void filter_devices(std::vector<int> *out) const override { out->assign(1, 0); }
};

uint64_t g_bad = 0;
#define CHECK(cond, ...)                                                                          \
  do {                                                                                            \
    if (!(cond)) { ++g_bad; fprintf(stderr, "BAD [%s] ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
  } while (0)

}  // namespace

int main(int argc, char **argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 300;
  hipv::set_device_count(1);
  std::mt19937_64 rng(12345);
  vk_index_params p{};
  p.struct_size = sizeof p;
  p.dim = kDim;
  p.algo = VK_ALGO_FLAT;
  HandleIndex ix(p);
  // four filters: empty, full (65 bits: a masked last word), sparse over a few tiles, and labels that are all unknown
  struct F { std::shared_ptr<vk::FilterSet> set; std::vector<uint64_t> list; };
  std::vector<F> fs(4);
  const uint64_t nbits[4] = {100, 65, 70000, 500};
  for (int j = 0; j < 4; ++j) {
    std::vector<uint64_t> ids;
    if (j == 1) for (uint64_t b = 0; b < 70; ++b) ids.push_back(b);                       // (66 .. 69 are past nbits: ignored)
    if (j == 2) for (int i = 0; i < 900; ++i) ids.push_back(rng() % (nbits[2] + 50));
    if (j == 3) for (uint64_t b = 3; b < 500; b += 5) ids.push_back(b);
    CHECK(vk::FilterSet::build({0}, nbits[j], ids.data(), ids.size(), nullptr, 0, nullptr, &fs[j].set).ok(), "build %d", j);
    if (!fs[j].set) return 1;
    std::vector<bool> m(nbits[j], false);
    for (uint64_t id : ids) if (id < nbits[j]) m[id] = true;
    for (uint64_t b = 0; b < nbits[j]; ++b) if (m[b]) fs[j].list.push_back(b);
    // vk_filter_read_labels' code: the whole list, a short buffer, no buffer
    const uint64_t total_want = fs[j].list.size();
    for (uint64_t cap : {total_want, total_want / 2, (uint64_t)0, total_want + 7}) {
      std::vector<uint64_t> got(cap + 1, 0xEEEEEEEEEEEEEEEEull);
      uint64_t total = ~0ull;
      CHECK(vk::filter_read_labels(*fs[j].set, got.data(), cap, &total).ok() && total == total_want, "read_labels %d cap %llu", j, (unsigned long long)cap);
      const uint64_t n = std::min(cap, total_want);
      CHECK(std::equal(got.begin(), got.begin() + (std::ptrdiff_t)n, fs[j].list.begin()), "read_labels %d: labels", j);
      for (uint64_t i = n; i <= cap; ++i) CHECK(got[i] == 0xEEEEEEEEEEEEEEEEull, "read_labels %d: wrote past min(total, cap)", j);
    }
  }
  uint64_t want_batches = 0, want_queries = 0, want_runs = 0, want_fell = 0, want_down = 0, modes[3] = {0, 0, 0};
  const uint64_t ks[3] = {1, 5, 64};
  for (int r = 0; r < rounds; ++r) {
    const uint64_t nq = rng() % 41, k = ks[rng() % 3];
    std::vector<float> Q(nq * kDim + 1);
    std::vector<const vk::FilterSet *> tab(nq);
    std::vector<int> which(nq);
    uint64_t runs = 0, fell = 0, down = 0;
    for (uint64_t q = 0; q < nq;) {
      const int j = (int)(rng() % 4), mode = (int)(rng() % 3);   // this run: marks on none / all / some of its queries
      uint64_t len = 1 + rng() % 6, marked = 0;
      // (two neighbouring stretches may draw the same handle: then they are ONE run, counted below)
      for (uint64_t e = q; e < std::min(nq, q + len); ++e) {
        which[e] = j;
        tab[e] = fs[j].set.get();
        float *qv = Q.data() + e * kDim;
        qv[0] = (float)(rng() % 50); qv[1] = 0.25f * (float)(rng() % 3); qv[3] = 0.f;
        const bool mark = mode == 1 || (mode == 2 && rng() % 2);
        qv[2] = mark ? 1.f : 0.f;
        marked += mark;
      }
      ++modes[mode];
      fell += marked;
      q = std::min(nq, q + len);
    }
    // runs = maximal stretches of one handle; downloaded runs: those with at least one mark
    for (uint64_t q = 0; q < nq;) {
      uint64_t e = q;
      bool any = false;
      while (e < nq && tab[e] == tab[q]) { any = any || Q[e * kDim + 2] != 0.f; ++e; }
      down += any;
      ++runs;
      q = e;
    }
    std::vector<float> od(nq * k + 1, 7.f);
    std::vector<uint64_t> ol(nq * k + 1, 7), on(nq + 1, 7);
    vk::Status st = ix.search_filter_exact_batch(Q.data(), nq, k, tab.data(), od.data(), ol.data(), on.data());
    CHECK(st.ok(), "search_filter_exact_batch: %s", st.msg.c_str());
    CHECK(od[nq * k] == 7.f && ol[nq * k] == 7 && on[nq] == 7, "wrote past the outputs");
    for (uint64_t q = 0; q < nq; ++q) {
      const std::vector<uint64_t> &list = fs[which[q]].list;
      std::vector<float> d(list.size()), wd(k);
      std::vector<uint64_t> l(list.size()), wl(k);
      uint64_t wn = 0;
      for (size_t i = 0; i < list.size(); ++i) { l[i] = known(list[i]) ? list[i] : ~0ull; d[i] = fake_distance(Q.data() + q * kDim, list[i]); }
      vk::prefilter_heap_rule(d.data(), l.data(), list.size(), k, wd.data(), wl.data(), &wn);
      bool ok = on[q] == wn;
      for (uint64_t i = 0; ok && i < wn; ++i) ok = od[q * k + i] == wd[i] && ol[q * k + i] == wl[i];
      for (uint64_t i = wn; ok && i < k; ++i) ok = od[q * k + i] == __builtin_inff() && ol[q * k + i] == ~0ull;
      CHECK(ok, "round %d query %llu (filter %d, mark %g, k %llu): answer differs", r, (unsigned long long)q, which[q], Q[q * kDim + 2], (unsigned long long)k);
    }
    if (nq) { ++want_batches; want_queries += nq; want_runs += runs; want_fell += fell; want_down += down; }
    vk_filter_exact_stats s;
    CHECK(ix.filter_exact_stats(&s).ok(), "stats");
    CHECK(s.batches == want_batches && s.queries == want_queries && s.runs == want_runs && s.fallback_queries == want_fell &&
              s.downloaded_runs == want_down && s.struct_size == sizeof s,
          "round %d: stats %llu %llu %llu %llu %llu, want %llu %llu %llu %llu %llu", r, (unsigned long long)s.batches, (unsigned long long)s.queries,
          (unsigned long long)s.runs, (unsigned long long)s.fallback_queries, (unsigned long long)s.downloaded_runs, (unsigned long long)want_batches,
          (unsigned long long)want_queries, (unsigned long long)want_runs, (unsigned long long)want_fell, (unsigned long long)want_down);
    CHECK(down == 0 || ix.list_batches > 0, "the list path was not taken");
  }
  // k == 0 and nq == 0
  {
    uint64_t on[3] = {7, 7, 7};
    float q[3 * kDim] = {0};
    const vk::FilterSet *tab[3] = {fs[1].set.get(), fs[1].set.get(), fs[2].set.get()};
    CHECK(ix.search_filter_exact_batch(q, 3, 0, tab, nullptr, nullptr, on).ok() && on[0] == 0 && on[1] == 0 && on[2] == 0, "k == 0");
    CHECK(ix.search_filter_exact_batch(nullptr, 0, 5, nullptr, nullptr, nullptr, nullptr).ok(), "nq == 0");
  }
  fs.clear();
  for (const std::string &v : hipv::take_violations()) { fprintf(stderr, "VIOLATION %s\n", v.c_str()); ++g_bad; }
  printf("rounds=%d runs=%llu fell=%llu downloaded=%llu modes=%llu/%llu/%llu stage_calls=%llu list_batches=%llu kernels=%llu bad=%llu\n", rounds,
         (unsigned long long)want_runs, (unsigned long long)want_fell, (unsigned long long)want_down, (unsigned long long)modes[0],
         (unsigned long long)modes[1], (unsigned long long)modes[2], (unsigned long long)ix.stage_calls, (unsigned long long)ix.list_batches,
         (unsigned long long)hipv::kernels(), (unsigned long long)g_bad);
  return g_bad ? 1 : 0;
}
