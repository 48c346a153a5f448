// Compile-and-run check of the MAINTAINED predicates of include/vk_vector_adaptor.h (MaintainFilter / NoteFilterChange /
// OnWritePhaseEnd) against the MOCK of the module's interface (tests/helpers/mock_valkey_search.h).  Compiled with
// -Wall -Wextra -Werror on every CPU run (tests/test_filter_delta_abi.py); run on a GPU by tests/test_filter_delta_gpu.py.
//
// A model of a tag index (src/indexes/tag.cc): every record has one of four tags; "@tag:{a}", "@tag:{b}", "@tag:{c}" are
// maintained, "@tag:{d}" is not.  Write phases mutate the model from several writer threads the way Tag::AddRecord /
// ModifyRecord / RemoveRecord do and note each change; after every OnWritePhaseEnd():
//   * filters_built went up by exactly the number of maintained keys that had changes (notes, or a longer label range);
//   * a maintained key is a cache HIT under the new epoch (hits +1, nothing built), its bitmap and count equal the model's and
//     those of a filter built from the fetchers;
//   * the unmaintained key is a miss, built from its fetchers, as before.
// Then the LRU bound evicts a maintained key: the next BuildFilter rebuilds it from the fetchers, and a write phase later
// (its notes were dropped: nothing was cached) it is still right.  One line per check, `bad=<n>` at the end.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "mock_valkey_search.h"
#include "vk_vector_adaptor.h"

using namespace valkey_search;
using namespace valkey_search::indexes;

extern "C" int ValkeyModule_ReplyWithSimpleString(ValkeyModuleCtx *, const char *) { return 0; }
extern "C" int ValkeyModule_ReplyWithLongLong(ValkeyModuleCtx *, long long) { return 0; }

static int g_bad = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) { ++g_bad; printf("BAD " __VA_ARGS__); printf("  [%s]\n", #cond); } \
  } while (0)

struct ListFetcher : EntriesFetcherBase {
  std::vector<InternedStringPtr> keys;
  struct It : EntriesFetcherIteratorBase {
    const std::vector<InternedStringPtr> *k;
    size_t i = 0;
    explicit It(const std::vector<InternedStringPtr> *keys) : k(keys) {}
    bool Done() const override { return i >= k->size(); }
    void Next() override { ++i; }
    const InternedStringPtr &operator*() const override { return (*k)[i]; }
  };
  size_t Size() const override { return keys.size(); }
  std::unique_ptr<EntriesFetcherIteratorBase> Begin() override { return std::make_unique<It>(&keys); }
};

constexpr int kTags = 4, kWriters = 4, kDim = 8;
static const char *kKey[kTags] = {"@tag:{a}", "@tag:{b}", "@tag:{c}", "@tag:{d}"};   // (d is not maintained)
struct Model {
  std::vector<int> tag;   // per internal id: 0..3, -1 = no record
  // the posting list of a tag, plus keys of the schema without a vector in this index
  std::queue<std::unique_ptr<EntriesFetcherBase>> fetchers(int t) const {
    auto f = std::make_unique<ListFetcher>();
    for (size_t i = 0; i < tag.size(); ++i)
      if (tag[i] == t) f->keys.push_back(std::make_shared<InternedString>(std::to_string(i)));
    f->keys.push_back(std::make_shared<InternedString>("doc:stranger"));
    std::queue<std::unique_ptr<EntriesFetcherBase>> q;
    q.push(std::move(f));
    return q;
  }
  std::vector<uint64_t> words(int t, uint64_t nbits, uint64_t *count) const {
    std::vector<uint64_t> w((nbits + 63) / 64, 0);
    *count = 0;
    for (size_t i = 0; i < tag.size() && i < nbits; ++i)
      if (tag[i] == t) { w[i >> 6] |= 1ull << (i & 63); ++*count; }
    return w;
  }
};
static uint32_t rnd(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
static std::string row_of(uint64_t id) {
  float v[kDim];
  uint64_t s = id * 977 + 5;
  for (float &f : v) f = (float)(rnd(s) % 2001) / 1000.f - 1.f;
  return std::string(reinterpret_cast<const char *>(v), sizeof v);
}
static vk_index_stats stats_of(vk_index *h) {
  vk_index_stats s;
  memset(&s, 0, sizeof s);
  vk_index_get_stats(h, &s);
  return s;
}

// what one writer thread does in a phase, on the ids it owns (id % kWriters == w)
struct Plan { int adds, add_tag, changes, from, to, removals; };   // add_tag / from / to: -1 = any tag

template <class Ix>
static void write_phase(Ix &ix, Model &m, const Plan &p, int phase) {
  const size_t old_n = m.tag.size();
  m.tag.resize(old_n + (size_t)p.adds * kWriters, -1);
  std::vector<std::thread> ts;
  std::atomic<int> failed{0};
  for (int w = 0; w < kWriters; ++w)
    ts.emplace_back([&, w] {
      uint64_t s = (uint64_t)phase * 1000 + (uint64_t)w;
      auto pick = [&](int want) {   // an id this writer owns with a record (and the wanted tag), or -1
        for (int tries = 0; tries < 200; ++tries) {
          const size_t id = (rnd(s) % (old_n / kWriters)) * kWriters + (size_t)w;
          if (id < old_n && m.tag[id] >= 0 && (want < 0 || m.tag[id] == want)) return (long)id;
        }
        return -1l;
      };
      for (int i = 0; i < p.adds; ++i) {             // Tag::AddRecord: a new key, its tag starts matching
        const size_t id = old_n + (size_t)i * kWriters + (size_t)w;
        const std::string rec = row_of(id);
        if (!ix.MockAdd(id, rec, std::make_shared<InternedString>(rec)).ok()) { failed.fetch_add(1); continue; }
        m.tag[id] = p.add_tag >= 0 ? p.add_tag : (int)(rnd(s) % kTags);
        ix.NoteFilterChange(kKey[m.tag[id]], id, true);
      }
      for (int i = 0; i < p.changes; ++i) {          // Tag::ModifyRecord: the old tag stops matching, the new one starts
        const long id = pick(p.from);
        if (id < 0) continue;
        const int to = p.to >= 0 ? p.to : (int)(rnd(s) % kTags);
        ix.NoteFilterChange(kKey[m.tag[(size_t)id]], (uint64_t)id, false);
        ix.NoteFilterChange(kKey[to], (uint64_t)id, true);      // (to == from: off then on, the last note wins)
        m.tag[(size_t)id] = to;
        if (i % 7 == 0) {                             // ... and back again within the phase
          ix.NoteFilterChange(kKey[to], (uint64_t)id, false);
          ix.NoteFilterChange(kKey[to], (uint64_t)id, true);
        }
      }
      for (int i = 0; i < p.removals; ++i) {         // Tag::RemoveRecord + the vector index's own removal
        const long id = pick(-1);
        if (id < 0) continue;
        ix.NoteFilterChange(kKey[m.tag[(size_t)id]], (uint64_t)id, false);
        if (!ix.MockRemove((uint64_t)id).ok()) failed.fetch_add(1);
        m.tag[(size_t)id] = -1;
      }
    });
  for (auto &t : ts) t.join();
  CHECK(failed.load() == 0, "phase %d: %d mutations failed", phase, failed.load());
}

// BuildFilter of tag t after a phase: hit or miss as expected, bitmap and count equal the model's and a fresh build's
template <class Ix>
static void check_key(Ix &ix, const Model &m, int t, bool want_hit, const char *when) {
  const uint64_t nbits = ix.GetMaxInternalLabel() + 1;
  const vk_index_stats s0 = stats_of(ix.handle());
  auto fq = m.fetchers(t);
  auto f = ix.BuildFilter(fq, nullptr, kKey[t]);
  const vk_index_stats s1 = stats_of(ix.handle());
  CHECK(f.ok(), "%s %s: BuildFilter failed", when, kKey[t]);
  if (!f.ok()) return;
  const uint64_t hits = s1.filter_cache_hits - s0.filter_cache_hits, misses = s1.filter_cache_misses - s0.filter_cache_misses,
                 built = s1.filters_built - s0.filters_built;
  if (want_hit) CHECK(hits == 1 && misses == 0 && built == 0, "%s %s: hits +%llu misses +%llu built +%llu, want a hit", when, kKey[t],
                      (unsigned long long)hits, (unsigned long long)misses, (unsigned long long)built);
  else CHECK(hits == 0 && misses == 1 && built == 1, "%s %s: hits +%llu misses +%llu built +%llu, want a miss and a build", when, kKey[t],
             (unsigned long long)hits, (unsigned long long)misses, (unsigned long long)built);
  uint64_t want_count = 0, got_nbits = 0, got_count = 0;
  const std::vector<uint64_t> want = m.words(t, nbits, &want_count);
  vk_filter_info(f.value().get(), &got_nbits, &got_count);
  std::vector<uint64_t> got(want.size() + 2, ~0ull);
  CHECK(vk_filter_read(f.value().get(), got.data(), got.size()) == VK_OK, "%s %s: read failed", when, kKey[t]);
  CHECK(got_nbits == nbits && got_count == want_count, "%s %s: nbits %llu / %llu allowed %llu / %llu", when, kKey[t], (unsigned long long)got_nbits,
        (unsigned long long)nbits, (unsigned long long)got_count, (unsigned long long)want_count);
  CHECK(std::equal(want.begin(), want.end(), got.begin()) && got[want.size()] == 0 && got[want.size() + 1] == 0, "%s %s: bitmap differs from the model", when, kKey[t]);
  auto fq2 = m.fetchers(t);
  auto fresh = ix.BuildFilter(fq2, nullptr);         // (no cache key: built from the fetchers)
  CHECK(fresh.ok(), "%s %s: fresh BuildFilter failed", when, kKey[t]);
  if (!fresh.ok()) return;
  std::vector<uint64_t> ref(got.size(), ~0ull);
  vk_filter_read(fresh.value().get(), ref.data(), ref.size());
  CHECK(ref == got && fresh.value().allowed() == got_count, "%s %s: differs from the filter built from the fetchers", when, kKey[t]);
  printf("%s %s: %s, %llu of %llu allowed\n", when, kKey[t], want_hit ? "hit" : "miss", (unsigned long long)got_count, (unsigned long long)nbits);
}

template <class Ix>
static int run(Ix &ix, const char *name) {
  Model m;
  const size_t n0 = 2000;
  uint64_t s = 42;
  for (size_t i = 0; i < n0; ++i) {
    const std::string rec = row_of(i);
    if (!ix.MockAdd(i, rec, std::make_shared<InternedString>(rec)).ok()) { printf("%s add failed at %zu\n", name, i); return 1; }
    m.tag.push_back((int)(rnd(s) % kTags));
  }
  for (int t = 0; t < 3; ++t) ix.MaintainFilter(kKey[t]);
  ix.NoteFilterChange("@tag:{zzz}", 1, true);        // a key nobody maintains: dropped
  CHECK(ix.OnWritePhaseEnd().ok(), "first flush");
  for (int t = 0; t < kTags; ++t) check_key(ix, m, t, false, "phase0");   // nothing cached yet: every key is built from its fetchers
  const Plan plans[5] = {
      {40, -1, 60, -1, -1, 10},   // adds, tag changes and removals across every tag
      {0, -1, 30, 0, 3, 0},       // only a -> d: b and c have neither notes nor growth
      {0, -1, 0, -1, -1, 0},      // nothing at all
      {25, 3, 0, -1, -1, 0},      // adds under the unmaintained tag only: every maintained filter just grows
      {30, -1, 80, -1, -1, 25}};
  const int want_built[5] = {3, 1, 0, 3, 3};
  int phases = 0;
  for (int p = 0; p < 5; ++p) {
    write_phase(ix, m, plans[p], p + 1);
    const vk_index_stats s0 = stats_of(ix.handle());
    CHECK(ix.OnWritePhaseEnd().ok(), "phase %d: OnWritePhaseEnd", p + 1);
    const vk_index_stats s1 = stats_of(ix.handle());
    CHECK((int)(s1.filters_built - s0.filters_built) == want_built[p], "phase %d: filters_built +%llu, want +%d", p + 1,
          (unsigned long long)(s1.filters_built - s0.filters_built), want_built[p]);
    const std::string when = "phase" + std::to_string(p + 1);
    for (int t = 0; t < kTags; ++t) check_key(ix, m, t, t < 3, when.c_str());
    ++phases;
  }
  // ---- the LRU bound evicts a maintained key: rebuilt from its fetchers, and right again a phase later
  CHECK(vk_index_set_option(ix.handle(), "filter-cache-entries", 2) == VK_OK, "set filter-cache-entries");
  write_phase(ix, m, Plan{8, -1, 40, -1, -1, 4}, 6);
  CHECK(ix.OnWritePhaseEnd().ok(), "evict: OnWritePhaseEnd");
  const vk_index_stats se = stats_of(ix.handle());
  CHECK(se.filter_cache_entries == 2, "evict: %llu entries, want 2", (unsigned long long)se.filter_cache_entries);
  int rebuilt = 0;
  for (int t = 0; t < 3; ++t) {
    vk_filter *probe = nullptr;                       // (which of the three was pushed out?)
    vk_index_filter_cache_get(ix.handle(), kKey[t], strlen(kKey[t]), ix.FilterEpoch(), &probe);
    if (probe) vk_filter_release(probe);
    else ++rebuilt;
    // (the probe of an evicted key counted one miss already; check_key's own lookup is what it measures)
    check_key(ix, m, t, probe != nullptr, "evict");
  }
  CHECK(rebuilt >= 1, "evict: no maintained key was evicted");
  write_phase(ix, m, Plan{4, -1, 40, -1, -1, 4}, 7);
  CHECK(ix.OnWritePhaseEnd().ok(), "after evict: OnWritePhaseEnd");
  for (int t = 0; t < 3; ++t) {
    vk_filter *probe = nullptr;
    vk_index_filter_cache_get(ix.handle(), kKey[t], strlen(kKey[t]), ix.FilterEpoch(), &probe);
    if (probe) vk_filter_release(probe);
    check_key(ix, m, t, probe != nullptr, "after-evict");
  }
  ix.ForgetFilter(kKey[0]);                           // no longer maintained: a miss after the next phase, like d
  write_phase(ix, m, Plan{0, -1, 20, -1, -1, 0}, 8);
  CHECK(ix.OnWritePhaseEnd().ok(), "forget: OnWritePhaseEnd");
  check_key(ix, m, 0, false, "forgotten");
  printf("%s phases=%d bad=%d\n", name, phases, g_bad);
  return g_bad ? 1 : 0;
}

int main(int argc, char **argv) {
  const std::string algo = argc > 1 ? argv[1] : "flat";
  data_model::VectorIndex proto;
  proto.dimension_count_ = kDim;
  proto.initial_cap_ = 8192;
  proto.distance_metric_ = data_model::DISTANCE_METRIC_L2;
  proto.hnsw_.ef_construction_ = 60;
  if (algo == "flat") {
    auto ix = VectorGpuFlat<float>::Create(proto, "v", data_model::ATTRIBUTE_DATA_TYPE_HASH);
    if (!ix.ok()) { printf("create failed: %s\n", ix.status().message().c_str()); return 1; }
    return run(*ix.value(), "flat");
  }
  auto ix = VectorGpuHNSW<float>::Create(proto, "v", data_model::ATTRIBUTE_DATA_TYPE_HASH, false, 8192);
  if (!ix.ok()) { printf("create failed: %s\n", ix.status().message().c_str()); return 1; }
  return run(*ix.value(), "hnsw");
}
