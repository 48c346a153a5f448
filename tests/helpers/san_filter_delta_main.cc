// san_filter_delta_main.cc -- TEST INFRASTRUCTURE: the host side of FilterSet::apply_delta_batch under the sanitizers.
//
// The REAL filter_set.cc and filter_delta.cc are linked against the model of the HIP runtime with virtual devices and
// asynchronous streams (hip_virtual.cc) and host models of the filter kernels below, which read and write THROUGH the device
// pointers the host code handed them, at the moment the stream reaches them.  Several threads derive batches of filters on
// 1 to 3 devices (a device listed twice, as logical shards do) and chain them; every bitmap and every count is compared with
// a host model, the bases must stay as they were, argument errors must leave nothing behind.  Under -fsanitize=thread a
// staging block reused while its copy is in flight is a data race, under -fsanitize=address an overrun of the staging block
// or of a bitmap is a heap overflow (tests/test_filter_delta_abi.py builds both).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <random>
#include <thread>

#include "filter_set.hpp"
#include "hip_virtual.hpp"
#include "kernels.hpp"

namespace vk {
// ---- filter_build.hip as host models on the virtual streams
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
hipError_t launch_filter_set_runs(uint64_t *, uint64_t, const uint64_t *, uint64_t, unsigned long long *, hipStream_t) { return hipErrorNotSupported; }   // (not used here)
hipError_t launch_filter_popcount(const uint64_t *bits, uint64_t words, unsigned long long *d_out, hipStream_t s) {
  hipv::launch(s, "filter_popcount_kernel", {{bits, (size_t)words * 8, "bits"}, {d_out, 8, "count"}}, [=] {
    for (uint64_t i = 0; i < words; ++i) *d_out += (unsigned long long)__builtin_popcountll(bits[i]);
  });
  return hipSuccess;
}
hipError_t launch_filter_combine(uint64_t *, const uint64_t *, const uint64_t *, uint64_t, uint32_t, unsigned long long *, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_filter_combine_batch(const uint64_t *, uint32_t, uint64_t, unsigned long long *, hipStream_t) { return hipErrorNotSupported; }

static void check_local(hipStream_t s, const char *kernel, const void *p, size_t bytes, uint32_t item) {
  if (hipv::memory_device(p, bytes) != hipv::stream_device(s)) {
    fprintf(stderr, "VIOLATION %s: item %u names memory of another device (or past its block)\n", kernel, item);
    abort();
  }
}
hipError_t launch_filter_delta_copy(const uint64_t *d_items, uint32_t n, uint64_t max_dst_words, hipStream_t s) {
  hipv::launch(s, "filter_delta_copy_kernel", {{d_items, (size_t)n * kFilterDeltaItemWords * 8, "items"}}, [=] {
    for (uint32_t i = 0; i < n; ++i) {
      const uint64_t *t = d_items + (size_t)i * kFilterDeltaItemWords;
      uint64_t *dst = reinterpret_cast<uint64_t *>(t[0]);
      const uint64_t *base = reinterpret_cast<const uint64_t *>(t[1]);
      const uint64_t base_words = t[2], dst_words = t[3], nbits = t[4];
      if (dst_words > max_dst_words || base_words > dst_words) { fprintf(stderr, "VIOLATION filter_delta_copy_kernel: item %u: words out of range\n", i); abort(); }
      check_local(s, "filter_delta_copy_kernel", dst, (size_t)(dst_words + 1) * 8, i);
      if (base) check_local(s, "filter_delta_copy_kernel", base, (size_t)base_words * 8, i);
      for (uint64_t w = 0; w < dst_words; ++w) dst[w] = w < base_words ? base[w] : 0;
      if (dst_words && nbits % 64) dst[dst_words - 1] &= ~0ull >> (64 - nbits % 64);
      dst[dst_words] = 0;
    }
  });
  return hipSuccess;
}
hipError_t launch_filter_delta_apply(const uint64_t *d_items, const uint64_t *d_recs, uint64_t n_recs, int set, unsigned long long *d_counts, hipStream_t s) {
  if (n_recs == 0) return hipSuccess;
  hipv::launch(s, "filter_delta_apply_kernel", {{d_recs, (size_t)n_recs * 8, "records"}}, [=] {
    for (uint64_t r = 0; r < n_recs; ++r) {
      const uint32_t item = (uint32_t)(d_recs[r] >> kFilterDeltaLabelBits);
      const uint64_t label = d_recs[r] & (((uint64_t)1 << kFilterDeltaLabelBits) - 1);
      const uint64_t *t = d_items + (size_t)item * kFilterDeltaItemWords;
      check_local(s, "filter_delta_apply_kernel", t, kFilterDeltaItemWords * 8, item);
      check_local(s, "filter_delta_apply_kernel", d_counts + item, 8, item);
      if (label >= t[4]) continue;
      uint64_t *dst = reinterpret_cast<uint64_t *>(t[0]);
      const uint64_t b = 1ull << (label & 63);
      if (set && !(dst[label >> 6] & b)) { dst[label >> 6] |= b; d_counts[item] += 1; }
      if (!set && (dst[label >> 6] & b)) { dst[label >> 6] &= ~b; d_counts[item] -= 1; }
    }
  });
  return hipSuccess;
}
}  // namespace vk

namespace {
std::atomic<uint64_t> g_bad{0};
#define CHECK(cond, ...)                                                                          \
  do {                                                                                            \
    if (!(cond)) { g_bad.fetch_add(1); fprintf(stderr, "BAD [%s] ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
  } while (0)

using Bits = std::vector<bool>;
void expect(const vk::FilterSet &f, const Bits &model, const char *what) {
  uint64_t count = 0;
  std::vector<uint64_t> want((model.size() + 63) / 64 + 2, 0), got(want.size(), ~0ull);
  for (size_t i = 0; i < model.size(); ++i)
    if (model[i]) { want[i >> 6] |= 1ull << (i & 63); ++count; }
  CHECK(f.read(got.data(), got.size()).ok(), "%s: read", what);
  CHECK(got == want, "%s: bitmap differs (nbits %zu)", what, model.size());
  CHECK(f.nbits() == model.size() && f.allowed() == count, "%s: nbits %llu / %zu allowed %llu / %llu", what, (unsigned long long)f.nbits(), model.size(),
        (unsigned long long)f.allowed(), (unsigned long long)count);
}

void worker(const std::vector<int> &devs, uint64_t seed, int rounds) {
  std::mt19937_64 rng(seed);
  auto below = [&](uint64_t n) { return n ? rng() % n : 0; };
  // two lineages, derived together in every batch (plus an item without a base, and one base used twice)
  std::shared_ptr<vk::FilterSet> f[2];
  Bits m[2];
  for (int j = 0; j < 2; ++j) {
    const uint64_t nbits = j ? 70 : 5003;
    std::vector<uint64_t> ids(below(400));
    for (uint64_t &id : ids) id = below(nbits + 20);
    m[j].assign(nbits, false);
    for (uint64_t id : ids)
      if (id < nbits) m[j][id] = true;
    CHECK(vk::FilterSet::build(devs, nbits, ids.data(), ids.size(), nullptr, 0, nullptr, &f[j]).ok(), "build");
    if (!f[j]) return;
    expect(*f[j], m[j], "base");
  }
  for (int r = 0; r < rounds; ++r) {
    const int n = 4;
    const vk::FilterSet *bases[n] = {f[0].get(), f[1].get(), nullptr, f[0].get()};
    const Bits *bm[n] = {&m[0], &m[1], nullptr, &m[0]};
    std::vector<uint64_t> set[n], clr[n];
    vk::FilterSet::Delta items[n];
    Bits want[n];
    for (int i = 0; i < n; ++i) {
      const uint64_t base_bits = bases[i] ? bases[i]->nbits() : 0;
      const uint64_t grow[] = {0, 0, 1, 63, 64, 65, 700};
      const uint64_t nbits = base_bits + grow[below(7)] + (bases[i] ? 0 : 1 + below(300));
      set[i].resize(below(300));
      clr[i].resize(below(300));
      for (uint64_t &v : set[i]) v = below(nbits + 30);
      for (uint64_t &v : clr[i]) v = below(nbits + 30);
      if (!set[i].empty() && !clr[i].empty()) clr[i][0] = set[i][0];   // in both lists: ends up set
      want[i].assign(nbits, false);
      if (bm[i]) std::copy(bm[i]->begin(), bm[i]->end(), want[i].begin());
      for (uint64_t v : clr[i]) if (v < nbits) want[i][v] = false;
      for (uint64_t v : set[i]) if (v < nbits) want[i][v] = true;
      items[i] = vk::FilterSet::Delta{bases[i], nbits, clr[i].data(), clr[i].size(), set[i].data(), set[i].size()};
    }
    std::vector<std::shared_ptr<vk::FilterSet>> out;
    vk::Status st = vk::FilterSet::apply_delta_batch(devs, items, n, &out);
    CHECK(st.ok() && out.size() == (size_t)n, "apply_delta_batch: %s", st.msg.c_str());
    if (!st.ok()) return;
    for (int i = 0; i < n; ++i) expect(*out[i], want[i], "derived");
    expect(*f[0], m[0], "base after the call");
    expect(*f[1], m[1], "base after the call");
    // one bad item (below its base) fails the whole call before any device work and leaves nothing behind
    if (f[0]->nbits() > 0) {
      vk::FilterSet::Delta bad[2] = {items[1], items[0]};
      bad[1].nbits = f[0]->nbits() - 1;
      std::vector<std::shared_ptr<vk::FilterSet>> none;
      CHECK(!vk::FilterSet::apply_delta_batch(devs, bad, 2, &none).ok() && none.empty(), "a shrinking item must fail the batch");
    }
    f[0] = out[0]; m[0] = want[0];   // the lineages go on from the derived filters; the old ones are released here
    f[1] = out[1]; m[1] = want[1];
  }
  std::shared_ptr<vk::FilterSet> one;
  const uint64_t ids[3] = {0, 5, 1ull << 50};
  CHECK(vk::FilterSet::apply_delta(devs, vk::FilterSet::Delta{nullptr, 6, nullptr, 0, ids, 3}, &one).ok() && one && one->allowed() == 2, "single apply_delta");
  CHECK(!vk::FilterSet::apply_delta(devs, vk::FilterSet::Delta{nullptr, 6, nullptr, 2, nullptr, 0}, &one).ok(), "a NULL list with a length");
}
}  // namespace

int main() {
  hipv::set_device_count(3);
  for (int a = 0; a < 3; ++a)   // (what the sharded index does before its first filter: FilterSet::build copies peer to peer)
    for (int b = 0; b < 3; ++b)
      if (a != b) { (void)hipSetDevice(a); (void)hipDeviceEnablePeerAccess(b, 0); }
  const std::vector<std::vector<int>> worlds = {{0}, {1, 2}, {2, 0, 1, 0}};
  for (const auto &devs : worlds) {
    std::vector<std::thread> ts;
    for (int t = 0; t < 4; ++t) ts.emplace_back(worker, devs, 1000 + 17 * t + devs.size(), 12);
    for (auto &t : ts) t.join();
  }
  std::vector<std::shared_ptr<vk::FilterSet>> none;
  CHECK(vk::FilterSet::apply_delta_batch({0}, nullptr, 0, &none).ok(), "n == 0");
  CHECK(!vk::FilterSet::apply_delta_batch({0}, nullptr, 70000, &none).ok(), "n > 65535");
  for (const std::string &v : hipv::take_violations()) { fprintf(stderr, "VIOLATION %s\n", v.c_str()); g_bad.fetch_add(1); }
  printf("worlds=%zu kernels=%llu bad=%llu\n", worlds.size(), (unsigned long long)hipv::kernels(), (unsigned long long)g_bad.load());
  return g_bad.load() ? 1 : 0;
}
