// san_prefilter_submit_main.cc -- TEST INFRASTRUCTURE (tests/test_prefilter_submit_cpu.py): the pre-filter lane of
// csrc/dispatcher.hpp (Dispatcher::submit_labels -> Index::search_labels_batch) under ASAN / UBSAN and TSAN, host only.
//
// The REAL dispatcher, the real Index::search_labels_batch (csrc/prefilter_batch.cc: candidates -> the heap rule) and
// index_common.cc are linked against the virtual HIP layer (hip_virtual.cc); the index is a fake whose device stage
// (prefilter_candidates) computes every known key's distance on the host -- a superset of what the select kernel hands
// back, which the heap rule is exact over (prefilter_host.hpp).  Several threads submit requests -- some bring ONE shared
// list (same pointer and length: the runner's shared path), some their own list, which they free the moment their completion
// fires -- with callbacks and through the bulk hook, against a shallow queue (VK_ERR_BUSY, retried), and an index that is
// destroyed with requests still queued.  Every answer must be prefilter_heap_rule's over the caller's list.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <thread>
#include <vector>

#include "dispatcher.hpp"

namespace vk {
// the kernels' launchers and the single call's path: linked by prefilter_batch.cc, never reached from a fake index
uint32_t prefilter_tiles(uint64_t entries) { return (uint32_t)((entries + 63) / 64); }
hipError_t launch_prefilter_distance(const PrefilterDistArgs &, bool, bool, hipStream_t) { abort(); }
hipError_t launch_prefilter_select(const PrefilterSelectArgs &, hipStream_t) { abort(); }
Status Index::search_labels(const float *, uint64_t, const uint64_t *, uint64_t, float *, uint64_t *, uint64_t *) { abort(); }
}  // namespace vk

namespace {

vk::Status labels_batch(vk::Index *ix, const float *q, uint64_t nq, uint64_t k, const uint64_t *labels, const uint64_t *lb, uint64_t n, float *d,
                        uint64_t *l, uint64_t *on) {
  return ix->search_labels_batch(q, nq, k, labels, lb, n, d, l, on);   // what vk_index.cc hands the dispatcher
}

constexpr uint64_t kKnown = 5000;   // labels below this are "in the index"
float fake_distance(const float *q, uint64_t label) { return (float)((label * 37 + (uint64_t)q[0] * 11) % 101) + q[1]; }

struct LabelIndex final : vk::Index {
  explicit LabelIndex(const vk_index_params &p) : Index(p) {}
  std::atomic<uint64_t> batches{0}, queries{0}, shared_batches{0}, max_batch{0};
  vk::Status prefilter_candidates(const float *queries_, uint64_t nq, uint64_t, const uint64_t *labels, const uint64_t *list_begin,
                                  uint64_t n_labels, vk::PrefilterCands *out) override {
    batches += 1;
    queries += nq;
    if (!list_begin) shared_batches += 1;
    uint64_t m = max_batch.load();
    while (nq > m && !max_batch.compare_exchange_weak(m, nq)) {}
    std::this_thread::sleep_for(std::chrono::microseconds(150));   // a device pass takes a while: requests pile up behind it
    out->reset(nq, false);
    for (uint64_t q = 0; q < nq; ++q) {
      const uint64_t lo = list_begin ? list_begin[q] : 0, hi = list_begin ? list_begin[q + 1] : n_labels;
      for (uint64_t i = lo; i < hi; ++i)
        if (labels[i] < kKnown) out->items.push_back(vk::PrefilterCand{i, fake_distance(queries_ + q * params_.dim, labels[i])});
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
  void filter_devices(std::vector<int> *out) const override { out->clear(); }
};

constexpr uint64_t kK = 5;
// one request: owns its query copy's source, its list (unless it uses the shared one) and its outputs
struct Request {
  float q[4];
  std::unique_ptr<uint64_t[]> own;
  const uint64_t *labels = nullptr;
  uint64_t n = 0;
  float d[kK];
  uint64_t l[kK], out_n = 99;
  std::atomic<int> fired{0};
  int status = -1;
  std::atomic<int> *bad = nullptr;
  std::atomic<uint64_t> *completed = nullptr;
};

void verify_and_release(Request *r, int status) {
  r->status = status;
  float wd[kK];
  uint64_t wl[kK], wn = 0;
  std::vector<float> dist(r->n);
  std::vector<uint64_t> lab(r->n);
  for (uint64_t i = 0; i < r->n; ++i) {
    lab[i] = r->labels[i] < kKnown ? r->labels[i] : ~0ull;
    dist[i] = fake_distance(r->q, r->labels[i]);
  }
  vk::prefilter_heap_rule(dist.data(), lab.data(), r->n, kK, wd, wl, &wn);
  bool ok = status == 0 && r->out_n == wn;
  for (uint64_t i = 0; ok && i < wn; ++i) ok = r->d[i] == wd[i] && r->l[i] == wl[i];
  if (!ok) r->bad->fetch_add(1);
  r->own.reset();   // the caller's list dies with the completion
  if (r->fired.fetch_add(1) != 0) r->bad->fetch_add(1);   // exactly once
  r->completed->fetch_add(1);
}
void on_done(void *user, int status) { verify_and_release(static_cast<Request *>(user), status); }
void on_bulk(void *, void *const *users, const int *statuses, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) verify_and_release(static_cast<Request *>(users[i]), statuses[i]);
}

int run(int threads, int per_thread, uint32_t max_batch, uint64_t depth, bool bulk, bool destroy_early) {
  vk_index_params p{};
  p.struct_size = sizeof p;
  p.dim = 4;
  p.algo = VK_ALGO_FLAT;
  LabelIndex ix(p);
  std::atomic<int> bad{0};
  std::atomic<uint64_t> completed{0}, accepted{0}, busy{0};
  std::vector<uint64_t> shared(300);
  for (size_t i = 0; i < shared.size(); ++i) shared[i] = (i * 7919) % (kKnown + 600);
  std::vector<std::vector<std::unique_ptr<Request>>> reqs(threads);
  {
    auto co = std::make_unique<vk::Dispatcher>(&ix);
    co->set_labels_batch(&labels_batch);
    co->configure(max_batch, 500);
    co->set_queue_depth(depth);
    if (bulk) co->set_batch_done(&on_bulk, nullptr);
    std::vector<std::thread> ts;
    for (int t = 0; t < threads; ++t)
      ts.emplace_back([&, t] {
        for (int i = 0; i < per_thread; ++i) {
          auto r = std::make_unique<Request>();
          const int id = t * per_thread + i;
          r->q[0] = (float)(id % 50); r->q[1] = 0.25f * (float)(id % 3); r->q[2] = r->q[3] = 0.f;
          r->bad = &bad;
          r->completed = &completed;
          if (id % 3 == 0) {   // the shared list: same pointer, same length
            r->labels = shared.data();
            r->n = shared.size();
          } else {
            r->n = (uint64_t)(id % 40);   // (0: an empty list)
            r->own = std::make_unique<uint64_t[]>(r->n ? r->n : 1);
            for (uint64_t j = 0; j < r->n; ++j) r->own[j] = ((uint64_t)id * 131 + j * 17) % (kKnown + 900);
            r->labels = r->own.get();
          }
          Request *raw = r.get();
          reqs[t].push_back(std::move(r));
          float q[4] = {raw->q[0], raw->q[1], raw->q[2], raw->q[3]};   // the submitted query is a temporary: it is copied
          for (;;) {
            vk::Status st = co->submit_labels(q, kK, raw->labels, raw->n, raw->d, raw->l, &raw->out_n, &on_done, raw);
            if (st.ok()) { accepted += 1; break; }
            if (st.code != VK_ERR_BUSY) { bad += 1; break; }
            busy += 1;
            std::this_thread::yield();
          }
          q[0] = -1.f;
        }
      });
    for (auto &t : ts) t.join();
    if (!destroy_early)
      while (completed.load() < accepted.load()) std::this_thread::yield();
    co.reset();   // destroy answers what is still queued and waits for the callbacks
  }
  if (completed.load() != accepted.load()) bad += 1;
  if (accepted.load() != (uint64_t)threads * per_thread) bad += 1;
  if (ix.queries.load() != accepted.load()) bad += 1;
  if (ix.max_batch.load() > max_batch) bad += 1;
  for (auto &v : reqs)
    for (auto &r : v)
      if (r->fired.load() != 1) bad += 1;
  printf("threads=%d accepted=%llu busy=%llu batches=%llu shared_batches=%llu max_batch=%llu bad=%d\n", threads,
         (unsigned long long)accepted.load(), (unsigned long long)busy.load(), (unsigned long long)ix.batches.load(),
         (unsigned long long)ix.shared_batches.load(), (unsigned long long)ix.max_batch.load(), bad.load());
  return bad.load();
}

// eight submissions of the same (pointer, length) from one thread: ONE batch, over the shared list
int shared_burst() {
  vk_index_params p{};
  p.struct_size = sizeof p;
  p.dim = 4;
  p.algo = VK_ALGO_HNSW;
  LabelIndex ix(p);
  std::atomic<int> bad{0};
  std::atomic<uint64_t> completed{0};
  std::vector<uint64_t> list(100);
  for (size_t i = 0; i < list.size(); ++i) list[i] = i * 61;
  std::vector<std::unique_ptr<Request>> reqs;
  vk::Dispatcher co(&ix);
  co.set_labels_batch(&labels_batch);
  co.configure(8, 1000000);
  for (int i = 0; i < 8; ++i) {
    auto r = std::make_unique<Request>();
    r->q[0] = (float)i; r->q[1] = r->q[2] = r->q[3] = 0.f;
    r->labels = list.data();
    r->n = list.size();
    r->bad = &bad;
    r->completed = &completed;
    reqs.push_back(std::move(r));
  }
  for (auto &r : reqs)
    if (!co.submit_labels(r->q, kK, r->labels, r->n, r->d, r->l, &r->out_n, &on_done, r.get()).ok()) bad += 1;
  while (completed.load() < 8) std::this_thread::yield();
  // (a sanitizer build may start its runner slowly and split the burst: whatever was formed must have been shared)
  if (ix.shared_batches.load() != ix.batches.load() || ix.queries.load() != 8 || co.queries() != 8 || co.submitted() != 8) bad += 1;
  return bad.load();
}

}  // namespace

int main(int argc, char **argv) {
  const int scale = argc > 1 ? atoi(argv[1]) : 1;
  int bad = 0;
  bad += run(8, 60 * scale, 8, 100000, false, false);
  bad += run(6, 60 * scale, 16, 100000, true, false);    // completions through the bulk hook
  bad += run(8, 40 * scale, 4, 3, false, false);         // a shallow queue: VK_ERR_BUSY, retried
  bad += run(4, 30 * scale, 64, 100000, false, true);    // destroyed with requests queued
  bad += run(4, 30 * scale, 64, 100000, true, true);
  bad += shared_burst();
  printf("bad=%d\n", bad);
  return bad ? 1 : 0;
}
