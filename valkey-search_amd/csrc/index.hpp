// index.hpp -- the objects behind the C ABI (include/vk_index.h).
//
//   FlatIndex  stands in for hnswlib::BruteforceSearch<float>  (third_party/hnswlib/bruteforce.h)
//   HnswIndex  stands in for hnswlib::HierarchicalNSW<float>   (third_party/hnswlib/hnswalg.h)
// Host side keeps what the reference keeps on the host (label<->slot maps, the HNSW
// graph's authoritative copy); the device holds the row table (row_store.hpp) and, for
// HNSW, a fixed-stride mirror of the link lists, and answers the searches.
#pragma once
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <unordered_map>
#include <vector>

#include "../../include/vk_index.h"
#include "filter_set.hpp"
#include "kernels.hpp"
#include "label_map_delta_host.hpp"
#include "options.hpp"
#include "prefilter_handle_host.hpp"
#include "prefilter_host.hpp"
#include "row_store.hpp"

namespace vk {

// grow-only device / pinned buffers
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  Status ensure(size_t bytes);
  void release();
  template <class T> T *as() { return reinterpret_cast<T *>(p); }
};
struct PinBuf {
  void *p = nullptr;
  size_t cap = 0;
  Status ensure(size_t bytes);
  void release();
  template <class T> T *as() { return reinterpret_cast<T *>(p); }
};

// The device label map of one index on one device (label_map.hip; option prefilter-device-resolve): label -> slot for the
// batched pre-filter search.  Built whole, lazily, on the stream of the first batch that wants it, and tagged with what it was
// built from: the index's publication counter and published count.  A batch that finds another tag rebuilds it -- a flush
// stands between the two, and a flush holds the index's lock exclusively, so no kernel of an earlier batch still reads the
// table.  Callers hold the index's shared lock (ready) or its exclusive lock (release).
// With option prefilter-label-map-upkeep = 1 (LabelMapUpkeep::on) a batch that finds another tag does not rebuild: the labels
// the write phase touched (touched(), recorded by the index wherever a label's answer can change) are turned into records
// against the index's own truth and applied on the device (label_map_apply_kernel); label_map_delta_host.hpp has the rules
// for when a rebuild is due all the same, and the check of the counters behind every apply.
struct LabelMapUpkeep {
  bool on = false;
  uint64_t delta_max = 65536;                   // option prefilter-label-map-delta-max
  uint64_t live = 0;                            // labels the index answers under this publication (HNSW: without tombstones)
  std::function<uint32_t(uint64_t)> truth;      // label -> its slot now, or kLabelMapNone: the host resolve's own lookup
};

class DeviceLabelMap {
 public:
  ~DeviceLabelMap() { buf_.release(); delta_.release(); }
  // false = no map for this publication (no room on the device, or the build's failure word was not zero): the batch
  // resolves on the host.  links0 != nullptr: HNSW, tombstoned nodes stay out.
  // budget: most bytes the table may take (option prefilter-label-map-bytes); read when the map is (re)built
  bool ready(uint64_t epoch, uint32_t count, const uint64_t *d_labels, const uint32_t *d_links0, uint32_t l0_stride, uint64_t budget,
             hipStream_t s, LabelMapTable *out, const LabelMapUpkeep *up = nullptr);
  void release();   // ... and the touched set cleared: the next build starts from the published labels
  uint64_t bytes() const { return bytes_.load(std::memory_order_relaxed); }
  uint64_t builds() const { return builds_.load(std::memory_order_relaxed); }
  LabelTouchSet &touched() { return touched_; }
  void stats(vk_label_map_stats *out);          // (struct_size is the caller's business)
  // vk_index_label_map_read: the live (label, slot) pairs of the table as it stands (after ready())
  Status read(uint64_t *out_labels, uint32_t *out_slots, uint64_t cap, uint64_t *out_n);

 private:
  bool rebuild(uint64_t epoch, uint32_t count, const uint64_t *d_labels, const uint32_t *d_links0, uint32_t l0_stride, uint64_t budget,
               hipStream_t s, uint64_t headroom);
  std::mutex mu_;
  DevBuf buf_, delta_;                          // the table | the records of an apply launch
  LabelMapTable t_{};
  uint64_t epoch_ = 0;
  uint32_t count_ = 0;
  bool tagged_ = false, usable_ = false;
  uint64_t used_ = 0, live_ = 0;                // keys in the table (dead ones included) | entries with a slot
  LabelTouchSet touched_;
  std::atomic<uint64_t> bytes_{0}, builds_{0};
  std::atomic<uint64_t> delta_batches_{0}, delta_records_{0}, claimed_{0}, revived_{0}, killed_{0}, moved_{0}, delta_mismatches_{0},
      rebuilds_forced_{0};
};

// Results this small are written by the kernels straight into the pinned host buffers (hipHostMalloc memory is
// mapped into the device's address space): a one-at-a-time query pays no device-to-host copy calls, only the
// stream synchronisation.  Larger results go through device buffers and one copy each (PCIe bandwidth, not latency).
constexpr uint64_t kZeroCopyEntries = 4096;   // nq * k

// Per-call resources: a stream plus scratch, so that concurrent reader threads
// (search.cc:886-910 schedules one query per reader-pool thread) do not serialise.
struct SearchCtx {
  hipStream_t stream = nullptr;
  DevBuf d_q, d_part_d, d_part_l, d_out_d, d_out_l, d_out_n, d_allow, d_idx, d_tmp, d_stats, d_sync, d_pool, d_pool2, d_redo,
      d_fq16, d_fthr, d_fcnt, d_fcand, d_fspill, d_fsmax, d_fpart_d, d_fpart_l,   // candidate filter (flat_filter.hip)
      d_allow_tab,                                             // per-query filter table + the bitmaps behind it
      d_mask,                                                  // HNSW node masks: build items + counts, per-query mask table
      d_lk_dist, d_lk_work;                                    // FLAT k > 1024 in one pass: distances | state, hand-back lists, histograms
  // what the work enqueued last must outlive although its caller may let go of it (node masks of a device-buffer search);
  // replaced by the context's next user
  std::vector<std::shared_ptr<const void>> keep_alive;
  PinBuf h_q, h_out_d, h_out_l, h_out_n, h_tmp, h_idx, h_cancel, h_lk;
  // per-member cancellation (SearchRequest::member_cancel): the words the kernel polls follow the batch word in h_cancel
  static constexpr size_t kMemberCancelOffset = 16;   // in u32 words
  Status wait(const volatile int *caller_flag, const volatile uint32_t *member_cancel, uint64_t nq);
  // In-kernel cancellation: the caller's flag (any host memory) cannot be read by the device, so the thread that
  // waits for the stream polls it and raises the context's own word in pinned memory, which the kernels poll
  // (FlatScanArgs::cancel).  arm_cancel: allocate + clear, returns the device-visible word (nullptr when the call
  // carries no flag); wait: hipStreamSynchronize, or with a flag a poll of stream and flag.
  Status arm_cancel(const volatile int *caller_flag, const uint32_t **device_word, uint64_t n_members = 0,
                    const uint32_t **member_words = nullptr);
  Status wait(const volatile int *caller_flag);
  // A device-buffer search (vk_index_search_batch_device) returns with its kernels still in flight on the CALLER's
  // stream and gives the context back: `busy` is recorded behind that work, and whoever leases the context next makes
  // its own stream wait for it before touching the scratch (begin_on) -- no host wait, and no two calls ever share
  // scratch that is live.  (DevBuf::ensure growing a buffer frees the old one with hipFree, which waits for the device.)
  hipEvent_t busy = nullptr;
  bool has_busy = false;
  // kernel-level timing of the candidate filter for vk_index_stats (bench.py's roofline): event pairs around its
  // launches, drained into the index's totals when a pair is reused or when the statistics are read
  struct TimedPair { hipEvent_t t0 = nullptr, t1 = nullptr; bool pending = false; };
  TimedPair timed[32];
  uint32_t timed_next = 0;
  Status begin_on(hipStream_t s);   // order the work about to be enqueued on `s` behind the context's previous user
  Status end_async(hipStream_t s);  // the work enqueued on `s` is the context's last user from now on
  ~SearchCtx();
};

class CtxPool {
 public:
  explicit CtxPool(int device, size_t max_ctx = 16) : device_(device), max_(max_ctx) {}
  ~CtxPool();
  // `on` = the stream the lease holder will enqueue on (nullptr = the context's own): it is ordered behind the
  // context's previous asynchronous user (SearchCtx::busy)
  SearchCtx *acquire(hipStream_t on = nullptr);
  void release(SearchCtx *c);
  // every context that is not leased right now
  template <class F> void for_each_free(F &&f) {
    std::lock_guard<std::mutex> lk(mu_);
    for (SearchCtx *c : free_) f(c);
  }

 private:
  int device_;
  size_t max_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<SearchCtx *> free_;
  std::vector<std::unique_ptr<SearchCtx>> all_;
};

struct CtxLease {
  CtxPool &pool;
  SearchCtx *ctx;
  explicit CtxLease(CtxPool &p, hipStream_t on = nullptr) : pool(p), ctx(p.acquire(on)) {}
  ~CtxLease() { pool.release(ctx); }
};

// The caller's cancellation word (BaseCancellationFunctor, hnswlib.h:153-157; the reference's cancel::Token is an atomic
// bool) is written by another thread while searches read it: a relaxed atomic load, not a plain read of a volatile int.
inline bool cancel_raised(const volatile int *flag) {
  return flag != nullptr && __atomic_load_n(const_cast<const int *>(flag), __ATOMIC_RELAXED) != 0;
}

struct SearchRequest {
  const float *queries = nullptr;   // host or device, [nq][dim] (host) / [nq][stride_f] padded (device)
  // host entry points only: one pointer per query instead of `queries` (the dispatcher's batches are made of single-query
  // calls whose vectors still lie in their callers' buffers; they are gathered straight into the pinned staging block)
  const float *const *query_tab = nullptr;
  uint64_t nq = 0, k = 0, ef = 0;
  const uint64_t *allow_bits = nullptr;
  uint64_t allow_nbits = 0;
  // one filter per query (host entry points: host arrays of host pointers, nullptr entry = unfiltered); overrides
  // allow_bits.  The reference builds its filter per FT.SEARCH (search.cc:103-134), so a batch of coalesced hybrid
  // queries carries as many bitmaps as queries.
  const uint64_t *const *allow_tab = nullptr;
  const uint64_t *allow_nbits_tab = nullptr;
  // device-resident filters (filter_set.hpp; host entry points): one for the whole batch, or one per query (a nullptr
  // entry = that query's allow_tab entry, or no filter).  They override allow_bits / allow_tab and are never uploaded.
  const FilterSet *filter = nullptr;
  const FilterSet *const *filter_tab = nullptr;
  const volatile int *cancel_flag = nullptr;
  bool partial_ok = true;
  // dispatcher batches: one host word per member, raised when THAT member's token goes up.  HNSW relays it to the wave
  // working on the member's query, which stops like the reference's loop does (hnswalg.h:400-402); FLAT ignores it (a
  // row pass costs the same with or without the member).
  const volatile uint32_t *member_cancel = nullptr;
  // search_device only: a device-visible cancellation word the caller maintains itself (the sharded index relays one
  // host flag to the kernels of every shard through it)
  const uint32_t *cancel_word = nullptr;
};

class Index {
 public:
  virtual ~Index() = default;
  const vk_index_params &params() const { return params_; }
  bool l2() const { return params_.metric == VK_METRIC_L2; }

  virtual Status add(uint64_t label, const float *row) = 0;
  virtual Status add_batch(const uint64_t *labels, const float *rows, uint64_t n) = 0;
  virtual Status remove(uint64_t label) = 0;
  virtual Status resize(uint64_t new_max) = 0;
  virtual Status set_ef(uint32_t ef) = 0;
  virtual Status flush() = 0;
  // host buffers in/out
  virtual Status search(const SearchRequest &rq, float *out_dist, uint64_t *out_label, uint64_t *out_n) = 0;
  // device buffers in/out, enqueued on `stream` (nullptr = internal) without host sync
  virtual Status search_device(const SearchRequest &rq, float *d_out_dist, uint64_t *d_out_label,
                               uint32_t *d_out_n, hipStream_t stream) = 0;
  // distance of every listed label that the index holds (found[i] = 1), in list order: the device half of the
  // pre-filter path (ComputeDistanceFromRecordImpl per key, vector_base.cc:509-530)
  virtual Status label_distances(const float *query, const uint64_t *labels, uint64_t n, float *out_dist, uint8_t *found) = 0;
  // ... and its host half: AddPrefilteredKey's heap over those distances, in key order
  Status search_labels(const float *query, uint64_t k, const uint64_t *labels, uint64_t n, float *out_dist,
                       uint64_t *out_label, uint64_t *out_n);
  // vk_index_search_labels_batch: nq pre-filter searches, each answer bit for bit search_labels' (prefilter_batch.cc).  The
  // device stage is prefilter_candidates -- the shard-level call, candidates instead of an answer: per query every entry at
  // or below its k-th smallest distance, in position order (positions index `labels`), or the mark "take the per-query
  // path".  An index without a device stage marks every query.
  Status search_labels_batch(const float *queries, uint64_t nq, uint64_t k, const uint64_t *labels, const uint64_t *list_begin,
                             uint64_t n_labels, float *out_dist, uint64_t *out_label, uint64_t *out_n);
  virtual Status prefilter_candidates(const float *, uint64_t nq, uint64_t, const uint64_t *, const uint64_t *, uint64_t,
                                      PrefilterCands *out) {
    out->reset(nq, true);
    return Status::Ok();
  }
  virtual Status prefilter_stats(vk_prefilter_stats_v2 *out) {   // (a sharded index sums its shards)
    pf_.read(out);
    label_map_counters(&out->label_map_builds, &out->label_map_bytes);
    return Status::Ok();
  }
  virtual void label_map_counters(uint64_t *builds, uint64_t *bytes) { *builds = 0; *bytes = 0; }   // the index's DeviceLabelMap
  // vk_index_search_filter_exact_batch: exact kNN among the rows filter handles admit, each answer bit for bit search_labels'
  // over the handle's ascending label list (prefilter_handle.cc).  tab[q] is query q's filter; consecutive queries with the
  // same one form a run, and a run is one handle_candidates -- the shard-level call: per query every entry at or below its
  // k-th smallest distance with its label, in label order, or the mark "take the list path".  An index without a device
  // stage marks every query.
  Status search_filter_exact_batch(const float *queries, uint64_t nq, uint64_t k, const FilterSet *const *tab, float *out_dist,
                                   uint64_t *out_label, uint64_t *out_n);
  virtual Status handle_candidates(const float *, uint64_t nq, uint64_t, const FilterSet &, HandleCands *out) {
    out->reset(nq, true);
    return Status::Ok();
  }
  virtual Status filter_exact_stats(vk_filter_exact_stats *out) {   // (a sharded index adds its shards' device counters)
    hx_.read(out);
    return Status::Ok();
  }
  // vk_index_large_k_stats (FLAT; a sharded index sums its shards, HNSW answers zeros)
  virtual Status large_k_stats(vk_flat_large_k_stats *out) {
    memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    return Status::Ok();
  }
  // vk_index_label_map_stats (a sharded index sums its shards) / vk_index_label_map_read (a plain index only)
  virtual Status label_map_stats(vk_label_map_stats *out) {
    memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    return Status::Ok();
  }
  virtual Status label_map_read(uint64_t *, uint32_t *, uint64_t, uint64_t *) {
    return Status::Err(VK_ERR_INVALID, "the label map is read from a plain index");
  }
  virtual void release_label_map() {}   // ... given back (a sharded index's resize: its shards' maps)
  // sharded index: its shards (vk_index_shard_device_rows / _commit_device_rows address one of them)
  // the devices a filter of this index must be resident on (FilterSet::build)
  virtual void filter_devices(std::vector<int> *out) const = 0;
  virtual uint32_t shard_count() const { return 0; }
  virtual Status shard_device_rows(uint32_t, uint64_t, void **, uint64_t *) { return Status::Err(VK_ERR_INVALID, "not a sharded index"); }
  virtual Status shard_commit_device_rows(uint32_t, uint64_t, const uint64_t *) { return Status::Err(VK_ERR_INVALID, "not a sharded index"); }
  virtual Status shard_stats(uint32_t, vk_index_stats *) { return Status::Err(VK_ERR_INVALID, "not a sharded index"); }
  virtual Status distance(uint64_t label, const float *query, float *out) = 0;
  virtual Status get_row(uint64_t label, float *out) = 0;
  virtual Status contains(uint64_t label, bool *found) = 0;
  virtual Status stats(vk_index_stats *out) = 0;
  virtual uint64_t filter_image_bytes() { return 0; }   // vk_index_filter_image_bytes (FLAT)
  // vk_index_node_mask_stats / _read (HNSW; a sharded index sums / refuses)
  virtual Status node_mask_stats(vk_node_mask_stats *out) {
    const uint64_t sz = out->struct_size;
    memset(out, 0, sizeof(*out));
    out->struct_size = sz;
    return Status::Ok();
  }
  virtual Status node_mask_read(const FilterSet *, uint64_t *, uint64_t, uint64_t *) {
    return Status::Err(VK_ERR_INVALID, "node masks are read from a plain HNSW index");
  }
  virtual Status device_rows(uint64_t n, void **d_rows, uint64_t *stride_bytes) = 0;
  virtual Status commit_device_rows(uint64_t n, const uint64_t *labels) = 0;
  virtual Status save(vk_write_chunk_fn fn, void *user) = 0;
  // run-time options (options.hpp): vk_index_set_option / vk_index_get_option; a sharded index forwards to its shards
  virtual Status set_option(const char *name, uint64_t value) { return opt_.set(name, value); }
  Status get_option(const char *name, uint64_t *out) const { return opt_.get(name, out); }
  const Options &options() const { return opt_; }

 protected:
  explicit Index(const vk_index_params &p) : params_(p) {
    if (p.shard_ef_pct) opt_.set(kOptShardEfPct, p.shard_ef_pct);
  }
  vk_index_params params_;
  Options opt_;
  // counters of the batched pre-filter search (vk_prefilter_stats)
  struct PrefilterCounters {
    std::atomic<uint64_t> batches{0}, queries{0}, keys{0}, candidates{0}, fallback_queries{0}, candidate_cap{0}, device_resolved_keys{0};
    void read(vk_prefilter_stats_v2 *out) const {
      const uint64_t sz = out->struct_size;
      memset(out, 0, sizeof(*out));
      out->struct_size = sz;
      out->batches = batches.load(std::memory_order_relaxed);
      out->queries = queries.load(std::memory_order_relaxed);
      out->keys = keys.load(std::memory_order_relaxed);
      out->candidates = candidates.load(std::memory_order_relaxed);
      out->fallback_queries = fallback_queries.load(std::memory_order_relaxed);
      out->candidate_cap = candidate_cap.load(std::memory_order_relaxed);
      out->device_resolved_keys = device_resolved_keys.load(std::memory_order_relaxed);
    }
  } pf_;
  // ... and of the exact search from filter handles (vk_filter_exact_stats)
  struct HandleCounters {
    std::atomic<uint64_t> batches{0}, queries{0}, runs{0}, labels_expanded{0}, known_keys{0}, candidates{0}, fallback_queries{0},
        downloaded_runs{0};
    void read(vk_filter_exact_stats *out) const {
      memset(out, 0, sizeof(*out));
      out->struct_size = sizeof(*out);
      out->batches = batches.load(std::memory_order_relaxed);
      out->queries = queries.load(std::memory_order_relaxed);
      out->runs = runs.load(std::memory_order_relaxed);
      out->labels_expanded = labels_expanded.load(std::memory_order_relaxed);
      out->known_keys = known_keys.load(std::memory_order_relaxed);
      out->candidates = candidates.load(std::memory_order_relaxed);
      out->fallback_queries = fallback_queries.load(std::memory_order_relaxed);
      out->downloaded_runs = downloaded_runs.load(std::memory_order_relaxed);
    }
  } hx_;
  // what a leaf's handle_candidates adds after its device stage
  void count_handle_stage(const HandleCands &c, uint64_t expanded, uint64_t known) {
    uint64_t cands = 0;
    for (size_t q = 0; q < c.fallback.size(); ++q)
      if (!c.fallback[q]) cands += c.begin[q + 1] - c.begin[q];
    hx_.labels_expanded.fetch_add(expanded, std::memory_order_relaxed);
    hx_.known_keys.fetch_add(known, std::memory_order_relaxed);
    hx_.candidates.fetch_add(cands, std::memory_order_relaxed);
  }
};

// The device stage of prefilter_candidates on one device, for lists already resolved to row slots (prefilter_batch.cc):
// per chunk of queries one upload (queries, segment tables, slots), K8b, K8c, one download of the hand-back, one
// synchronise.  The caller holds the index's shared lock and the context's lease.
Status prefilter_device_stage(SearchCtx *ctx, const void *d_rows, uint32_t dim, uint32_t stride_f, bool l2, bool bf16, const float *queries,
                              uint64_t k, const PrefilterResolved &r, PrefilterCands *out);
// The same with the label -> slot step on the device (option prefilter-device-resolve): the raw labels are uploaded and
// label_map.hip's resolve launches write the slots, the segment offsets and the tile offsets that K8b and K8c read; the kept
// entries' positions come back with the hand-back.  *took = false: the batch has a list beyond the scratch, which the host
// resolve may still shorten enough -- nothing was done, the caller resolves on the host.  *resolved_keys = keys uploaded.
Status prefilter_device_stage_keys(SearchCtx *ctx, const LabelMapTable &map, const void *d_rows, uint32_t dim, uint32_t stride_f, bool l2,
                                   bool bf16, const float *queries, uint64_t nq, uint64_t k, const uint64_t *labels, const uint64_t *list_begin,
                                   uint64_t n_labels, PrefilterCands *out, bool *took, uint64_t *resolved_keys);

// The device stage of handle_candidates on one device (prefilter_handle.cc): the filter's bitmap expanded into the ascending
// list of its labels in the context's scratch (filter_expand.hip), that list resolved by label_map.hip's three launches as one
// shared segment, K8b and K8c as prefilter_device_stage_keys launches them, one gather of the candidates' labels, and a
// download of counts, candidates and candidate labels only.  map == nullptr (no usable label map), an admitted count beyond
// the scratch or different from the device's total, k beyond the hand-back, a query wider than K8b's LDS: every query is
// marked.  *expanded = labels the expansion wrote, *known = entries of the resolved list.  The caller holds the index's
// shared lock and the context's lease.
Status prefilter_handle_stage(SearchCtx *ctx, const LabelMapTable *map, const uint64_t *d_bits, uint64_t nbits, uint64_t allowed,
                              const void *d_rows, uint32_t dim, uint32_t stride_f, bool l2, bool bf16, const float *queries, uint64_t nq,
                              uint64_t k, HandleCands *out, uint64_t *expanded, uint64_t *known);
// vk_filter_read_labels, and the fallback's download: the filter's first copy expanded on its device's build lane
Status filter_read_labels(const FilterSet &f, uint64_t *out_labels, uint64_t cap, uint64_t *out_n);

// vk_index_load_tracked: the VectorTracker hook of LoadIndex (bruteforce.h:201, hnswalg.h:1000) -- set by the ABI entry
// around the load on the loading thread, called by the loaders once per element as it is read from the stream
struct LoadObserver { vk_row_fn fn; void *user; };
extern thread_local const LoadObserver *g_load_observer;
inline Status observe_loaded_row(uint64_t label, const void *row) {
  if (g_load_observer && g_load_observer->fn(g_load_observer->user, label, row))
    return Status::Err(VK_ERR_INTERNAL, "load: the row callback failed");
  return Status::Ok();
}

Status create_sharded(const vk_index_params &p, std::unique_ptr<Index> *out);
Status load_sharded(const vk_index_params &p, vk_read_chunk_fn fn, void *user, std::unique_ptr<Index> *out);
Status create_flat(const vk_index_params &p, std::unique_ptr<Index> *out);
Status create_hnsw(const vk_index_params &p, std::unique_ptr<Index> *out);
Status load_flat(const vk_index_params &p, vk_read_chunk_fn fn, void *user, std::unique_ptr<Index> *out);
Status load_hnsw(const vk_index_params &p, vk_read_chunk_fn fn, void *user, std::unique_ptr<Index> *out);

// shared helpers --------------------------------------------------------------------
// pad nq host queries of `dim` floats into ctx->h_q ([nq][stride_f]) and copy to ctx->d_q
// (query_tab != nullptr: one host pointer per query instead of the contiguous block; parallel: large blocks copied by four threads)
Status upload_queries(SearchCtx *ctx, const float *queries, uint64_t nq, uint32_t dim, uint32_t stride_f, bool parallel = true,
                      const float *const *query_tab = nullptr);
Status upload_allow(SearchCtx *ctx, const uint64_t *allow_bits, uint64_t allow_nbits, const uint64_t **d_allow);
// an index without per-query filters in its kernels: the batch split into runs of queries that share a bitmap
Status search_grouped_by_filter(Index *ix, const SearchRequest &rq, float *out_dist, uint64_t *out_label, uint64_t *out_n);
// exact kNN over gathered distances with the AddPrefilteredKey rule (vector_base.cc:509-530)
void prefilter_heap_select(const float *dist, const uint64_t *labels, uint64_t n, uint64_t k,
                           float *out_dist, uint64_t *out_label, uint64_t *out_n);

// protobuf varint helpers for the index.proto headers (persist.cc)
void pb_put_varint_field(std::string &s, uint32_t field, uint64_t v);
void pb_put_double_field(std::string &s, uint32_t field, double v);
struct PbReader {
  const uint8_t *p, *end;
  bool next(uint32_t *field, uint32_t *wire, uint64_t *val);
};

}  // namespace vk
