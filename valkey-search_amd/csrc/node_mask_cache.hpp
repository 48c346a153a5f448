// node_mask_cache.hpp -- the bookkeeping of an HNSW graph's node masks.  No HIP calls: tested on the CPU
// (tests/helpers/san_node_mask_main.cc).
//
// A device filter (filter_set.hpp) is a bitmap over LABELS; the graph walks INTERNAL ids.  A node mask is the filter
// translated once per (filter, graph publication): bit i = node i is live and its label is allowed (node_mask.hip), so a
// hop tests one bit instead of tombstone word -> label -> filter word.  This cache keeps those masks per graph:
//   * keyed by FilterSet::id(), tagged with the graph's publication EPOCH (bumped by every flush that changed the count, a
//     label or a tombstone): an entry of another epoch is dropped where it is met
//   * reference counted: the cache and every search in flight hold a Ref; the device memory goes when the last one does
//   * bounded in bytes, least recently used first out; an entry the asking batch itself uses is never evicted for it
//   * reserve() is the fallback decision: a mask that cannot be given room is not built and its queries take the label path
#pragma once
#include <stdint.h>

#include <list>
#include <memory>
#include <mutex>
#include <unordered_map>

namespace vk {

struct NodeMask {
  uint64_t filter_id = 0, epoch = 0;
  uint64_t *bits = nullptr;     // device memory, (count + 63) / 64 words, bits past count are 0
  uint64_t bytes = 0, admitted = 0;
};

struct NodeMaskCounters {
  uint64_t built = 0, hits = 0, evictions = 0, entries = 0, bytes = 0;
};

class NodeMaskCache {
 public:
  using Ref = std::shared_ptr<const NodeMask>;
  using FreeFn = void (*)(void *user, uint64_t *bits);
  NodeMaskCache(FreeFn free_fn, void *user) : free_(free_fn), user_(user) {}
  ~NodeMaskCache() { clear(); }
  NodeMaskCache(const NodeMaskCache &) = delete;
  NodeMaskCache &operator=(const NodeMaskCache &) = delete;

  // a batch names itself so that what it already holds is not evicted to make room for the rest of it
  uint64_t begin_batch() {
    std::lock_guard<std::mutex> lk(mu_);
    return ++batch_;
  }

  // the mask of `filter_id` as of `epoch`, now the most recently used and held by `batch`; nullptr = none (an entry of
  // another epoch is dropped)
  Ref get(uint64_t filter_id, uint64_t epoch, uint64_t batch) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = by_id_.find(filter_id);
    if (it == by_id_.end()) return nullptr;
    if (it->second->ref->epoch != epoch) {
      drop(it->second);
      return nullptr;
    }
    lru_.splice(lru_.begin(), lru_, it->second);
    it->second->batch = batch;
    hits_ += 1;
    return it->second->ref;
  }

  // Room for a mask of `bytes` under `budget`: least recently used entries go first, never one that `batch` holds.  true =
  // the bytes are set aside (put() or unreserve() must follow); false = it does not fit, NOTHING was evicted, the caller
  // takes the label path.
  bool reserve(uint64_t bytes, uint64_t budget, uint64_t batch) {
    std::lock_guard<std::mutex> lk(mu_);
    if (bytes > budget) return false;
    uint64_t evictable = 0;
    for (const Slot &s : lru_)
      if (s.batch != batch) evictable += s.ref->bytes;
    if (bytes_ + reserved_ - evictable + bytes > budget) return false;
    for (auto it = lru_.end(); bytes_ + reserved_ + bytes > budget && it != lru_.begin();) {
      --it;
      if (it->batch == batch) continue;
      auto victim = it++;
      evictions_ += 1;
      drop(victim);
    }
    reserved_ += bytes;
    return true;
  }
  void unreserve(uint64_t bytes) {
    std::lock_guard<std::mutex> lk(mu_);
    reserved_ -= bytes;
  }

  // a built mask takes the room reserve() set aside.  Two batches may have built the same one: the first stays, the second's
  // memory is released and it gets the first's.
  Ref put(uint64_t filter_id, uint64_t epoch, uint64_t *bits, uint64_t bytes, uint64_t admitted, uint64_t batch) {
    Ref mine = make(filter_id, epoch, bits, bytes, admitted);
    std::lock_guard<std::mutex> lk(mu_);
    reserved_ -= bytes;
    built_ += 1;
    auto it = by_id_.find(filter_id);
    if (it != by_id_.end()) {
      if (it->second->ref->epoch == epoch) {
        it->second->batch = batch;
        return it->second->ref;
      }
      drop(it->second);
    }
    lru_.push_front(Slot{mine, batch});
    by_id_[filter_id] = lru_.begin();
    bytes_ += bytes;
    return mine;
  }

  // a mask that lives outside the cache (vk_index_node_mask_read with the option off): same ownership, no bookkeeping
  Ref make(uint64_t filter_id, uint64_t epoch, uint64_t *bits, uint64_t bytes, uint64_t admitted) const {
    NodeMask *m = new NodeMask;
    m->filter_id = filter_id;
    m->epoch = epoch;
    m->bits = bits;
    m->bytes = bytes;
    m->admitted = admitted;
    const FreeFn f = free_;
    void *const u = user_;
    return Ref(m, [f, u](const NodeMask *p) {
      f(u, p->bits);
      delete p;
    });
  }

  // every entry that is not of `epoch` (the graph published something new)
  void drop_stale(uint64_t epoch) {
    std::lock_guard<std::mutex> lk(mu_);
    for (auto it = lru_.begin(); it != lru_.end();) {
      auto cur = it++;
      if (cur->ref->epoch != epoch) drop(cur);
    }
  }
  void clear() {
    std::lock_guard<std::mutex> lk(mu_);
    while (!lru_.empty()) drop(lru_.begin());
  }

  NodeMaskCounters counters() const {
    std::lock_guard<std::mutex> lk(mu_);
    NodeMaskCounters c;
    c.built = built_;
    c.hits = hits_;
    c.evictions = evictions_;
    c.entries = lru_.size();
    c.bytes = bytes_;
    return c;
  }
  // most recently used first (tests)
  template <class F> void for_each(F &&f) const {
    std::lock_guard<std::mutex> lk(mu_);
    for (const Slot &s : lru_) f(*s.ref);
  }

 private:
  struct Slot { Ref ref; uint64_t batch; };
  void drop(std::list<Slot>::iterator it) {   // mu_ held
    bytes_ -= it->ref->bytes;
    by_id_.erase(it->ref->filter_id);
    lru_.erase(it);
  }
  FreeFn free_;
  void *user_;
  mutable std::mutex mu_;
  std::list<Slot> lru_;   // front = most recently used
  std::unordered_map<uint64_t, std::list<Slot>::iterator> by_id_;
  uint64_t bytes_ = 0, reserved_ = 0, batch_ = 0, built_ = 0, hits_ = 0, evictions_ = 0;
};

}  // namespace vk
