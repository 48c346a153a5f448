// label_map_delta_host.hpp -- the host half of the device label map's upkeep (option prefilter-label-map-upkeep): the set of
// labels a write phase touched, the records made from it, the decision between an apply launch and a rebuild, and the
// check of the counters an apply launch hands back.  No HIP header in here: a stand-alone host program drives it under the
// sanitizers (tests/helpers/san_label_map_delta_main.cc).  The kernel is label_map_apply_kernel (label_map.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "label_map_hash.hpp"

namespace vk {

// The labels whose answer (slot, or unknown) may have changed since the map was last brought up to date: any order,
// duplicates allowed.  Writers record under the set's own mutex, whatever lock of the index they hold.  Beyond `max` labels
// the set stops listing and means "everything" (the map is rebuilt whole); so does set_all(), for paths that bring labels in
// without naming them.
class LabelTouchSet {
 public:
  void touch(uint64_t label) {
    if (all_.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> g(mu_);
    if (all_.load(std::memory_order_relaxed)) return;
    labels_.push_back(label);
    collapse_if_over();
  }
  void touch_many(const uint64_t *labels, size_t n) {
    if (n == 0 || all_.load(std::memory_order_relaxed)) return;
    std::lock_guard<std::mutex> g(mu_);
    if (all_.load(std::memory_order_relaxed)) return;
    if (labels_.size() + n > max_) {   // (over the limit whatever the labels are: none of them is copied)
      std::vector<uint64_t>().swap(labels_);
      all_.store(true, std::memory_order_relaxed);
      return;
    }
    labels_.insert(labels_.end(), labels, labels + n);
  }
  void set_all() {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<uint64_t>().swap(labels_);
    all_.store(true, std::memory_order_relaxed);
  }
  void set_max(uint64_t max) {
    std::lock_guard<std::mutex> g(mu_);
    max_ = std::max<uint64_t>(max, 1);
    collapse_if_over();
  }
  // what was recorded so far moves out; the set is empty afterwards
  void take(std::vector<uint64_t> *labels, bool *all) {
    std::lock_guard<std::mutex> g(mu_);
    labels->clear();
    labels->swap(labels_);
    *all = all_.load(std::memory_order_relaxed);
    all_.store(false, std::memory_order_relaxed);
  }
  void clear() {
    std::lock_guard<std::mutex> g(mu_);
    labels_.clear();
    all_.store(false, std::memory_order_relaxed);
  }
  bool empty() const {
    std::lock_guard<std::mutex> g(mu_);
    return labels_.empty() && !all_.load(std::memory_order_relaxed);
  }

 private:
  void collapse_if_over() {   // under mu_
    if (labels_.size() <= max_) return;
    std::vector<uint64_t>().swap(labels_);
    all_.store(true, std::memory_order_relaxed);
  }
  mutable std::mutex mu_;
  std::vector<uint64_t> labels_;
  std::atomic<bool> all_{false};
  uint64_t max_ = 65536;
};

// the records of one apply launch: labels[i] now answers slots[i] (kLabelMapNone = unknown); every label once
struct LabelMapDelta {
  std::vector<uint64_t> labels;
  std::vector<uint32_t> slots;
  uint64_t upserts = 0, erases = 0;
};

// `touched` (sorted and deduplicated in place) against the index's own truth: truth(label) = the slot the label answers now,
// or kLabelMapNone.  A label recorded although nothing changed for it costs a record and changes nothing (the kernel stores
// what is there already).  The empty key is not a label (the index refuses it at the door) and is dropped.
template <class Truth>
void label_map_net_delta(std::vector<uint64_t> *touched, Truth &&truth, LabelMapDelta *out) {
  std::sort(touched->begin(), touched->end());
  touched->erase(std::unique(touched->begin(), touched->end()), touched->end());
  out->labels.clear();
  out->slots.clear();
  out->upserts = out->erases = 0;
  out->labels.reserve(touched->size());
  out->slots.reserve(touched->size());
  for (const uint64_t label : *touched) {
    if (label == kLabelMapEmpty) continue;
    const uint32_t slot = truth(label);
    out->labels.push_back(label);
    out->slots.push_back(slot);
    if (slot == kLabelMapNone) out->erases += 1;
    else out->upserts += 1;
  }
}

// what the host knows of the table between launches: used = keys in it, dead ones (value kLabelMapNone) included
struct LabelMapState {
  bool usable = false;
  uint64_t capacity = 0, used = 0, live = 0;
};

enum class LabelMapPlan : uint32_t {
  kApply = 0,
  kRebuildNoMap,        // no table, or one whose build failed
  kRebuildEverything,   // the touched set overflowed, or a path that names no labels ran
  kRebuildLoad,         // used + upserts would pass half the capacity (dead keys count: a probe run ends at an EMPTY bucket only)
  kRebuildSmall,        // capacity < 2 x count: the sizing rule of the build no longer holds
};

// apply or rebuild; count = published slots (HNSW: tombstoned ones included, as the build's sizing rule counts them)
inline LabelMapPlan label_map_plan(const LabelMapState &m, bool everything, uint64_t upserts, uint64_t count) {
  if (!m.usable || m.capacity == 0) return LabelMapPlan::kRebuildNoMap;
  if (everything) return LabelMapPlan::kRebuildEverything;
  if (m.used + upserts > m.capacity / 2) return LabelMapPlan::kRebuildLoad;
  if (m.capacity < 2 * count) return LabelMapPlan::kRebuildSmall;
  return LabelMapPlan::kApply;
}

// the words an apply launch leaves: the failure word, then the four counters in the kernel's order
struct LabelMapApplied {
  uint32_t fail = 0, claimed = 0, revived = 0, killed = 0, moved = 0;
};

// The self-check behind an apply: the live entries the table must hold now against the index's live count.  false = a touched
// label was missed somewhere (or a record found no bucket): the table is not served from, it is rebuilt.
inline bool label_map_check_applied(uint64_t live_before, const LabelMapApplied &c, uint64_t index_live, uint64_t *live_after) {
  *live_after = live_before + c.claimed + c.revived - c.killed;
  if (c.fail != 0) return false;
  if ((uint64_t)c.killed > live_before + c.claimed + c.revived) return false;
  return *live_after == index_live;
}

}  // namespace vk
