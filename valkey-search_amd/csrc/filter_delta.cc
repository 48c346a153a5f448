// filter_delta.cc -- FilterSet::apply_delta_batch: new filters derived ON THE DEVICE from older ones plus a delta of labels.
//
// The module's tag index changes a handful of keys per write phase (src/indexes/tag.cc AddRecord / ModifyRecord /
// RemoveRecord) and switches back to reading every few milliseconds (src/index_schema.cc:285-292).  Rebuilding the filter
// of `@tag:{x}` from its posting list after each phase moves the whole id list over PCIe again; here the filter of the last
// phase is copied device to device (grown if labels were assigned meanwhile) and only the changed labels travel.
// A filter stays immutable: searches in flight and callers holding the base keep exactly what they had.
#include <string.h>

#include <algorithm>

#include "filter_lane.hpp"
#include "filter_set.hpp"
#include "kernels.hpp"

namespace vk {
using namespace filter_lane;

Status FilterSet::apply_delta_batch(const std::vector<int> &devices, const Delta *items, uint64_t n,
                                    std::vector<std::shared_ptr<FilterSet>> *out) {
  out->clear();
  if (n == 0) return Status::Ok();
  if (n > 65535) return Status::Err(1, "filter: at most 65535 derivations per call");
  if (!items) return Status::Err(1, "filter: NULL delta list");
  std::vector<int> devs;   // (logical shards share a device: one copy per device)
  for (int d : devices)
    if (std::find(devs.begin(), devs.end(), d) == devs.end()) devs.push_back(d);
  if (devs.empty()) return Status::Err(1, "filter: the index has no device");
  // ---- every argument error before any device work
  uint64_t n_clear = 0, n_set = 0, max_words = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const Delta &it = items[i];
    if (it.nbits >= ((uint64_t)1 << kFilterDeltaLabelBits)) return Status::Err(1, "filter: nbits out of range");
    if ((it.n_clear && !it.clear) || (it.n_set && !it.set)) return Status::Err(1, "filter: NULL label list");
    if (it.base) {
      if (it.nbits < it.base->nbits_) return Status::Err(1, "filter: a derived filter cannot be smaller than its base (labels count up)");
      if (it.base->copies_.size() != devs.size()) return Status::Err(1, "filter: the base lives on other devices than the index");
      for (int d : devs)
        if (!it.base->bits_on(d)) return Status::Err(1, "filter: the base lives on other devices than the index");
    }
    max_words = std::max<uint64_t>(max_words, (it.nbits + 63) / 64);
  }
  // ---- the label records of all items: the clears, then the sets (labels >= nbits are ignored: they do not travel)
  std::vector<uint64_t> recs;
  for (int pass = 0; pass < 2; ++pass) {
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t *lab = pass ? items[i].set : items[i].clear;
      const uint64_t cnt = pass ? items[i].n_set : items[i].n_clear, nbits = items[i].nbits, tag = i << kFilterDeltaLabelBits;
      for (uint64_t j = 0; j < cnt; ++j)
        if (lab[j] < nbits) recs.push_back(lab[j] | tag);
    }
    (pass ? n_set : n_clear) = recs.size() - (pass ? n_clear : 0);
  }
  std::vector<std::shared_ptr<FilterSet>> res(n);
  for (uint64_t i = 0; i < n; ++i) VK_TRY(allocate(devs, items[i].nbits, &res[i]));
  const size_t cnt_bytes = (size_t)n * 8, tab_bytes = (size_t)n * kFilterDeltaItemWords * 8, rec_bytes = recs.size() * 8;
  std::vector<BuildLane *> lanes;
  struct DrainAll {   // (an error return lets the results go while kernels that write them may still run)
    std::vector<BuildLane *> &ls; const std::vector<int> &ds; bool armed = true;
    ~DrainAll() {
      if (!armed) return;
      for (size_t i = 0; i < ls.size(); ++i) { (void)hipSetDevice(ds[i]); (void)hipStreamSynchronize(ls[i]->stream); }
    }
  } drain_on_error{lanes, devs};
  std::vector<unsigned long long> counts(n, 0);
  for (size_t di = 0; di < devs.size(); ++di) {
    BuildLane *l = lane_of(devs[di]);
    std::lock_guard<std::mutex> lk(l->mu);
    VK_HIP_TRY(hipSetDevice(devs[di]));
    VK_TRY(lane_ready(l));
    lanes.push_back(l);
    if (cnt_bytes + tab_bytes > l->pin_cap) return Status::Err(1, "filter: batch too large for the staging block");
    VK_TRY(stage_ensure(l, tab_bytes + rec_bytes + cnt_bytes));
    // the pinned block (free while the lane's lock is held): [counts coming back | table | records], the device block:
    // [table | records | counts]
    uint64_t *tab = reinterpret_cast<uint64_t *>(l->pin + cnt_bytes);
    for (uint64_t i = 0; i < n; ++i) {
      uint64_t *t = tab + i * kFilterDeltaItemWords;
      t[0] = reinterpret_cast<uint64_t>(res[i]->copies_[di].bits);
      t[1] = items[i].base ? reinterpret_cast<uint64_t>(items[i].base->bits_on(devs[di])) : 0;
      t[2] = items[i].base ? items[i].base->words() : 0;
      t[3] = res[i]->words();
      t[4] = items[i].nbits;
      t[5] = 0;
    }
    char *stage = static_cast<char *>(l->d_stage);
    const uint64_t *d_tab = reinterpret_cast<const uint64_t *>(stage), *d_recs = reinterpret_cast<const uint64_t *>(stage + tab_bytes);
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(stage + tab_bytes + rec_bytes);
    if (cnt_bytes + tab_bytes + rec_bytes <= l->pin_cap) {   // the usual case: table and records leave in ONE copy, nothing is waited for
      if (rec_bytes) memcpy(l->pin + cnt_bytes + tab_bytes, recs.data(), rec_bytes);
      VK_HIP_TRY(hipMemcpyAsync(stage, tab, tab_bytes + rec_bytes, hipMemcpyHostToDevice, l->stream));
    } else {                                                  // millions of labels: in pieces, like the id list of a build
      VK_HIP_TRY(hipMemcpyAsync(stage, tab, tab_bytes, hipMemcpyHostToDevice, l->stream));
      VK_HIP_TRY(hipStreamSynchronize(l->stream));            // (upload() fills the pinned block the table is travelling from)
      VK_TRY(upload(l, stage + tab_bytes, recs.data(), rec_bytes));
    }
    VK_HIP_TRY(hipMemsetAsync(d_counts, 0, cnt_bytes, l->stream));
    VK_HIP_TRY(launch_filter_delta_copy(d_tab, (uint32_t)n, max_words, l->stream));
    VK_HIP_TRY(launch_filter_delta_apply(d_tab, d_recs, n_clear, 0, d_counts, l->stream));
    VK_HIP_TRY(launch_filter_delta_apply(d_tab, d_recs + n_clear, n_set, 1, d_counts, l->stream));
    // the counts come back with the first device's copy (every copy holds the same bits); every device is waited for under
    // its lane's lock: the table travels from the lane's pinned block, which the lock's next holder overwrites
    if (di == 0) VK_HIP_TRY(hipMemcpyAsync(l->pin, d_counts, cnt_bytes, hipMemcpyDeviceToHost, l->stream));
    VK_HIP_TRY(hipStreamSynchronize(l->stream));
    if (di == 0) memcpy(counts.data(), l->pin, cnt_bytes);
  }
  drain_on_error.armed = false;
  // (bits really set minus bits really cleared, as a two's complement sum)
  for (uint64_t i = 0; i < n; ++i) res[i]->allowed_ = (items[i].base ? items[i].base->allowed_ : 0) + counts[i];
  out->swap(res);
  return Status::Ok();
}

}  // namespace vk
