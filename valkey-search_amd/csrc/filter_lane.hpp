// filter_lane.hpp -- the per-device build lane of the filter code (filter_set.cc, filter_delta.cc): one stream, one pinned
// staging block and one device staging block per device, shared by the builds on it (they are short and serialise).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <mutex>

#include "row_store.hpp"   // Status

namespace vk {
namespace filter_lane {

struct BuildLane {
  std::mutex mu;
  hipStream_t stream = nullptr;
  char *pin = nullptr;
  size_t pin_cap = 0;
  void *d_stage = nullptr;
  size_t d_cap = 0;
  unsigned long long *d_count = nullptr;
  unsigned long long *d_partial = nullptr;   // [2 * kPartials]: per-block bit counts (ids | runs; a combine uses the first half)
};
constexpr size_t kPartials = 2048;
constexpr size_t kStageBytes = (size_t)4 << 20;   // ids travel in 4 MiB pieces through pinned memory: copy k+1 is filled while k is in flight

BuildLane *lane_of(int device);                   // (created on first use, never freed)
Status lane_ready(BuildLane *l);                  // the caller holds l->mu and has made the lane's device current: stream, pinned block (2 * kStageBytes), counters
Status stage_ensure(BuildLane *l, size_t bytes);  // ... d_stage of at least `bytes`
// host words -> device through the two halves of the pinned block; returns after the last copy has landed
Status upload(BuildLane *l, void *d_dst, const void *h_src, size_t bytes);
// An error return lets a half-built filter go, and its blocks back into the pool, while copies and kernels that write them may
// still be queued on the lane's stream: whatever way the scope is left, the stream is drained first.
struct LaneDrain {
  hipStream_t s;
  ~LaneDrain() { (void)hipStreamSynchronize(s); }
};

}  // namespace filter_lane
}  // namespace vk
