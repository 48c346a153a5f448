// label_map.hip -- the device label map of the batched pre-filter search (option prefilter-device-resolve), gfx950.
//
// An open-addressed hash table in HBM from label (u64) to slot (u32: FLAT's row slot, HNSW's internal id), linear probing,
// capacity a power of two at least twice the published count (label_map_hash.hpp has the hash and the sizing rule).  The
// empty key is UINT64_MAX, a label the index refuses at the door.
//
//   label_map_build_kernel     one pass over the published label array: slot i claims the first free bucket of its label's
//                              probe run with a 64-bit compare-and-swap on the key and writes its value with a plain store
//                              (lookups happen only in later launches).  HNSW: a node whose tombstone bit is set (word 0 of
//                              its level-0 list, where the search kernels read it) is not inserted.  A label met twice, the
//                              empty key as a label, or a probe run as long as the table, is counted in the failure word.
//   label_map_resolve_kernel   one block per 256-key tile of a CSR of key lists (a shared list = one segment): the slot of
//                              every key, or kLabelMapNone, into a scratch array, and the tile's number of known keys
//   label_map_offsets_kernel   one block: the running number of known keys before every tile, from it the segment offsets
//                              (seg_begin) and the running number of K8b's 64-entry tiles (tile_begin)
//   label_map_compact_kernel   one block per key tile again: the known keys' slots, and their positions in the key array,
//                              to their places -- a ballot and a prefix over the block's four waves, so the order is the
//                              list's and duplicates stay
//   label_map_apply_kernel     the map brought up to date after a write phase (option prefilter-label-map-upkeep): one record
//                              (label, slot or kLabelMapNone) per thread, every label at most once per launch.  A key that is
//                              there gets the new value -- an erase stores kLabelMapNone and LEAVES THE KEY, a dead entry, so
//                              probe runs stay whole and label_map_find answers "unknown" from the value; a key that is not
//                              claims the first empty bucket as the build does (an erase of it does nothing).  Four counters
//                              (claimed, revived, killed, moved) beside the failure word tell the host what happened.
//
// The three resolve launches write what prefilter_device_stage builds on the host from prefilter_resolve's output; K8b
// and K8c (prefilter_select.hip) read it as they read the host's.
//
// Every loop has a bound that does not depend on memory contents: a probe run ends after `capacity` buckets at the latest
// (build: a failure; lookup: "unknown"), the binary searches after 32 steps, the scans after their element count.  Nothing
// waits for another thread's write.  Plain vector loads and stores, LDS, and global atomics (the key claim and the failure
// count) only.
#include "device_common.hpp"
#include "kernels.hpp"
#include "label_map_hash.hpp"

namespace vk {

namespace {

constexpr uint32_t kKeyTile = 256;            // keys per block of the resolve / compact launches
constexpr uint32_t kDistTile = 64;            // K8b's tile (prefilter_tiles)
constexpr uint32_t kTombstone = 0x00010000u;  // HnswGraph::kDeleteFlag

__global__ __launch_bounds__(256) void label_map_build_kernel(LabelMapBuildArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.count) return;
  if (a.links0 != nullptr && (a.links0[(size_t)i * a.l0_stride] & kTombstone)) return;
  const uint64_t label = a.labels[i];
  if (label == kLabelMapEmpty) {
    atomicAdd(a.t.fail, 1u);
    return;
  }
  const uint64_t mask = a.t.capacity - 1;
  uint64_t h = label_map_bucket(label, a.t.capacity);
  for (uint64_t p = 0; p < a.t.capacity; ++p) {
    const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(a.t.keys + h), (unsigned long long)kLabelMapEmpty,
                                              (unsigned long long)label);
    if (prev == kLabelMapEmpty) {
      a.t.vals[h] = i;
      return;
    }
    if (prev == label) break;   // a label met twice
    h = (h + 1) & mask;
  }
  atomicAdd(a.t.fail, 1u);      // ... or no free bucket in a whole turn of the table
}

__device__ __forceinline__ uint32_t label_map_find(const LabelMapTable &t, uint64_t label) {
  if (label == kLabelMapEmpty) return kLabelMapNone;
  const uint64_t mask = t.capacity - 1;
  uint64_t h = label_map_bucket(label, t.capacity);
  for (uint64_t p = 0; p < t.capacity; ++p) {
    const uint64_t k = t.keys[h];
    if (k == label) return t.vals[h];
    if (k == kLabelMapEmpty) return kLabelMapNone;
    h = (h + 1) & mask;
  }
  return kLabelMapNone;
}

// the key this thread owns in key tile `b`: the segment whose tile range holds b (ktile_begin[s] <= b < ktile_begin[s + 1])
__device__ __forceinline__ bool key_of_thread(const LabelMapResolveArgs &a, uint32_t b, uint32_t *key_index) {
  uint32_t lo = 0, hi = a.n_seg;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.ktile_begin[mid] <= b) lo = mid; else hi = mid;
  }
  const uint32_t i = a.list_begin[lo] + (b - a.ktile_begin[lo]) * kKeyTile + threadIdx.x;
  *key_index = i;
  return i < a.list_begin[lo + 1];
}

__global__ __launch_bounds__(256) void label_map_resolve_kernel(LabelMapResolveArgs a) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t i;
  const bool valid = key_of_thread(a, blockIdx.x, &i);
  uint32_t slot = kLabelMapNone;
  if (valid) {
    slot = label_map_find(a.t, a.keys[i]);
    a.raw[i] = slot;
  }
  const uint64_t b = __ballot(slot != kLabelMapNone);
  if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) a.tile_off[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// in place: v[i] = v[0] + ... + v[i - 1] for i <= n (v[n] = the total); each thread owns one contiguous run
__device__ void block_exclusive_scan(uint32_t *v, uint32_t n, uint32_t *s_part) {
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n + 255) / 256;
  const uint32_t lo = min(tid * per, n), hi = min(lo + per, n);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += v[i];
  s_part[tid] = sum;
  __syncthreads();
  uint32_t base = 0;
  for (uint32_t t = 0; t < tid; ++t) base += s_part[t];
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t x = v[i];
    v[i] = base;
    base += x;
  }
  if (tid == 255) v[n] = base;
  __syncthreads();
}

__global__ __launch_bounds__(256) void label_map_offsets_kernel(LabelMapResolveArgs a) {
  __shared__ uint32_t s_part[256];
  block_exclusive_scan(a.tile_off, a.n_ktiles, s_part);
  for (uint32_t s = threadIdx.x; s <= a.n_seg; s += 256) a.seg_begin[s] = a.tile_off[a.ktile_begin[s]];
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < a.n_seg; s += 256)
    a.tile_begin[s] = (a.seg_begin[s + 1] - a.seg_begin[s] + kDistTile - 1) / kDistTile;
  __syncthreads();
  block_exclusive_scan(a.tile_begin, a.n_seg, s_part);
}

__global__ __launch_bounds__(256) void label_map_compact_kernel(LabelMapResolveArgs a) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t i;
  const bool valid = key_of_thread(a, blockIdx.x, &i);
  const uint32_t slot = valid ? a.raw[i] : kLabelMapNone;
  const bool keep = slot != kLabelMapNone;
  const uint64_t b = __ballot(keep);
  if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t before = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) before += w < wave ? s_cnt[w] : 0u;
  if (keep) {
    const uint32_t at = a.tile_off[blockIdx.x] + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    a.slot[at] = slot;
    a.pos[at] = i;
  }
}

// one record per thread, grid-stride: labels[i] now answers slots[i] (kLabelMapNone = unknown).  The host sends every label
// at most once per launch, so no two threads ever write the same value word; two threads may still want the same EMPTY
// bucket, which the build's compare-and-swap settles -- the loser probes on.  A key, once written, is never taken back (an
// erased label keeps its bucket with the value kLabelMapNone), so a key read with a plain load is either still empty --
// then the compare-and-swap decides -- or final.
__global__ __launch_bounds__(256) void label_map_apply_kernel(LabelMapApplyArgs a) {
  const uint64_t mask = a.t.capacity - 1;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    const uint64_t label = a.labels[i];
    const uint32_t slot = a.slots[i];
    if (label == kLabelMapEmpty) {
      atomicAdd(a.t.fail, 1u);
      continue;
    }
    uint64_t h = label_map_bucket(label, a.t.capacity);
    bool done = false;
    for (uint64_t p = 0; p < a.t.capacity; ++p) {
      uint64_t k = a.t.keys[h];
      if (k == kLabelMapEmpty) {
        if (slot == kLabelMapNone) {   // the map never held it: nothing to erase
          done = true;
          break;
        }
        k = atomicCAS(reinterpret_cast<unsigned long long *>(a.t.keys + h), (unsigned long long)kLabelMapEmpty, (unsigned long long)label);
        if (k == kLabelMapEmpty) {
          a.t.vals[h] = slot;
          atomicAdd(a.counters + kLabelMapClaimed, 1u);
          done = true;
          break;
        }
      }
      if (k == label) {
        const uint32_t old = a.t.vals[h];
        a.t.vals[h] = slot;
        if (old == kLabelMapNone && slot != kLabelMapNone) atomicAdd(a.counters + kLabelMapRevived, 1u);
        else if (old != kLabelMapNone && slot == kLabelMapNone) atomicAdd(a.counters + kLabelMapKilled, 1u);
        else if (old != slot) atomicAdd(a.counters + kLabelMapMoved, 1u);
        done = true;
        break;
      }
      h = (h + 1) & mask;
    }
    if (!done) atomicAdd(a.t.fail, 1u);   // a whole turn of the table without the key or a free bucket
  }
}

}  // namespace

uint32_t label_map_key_tiles(uint64_t keys) { return (uint32_t)((keys + kKeyTile - 1) / kKeyTile); }

hipError_t launch_label_map_build(const LabelMapBuildArgs &a, hipStream_t s) {
  if (a.t.capacity < kLabelMapMinCapacity || a.t.capacity > kLabelMapMaxCapacity || (a.t.capacity & (a.t.capacity - 1)) != 0 ||
      a.t.capacity < 2 * (uint64_t)a.count)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.t.keys, 0xFF, a.t.capacity * 8, s);   // every bucket empty
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.t.fail, 0, 4, s);
  if (e != hipSuccess) return e;
  if (a.count == 0) return hipSuccess;
  hipLaunchKernelGGL(label_map_build_kernel, dim3((a.count + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_label_map_resolve(const LabelMapResolveArgs &a, hipStream_t s) {
  if (a.n_seg == 0) return hipErrorInvalidValue;
  if (a.n_ktiles) {
    hipLaunchKernelGGL(label_map_resolve_kernel, dim3(a.n_ktiles), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(label_map_offsets_kernel, dim3(1), dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.n_ktiles == 0) return e;
  hipLaunchKernelGGL(label_map_compact_kernel, dim3(a.n_ktiles), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_label_map_apply(const LabelMapApplyArgs &a, hipStream_t s) {
  if (a.t.capacity < kLabelMapMinCapacity || a.t.capacity > kLabelMapMaxCapacity || (a.t.capacity & (a.t.capacity - 1)) != 0)
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.t.fail, 0, 4, s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(a.counters, 0, kLabelMapCounters * 4, s);
  if (e != hipSuccess || a.n == 0) return e;
  const uint64_t want = ((uint64_t)a.n + 255) / 256;
  const uint32_t blocks = (uint32_t)(want < kLabelMapApplyMaxBlocks ? want : kLabelMapApplyMaxBlocks);
  hipLaunchKernelGGL(label_map_apply_kernel, dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace vk
