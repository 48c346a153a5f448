// filter_expand.hip -- a device filter's bitmap turned into the ascending list of its set labels, gfx950: the first step of
// the exact kNN from a filter handle (vk_index_search_filter_exact_batch, prefilter_handle.cc), and the whole of
// vk_filter_read_labels.  The list it writes is what label_map.hip's resolve launches read as their key list.
//
// A tile is kExpandTileWords = 1024 words of the bitmap (65 536 labels), one 256-thread block, four rows of 256 words:
// in row j thread t owns word tile * 1024 + j * 256 + t, so a wave's loads are one contiguous 512 B piece per row.
//
//   filter_expand_count_kernel   one block per tile: the tile's number of set bits below nbits into tile_off[tile]
//   filter_expand_scan_kernel    one block: tile_off[] turned in place into the running number of set bits before every
//                                tile, kExpandScanTrip = 256 tiles per trip (one per thread: a wave prefix by six
//                                __shfl_up steps, then LDS over the four waves) with the carry in a register; the sum
//                                into *total
//   filter_expand_emit_kernel    one block per tile again: per row the block prefixes its threads' popcounts (the same
//                                wave prefix + LDS over the four waves, as label_map_compact_kernel does with its ballots),
//                                then each WAVE writes its words one after the other: the word and its place are broadcast
//                                from the lane that owns them, lane l tests bit l and the set lanes store their labels
//                                side by side.  A dense word is one coalesced 512 B store; an empty word costs nothing
//                                (the wave walks a ballot of its non-empty words).  Per-lane find-first-set loops would
//                                write the same bytes as 64 scattered 8 B stores per step.
//   filter_gather_labels_kernel  after K8c: per handed-back candidate (index into the resolved list, distance bits) the
//                                label keys[pos[index]] next to it, so that the host never sees pos[]
//
// Bits at or above nbits in the last word are masked out, and no word at or past (nbits + 63) / 64 is read (a FilterSet
// keeps one slack word there).  Nothing is written at or past cap, and nothing past min(total, cap).
//
// Every loop has a bound that does not depend on memory contents: four rows per tile, at most 64 words per wave and row,
// n_tiles / 256 trips of the scan, six steps of a wave prefix.  Nothing waits for another thread's write (a launch reads
// what an earlier launch wrote).  Plain vector loads and stores and LDS only.
#include "device_common.hpp"
#include "kernels.hpp"

namespace vk {

namespace {

constexpr uint32_t kExpandThreads = 256;
constexpr uint32_t kExpandRows = 4;                                      // words per thread and tile
constexpr uint32_t kExpandTileWords = kExpandThreads * kExpandRows;      // 1024 words = 65 536 labels
constexpr uint32_t kExpandScanTrip = 256;                                // tiles per trip of the scan block

// the thread's word of row j of tile `tile`, stray bits gone; words past the bitmap read as 0 (and are not loaded)
__device__ __forceinline__ uint64_t expand_word(const uint64_t *__restrict__ bits, uint64_t nbits, uint64_t wi) {
  const uint64_t words = (nbits + 63) >> 6;
  if (wi >= words) return 0;
  uint64_t w = bits[wi];
  const uint32_t tail = (uint32_t)(nbits & 63);
  if (wi == words - 1 && tail) w &= (1ull << tail) - 1ull;
  return w;
}

// inclusive prefix over the wave's 64 lanes
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// exclusive prefix of v over the block's 256 threads, and the block's sum; s_cnt: 4 words, free to rewrite on return
__device__ __forceinline__ uint32_t block_exclusive_sum(uint32_t v, uint32_t *s_cnt, uint32_t *block_sum) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc = wave_inclusive_sum(v, lane);
  if (lane == 63) s_cnt[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < 4; ++w) {
    const uint32_t c = s_cnt[w];
    before += w < wave ? c : 0u;
    all += c;
  }
  __syncthreads();
  *block_sum = all;
  return before + inc - v;
}

__global__ __launch_bounds__(256) void filter_expand_count_kernel(const uint64_t *__restrict__ bits, uint64_t nbits,
                                                                  unsigned long long *__restrict__ tile_off) {
  __shared__ uint32_t s_cnt[4];
  const uint64_t w0 = (uint64_t)blockIdx.x * kExpandTileWords + threadIdx.x;
  uint32_t pc = 0;
#pragma unroll
  for (uint32_t j = 0; j < kExpandRows; ++j) pc += (uint32_t)__popcll(expand_word(bits, nbits, w0 + (uint64_t)j * kExpandThreads));
  uint32_t all;
  (void)block_exclusive_sum(pc, s_cnt, &all);
  if (threadIdx.x == 0) tile_off[blockIdx.x] = all;
}

__global__ __launch_bounds__(256) void filter_expand_scan_kernel(unsigned long long *__restrict__ tile_off, uint32_t n_tiles,
                                                                 unsigned long long *__restrict__ total) {
  __shared__ uint32_t s_cnt[4];
  unsigned long long carry = 0;
  for (uint32_t base = 0; base < n_tiles; base += kExpandScanTrip) {
    const uint32_t t = base + threadIdx.x;
    const uint32_t v = t < n_tiles ? (uint32_t)tile_off[t] : 0u;   // (a tile holds 65 536 bits; a trip 2^24)
    uint32_t all;
    const uint32_t before = block_exclusive_sum(v, s_cnt, &all);
    if (t < n_tiles) tile_off[t] = carry + before;
    carry += all;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(256) void filter_expand_emit_kernel(const uint64_t *__restrict__ bits, uint64_t nbits,
                                                                 const unsigned long long *__restrict__ tile_off, uint64_t cap,
                                                                 uint64_t *__restrict__ labels) {
  __shared__ uint32_t s_cnt[4];
  const uint32_t lane = threadIdx.x & 63;
  uint64_t at_row = tile_off[blockIdx.x];   // the place of the row's first label
  if (at_row >= cap) return;                // (block-uniform: every later place is past cap as well)
  const uint64_t w0 = (uint64_t)blockIdx.x * kExpandTileWords + threadIdx.x;
  for (uint32_t j = 0; j < kExpandRows; ++j) {
    const uint64_t wi = w0 + (uint64_t)j * kExpandThreads;
    const uint64_t w = expand_word(bits, nbits, wi);
    uint32_t all;
    const uint32_t before = block_exclusive_sum((uint32_t)__popcll(w), s_cnt, &all);
    const uint64_t at = at_row + before;    // the place of this thread's first label
    uint64_t todo = __ballot(w != 0);       // the wave's non-empty words, walked in lane order
    for (uint32_t step = 0; step < 64 && todo != 0; ++step) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint64_t sw = readlane_u64(w, src), sat = readlane_u64(at, src), swi = readlane_u64(wi, src);
      if ((sw >> lane) & 1ull) {
        const uint64_t p = sat + (uint32_t)__popcll(sw & ((1ull << lane) - 1ull));
        if (p < cap) labels[p] = swi * 64 + lane;
      }
    }
    at_row += all;
  }
}

__global__ __launch_bounds__(256) void filter_gather_labels_kernel(const uint32_t *__restrict__ count, const uint2 *__restrict__ cand,
                                                                   const uint32_t *__restrict__ pos, const uint64_t *__restrict__ keys,
                                                                   uint32_t list_len, uint32_t cap, uint64_t *__restrict__ out) {
  const uint32_t q = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = count[q];
  if (n > cap || i >= n) return;            // (a NaN segment's count word is above every cap: the host takes the other path)
  const uint32_t e = cand[(size_t)q * cap + i].x;
  if (e < list_len) out[(size_t)q * cap + i] = keys[pos[e]];
}

}  // namespace

uint32_t filter_expand_tiles(uint64_t nbits) { return (uint32_t)((((nbits + 63) >> 6) + kExpandTileWords - 1) / kExpandTileWords); }
uint32_t filter_expand_tile_words() { return kExpandTileWords; }
uint32_t filter_expand_scan_trip() { return kExpandScanTrip; }

hipError_t launch_filter_expand(const uint64_t *bits, uint64_t nbits, uint64_t cap, uint64_t *labels, unsigned long long *total,
                                unsigned long long *tile_off, hipStream_t s) {
  if (nbits >= (1ull << 40) || (nbits && !bits) || !total || (nbits && !tile_off) || (cap && !labels)) return hipErrorInvalidValue;
  const uint32_t n_tiles = filter_expand_tiles(nbits);
  if (n_tiles) {
    hipLaunchKernelGGL(filter_expand_count_kernel, dim3(n_tiles), dim3(kExpandThreads), 0, s, bits, nbits, tile_off);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(filter_expand_scan_kernel, dim3(1), dim3(kExpandThreads), 0, s, tile_off, n_tiles, total);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || n_tiles == 0 || cap == 0) return e;
  hipLaunchKernelGGL(filter_expand_emit_kernel, dim3(n_tiles), dim3(kExpandThreads), 0, s, bits, nbits, tile_off, cap, labels);
  return hipGetLastError();
}

hipError_t launch_filter_gather_labels(const uint32_t *count, const uint2 *cand, const uint32_t *pos, const uint64_t *keys, uint32_t list_len,
                                       uint32_t nq, uint32_t cap, uint64_t *out, hipStream_t s) {
  if (nq == 0 || cap == 0) return hipSuccess;
  if (nq > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(filter_gather_labels_kernel, dim3((cap + 255) / 256, nq), dim3(256), 0, s, count, cand, pos, keys, list_len, cap, out);
  return hipGetLastError();
}

}  // namespace vk
