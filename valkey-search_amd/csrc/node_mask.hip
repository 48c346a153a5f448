// node_mask.hip -- device filters translated from LABEL space into the graph's INTERNAL-id space.
//
//   node_mask[f][i] = live[i] && allow_bit(filter_f, nbits_f, labels[i])        for i < count, n filters in ONE launch
//
// The HNSW search tests "may this node enter the result list" per neighbour: tombstone word (4 B out of a strided level-0
// record), label (8 B), filter word (its address known only once the label arrived) -- three dependent loads.  With a
// mask it is one bit in a table of count / 8 bytes (hnsw_search.hip, HnswSearchArgs::mask_tab).
//
// Layout of the pass: a wave owns kWordsPerWave consecutive mask words = 512 nodes; their labels are read ONCE, coalesced
// (64 lanes x 8 B), and stay in registers while the wave walks the n filters -- labels[] (8 B per node) is the only stream
// that scales with the graph, and it is read once whatever n is.  Per filter every lane tests its eight labels against
// the filter's bitmap (count / 8 bytes per filter: it sits in L2 / Infinity Cache when labels follow insertion order, and
// the test is a gather otherwise), one ballot per word, and lanes 0..7 write the eight words with one 64-byte store.  The
// admitted nodes are counted on the way: lane l of a wave keeps the count of filter 64g + l, a block adds its four waves'
// counts in LDS and issues one atomic per filter for every group of 64 filters.
#include <algorithm>

#include "kernels.hpp"

namespace vk {
namespace {
constexpr int kThreads = 256;
constexpr uint32_t kWordsPerWave = 8, kWordsPerBlock = kWordsPerWave * (kThreads / 64);

__global__ __launch_bounds__(kThreads) void node_mask_build_kernel(const uint64_t *__restrict__ labels, const uint64_t *__restrict__ live,
                                                                    uint32_t count, uint32_t words, const uint64_t *__restrict__ items,
                                                                    uint32_t n, unsigned long long *counts) {
  __shared__ unsigned int s_cnt[64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t w0 = (blockIdx.x * (kThreads / 64) + wave) * kWordsPerWave;
  uint64_t lab[kWordsPerWave];
  uint32_t valid = 0;   // bit k: node (w0 + k) * 64 + lane exists and is live
#pragma unroll
  for (uint32_t k = 0; k < kWordsPerWave; ++k) {
    const uint64_t i = (uint64_t)(w0 + k) * 64u + lane;
    lab[k] = 0;
    if (w0 + k < words && i < count) {
      lab[k] = labels[i];
      valid |= (uint32_t)((live[w0 + k] >> lane) & 1ull) << k;
    }
  }
  for (uint32_t g = 0; g < n; g += 64) {
    if (threadIdx.x < 64) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t in_group = n - g < 64u ? n - g : 64u;
    uint32_t my_cnt = 0;
    for (uint32_t fl = 0; fl < in_group; ++fl) {
      const uint64_t *it = items + (size_t)(g + fl) * kNodeMaskItemWords;
      const uint64_t *bits = reinterpret_cast<const uint64_t *>(it[0]);
      const uint64_t nbits = it[1];
      uint64_t *dst = reinterpret_cast<uint64_t *>(it[2]);
      uint64_t mine = 0;
      uint32_t c = 0;
#pragma unroll
      for (uint32_t k = 0; k < kWordsPerWave; ++k) {
        bool ok = false;
        if (((valid >> k) & 1u) && lab[k] < nbits) ok = (bits[lab[k] >> 6] >> (lab[k] & 63)) & 1ull;   // labels >= nbits are rejected
        const uint64_t b = __ballot(ok);
        if (lane == k) mine = b;
        c += (uint32_t)__popcll(b);
      }
      if (lane < kWordsPerWave && w0 + lane < words) dst[w0 + lane] = mine;
      if (lane == fl) my_cnt = c;
    }
    if (my_cnt) atomicAdd(&s_cnt[lane], my_cnt);
    __syncthreads();
    if (threadIdx.x < in_group && s_cnt[threadIdx.x]) atomicAdd(&counts[g + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    __syncthreads();
  }
}
}  // namespace

hipError_t launch_node_mask_build(const uint64_t *labels, const uint64_t *live, uint32_t count, const uint64_t *d_items, uint32_t n,
                                  unsigned long long *d_counts, hipStream_t s) {
  if (n == 0 || count == 0) return hipSuccess;
  const uint32_t words = (count + 63u) / 64u;
  const uint32_t blocks = (words + kWordsPerBlock - 1) / kWordsPerBlock;
  hipLaunchKernelGGL(node_mask_build_kernel, dim3(blocks), dim3(kThreads), 0, s, labels, live, count, words, d_items, n, d_counts);
  return hipGetLastError();
}

}  // namespace vk
