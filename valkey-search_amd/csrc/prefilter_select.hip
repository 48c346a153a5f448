// prefilter_select.hip -- the device stage of the batched pre-filter search (vk_index_search_labels_batch), gfx950.
//
//   K8b  prefilter_distance_kernel   distances of nq queries over a CSR of row-slot lists (one segment per query, or one
//                                    shared segment for all queries): out[e] = quad_row_distance(row, query_of(e)), the
//                                    function and lane layout of K8 (gather_distance_kernel), so every distance has the
//                                    bits the single-query path produces
//   K8c  prefilter_select_kernel     per query: T = the k-th smallest distance of its segment (the maximum when the
//                                    segment has fewer than k entries), then every entry <= T, IN LIST ORDER, as
//                                    (index in the segment, distance), and their number
//
// The host (prefilter_batch.cc) runs the reference's heap rule (vector_base.cc:509-530) over those entries only.
//
// Why that is exact (prefilter_host.hpp has the same note).  The rule's answer depends only on the entries with distance
// <= T and their relative order: after i entries the heap's distances are the min(i, k) smallest seen; an entry above T is
// only ever evicted by, or refused in favour of, something smaller, and never displaces an entry <= T; an entry <= T meets
// a heap that is not full, or a top above T, exactly when the run over the <= T subsequence alone would have had room for
// it.  So the rule over any superset of {distance <= T}, in list order, gives the same heap -- which is why the hand-back
// may hold more than k entries (ties at T, up to `cap`), and why a sharded index may take the union of its shards'.
//
// K8b's grid covers (query, tile) pairs, a tile = 64 entries = one 16-row wave tile for each of the block's four waves;
// the block's query sits in dynamic LDS like K8's (up to the 160 KB of a CU: D <= 40 960).  With a shared list the nq
// blocks that read one tile's rows should find them in L2 (4 MB per XCD, not shared between the eight XCDs; a tile of
// 768-d f32 rows is 192 KB) instead of going to HBM nq times.  Blocks are dealt round-robin over the XCDs (b and b + 8
// share one), so the block index is read as (group g = b / 8, residue x = b % 8): query g % nq, tile (g / nq) * 8 + x --
// the queries run fastest, and the nq blocks of a tile are dispatched close together in time AND on one XCD.  (Placement
// is an observation, not a promise: a different dealing costs speed only.)
//
// K8c is one block per query.  The threshold is the binary descent of wave_select (flat_scan.hip) over merge_key's
// order-preserving u32, block-wide: 32 counting passes, the first kSelReg x 256 keys from registers, the rest of a long
// segment re-read from memory (L2) in every pass.  The compaction is a block-wide prefix sum walked front to back, one
// barrier per 256 entries: no atomics, so the order is the list's.  Plain vector loads and stores and LDS only.
#include "device_common.hpp"
#include "kernels.hpp"
#include "prefilter_host.hpp"

namespace vk {

namespace {

constexpr uint32_t kTileEntries = 64;   // per block: 4 waves x kRowsPerWave
constexpr int kSelReg = 8;              // keys per thread the descent keeps in registers (segments up to 2048 never re-read)

__device__ __forceinline__ uint32_t select_key(float f) {   // merge_key of flat_scan.hip
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool kL2, bool kBf16>
__global__ __launch_bounds__(256) void prefilter_distance_kernel(PrefilterDistArgs a) {
  extern __shared__ float4 qs[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 3;
  const int rq = lane >> 2;
  const uint32_t chunks = a.chunks;
  // which (query, tile) this block serves
  uint32_t q, tile, seg_lo, seg_len;
  size_t out_lo;
  if (a.seg_begin == nullptr) {   // one shared segment: queries fastest, a tile's readers on one XCD (header comment)
    const uint32_t g = blockIdx.x >> 3;
    q = g % a.nq;
    tile = (g / a.nq) * 8 + (blockIdx.x & 7);
    if (tile * kTileEntries >= a.shared_len) return;   // (block-uniform: the tile count rounded up to eight)
    seg_lo = 0;
    seg_len = a.shared_len;
    out_lo = (size_t)q * a.shared_len;
  } else {                        // the query whose tile range holds this block: tile_begin[q] <= block < tile_begin[q + 1]
    uint32_t lo = 0, hi = a.nq;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.tile_begin[mid] <= blockIdx.x) lo = mid; else hi = mid;
    }
    q = lo;
    tile = blockIdx.x - a.tile_begin[q];
    seg_lo = a.seg_begin[q];
    seg_len = a.seg_begin[q + 1] - seg_lo;
    out_lo = seg_lo;
  }
  const float4 *__restrict__ query = reinterpret_cast<const float4 *>(a.queries + (size_t)q * a.q_stride_f);
  for (uint32_t i = threadIdx.x; i < chunks * 4; i += blockDim.x) qs[i] = query[i];
  __syncthreads();
  const uint32_t i = tile * kTileEntries + (uint32_t)wave * kRowsPerWave + rq;
  const bool valid = i < seg_len;   // (seg_len >= 1: a query without entries has no tile)
  const uint32_t row = a.idx[seg_lo + (valid ? i : seg_len - 1)];
  const float dist = quad_row_distance<kL2, kBf16>(row_base<kBf16>(a.rows, row, a.row_stride_f), qs, chunks, j);
  if (valid && j == 0) a.out[out_lo + i] = dist;
}

__global__ __launch_bounds__(256) void prefilter_select_kernel(PrefilterSelectArgs a) {
  __shared__ uint32_t s_cnt[2][4];
  const uint32_t q = blockIdx.x;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t n;
  const float *__restrict__ d;
  if (a.seg_begin == nullptr) {
    n = a.shared_len;
    d = a.dist + (size_t)q * a.shared_len;
  } else {
    const uint32_t lo = a.seg_begin[q];
    n = a.seg_begin[q + 1] - lo;
    d = a.dist + lo;
  }
  if (n == 0) {
    if (tid == 0) a.count[q] = 0;
    return;
  }
  // the keys: the first kSelReg * 256 in registers (an entry past the end: all ones, below no threshold)
  uint32_t key[kSelReg];
  int nan = 0;
#pragma unroll
  for (int u = 0; u < kSelReg; ++u) {
    const uint32_t i = tid + 256u * u;
    key[u] = 0xFFFFFFFFu;
    if (i < n) {
      const float v = d[i];
      nan |= v != v;
      key[u] = select_key(v);
    }
  }
  for (uint32_t base = 256u * kSelReg; base < n; base += 256) {
    const uint32_t i = base + tid;
    if (i < n) { const float v = d[i]; nan |= v != v; }
  }
  if (__syncthreads_or(nan)) {   // a NaN has no place in the order: the per-query path answers
    if (tid == 0) a.count[q] = kPrefilterCountNaN;
    return;
  }
  uint32_t phase = 0;
  // block-wide sum of the waves' (uniform) counts through LDS, one barrier (the two halves of s_cnt alternate)
  auto block_sum = [&](uint32_t mine) -> uint32_t {
    if (lane == 0) s_cnt[phase][wave] = mine;
    __syncthreads();
    const uint32_t t = s_cnt[phase][0] + s_cnt[phase][1] + s_cnt[phase][2] + s_cnt[phase][3];
    phase ^= 1;
    return t;
  };
  // T = the k-th smallest key = the largest T with count(key < T) < k; all ones when the segment has fewer than k entries
  uint32_t T = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t cand = T | (1u << bit);
    uint32_t c = 0;
#pragma unroll
    for (int u = 0; u < kSelReg; ++u) c += (uint32_t)__popcll(__ballot(key[u] < cand));
    for (uint32_t base = 256u * kSelReg; base < n; base += 256) {
      const uint32_t i = base + tid;
      const uint32_t kk = i < n ? select_key(d[i]) : 0xFFFFFFFFu;
      c += (uint32_t)__popcll(__ballot(kk < cand));
    }
    if (block_sum(c) < a.k) T = cand;
  }
  // every entry <= T, front to back
  uint2 *__restrict__ out = a.cand + (size_t)q * a.cap;
  uint32_t running = 0;
  for (uint32_t base = 0; base < n; base += 256) {
    const uint32_t i = base + tid;
    float v = 0.f;
    bool keep = false;
    if (i < n) {
      v = d[i];
      keep = select_key(v) <= T;
    }
    const uint64_t b = __ballot(keep);
    if (lane == 0) s_cnt[phase][wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
      const uint32_t c = s_cnt[phase][w];
      before += w < wave ? c : 0u;
      total += c;
    }
    phase ^= 1;
    const uint32_t at = running + before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (keep && at < a.cap) out[at] = make_uint2(i, __float_as_uint(v));
    running += total;
    if (running > a.cap) break;   // (block-uniform) ties at T beyond the hand-back: the per-query path answers
  }
  if (tid == 0) a.count[q] = running;
}

}  // namespace

uint32_t prefilter_tiles(uint64_t entries) { return (uint32_t)((entries + kTileEntries - 1) / kTileEntries); }

hipError_t launch_prefilter_distance(const PrefilterDistArgs &a, bool l2, bool bf16, hipStream_t s) {
  // shared segment: (tiles rounded up to eight) x nq blocks; CSR: the host's tile_begin[nq] = a.n_tiles
  const uint64_t blocks = a.seg_begin == nullptr ? (uint64_t)((prefilter_tiles(a.shared_len) + 7) / 8) * 8 * a.nq : a.n_tiles;
  if (blocks == 0) return hipSuccess;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const size_t lds = (size_t)a.chunks * 64;
  if (lds > 160 * 1024 || a.nq == 0) return hipErrorInvalidValue;
  const void *f = l2 ? (bf16 ? reinterpret_cast<const void *>(&prefilter_distance_kernel<true, true>)
                             : reinterpret_cast<const void *>(&prefilter_distance_kernel<true, false>))
                     : (bf16 ? reinterpret_cast<const void *>(&prefilter_distance_kernel<false, true>)
                             : reinterpret_cast<const void *>(&prefilter_distance_kernel<false, false>));
  if (lds > 48 * 1024) {
    hipError_t e = ensure_max_lds(f);
    if (e != hipSuccess) return e;
  }
  PrefilterDistArgs args = a;
  void *params[] = {&args};
  return hipLaunchKernel(f, dim3((uint32_t)blocks), dim3(256), params, lds, s);
}

hipError_t launch_prefilter_select(const PrefilterSelectArgs &a, hipStream_t s) {
  if (a.nq == 0) return hipSuccess;
  if (a.k == 0 || a.cap < a.k) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prefilter_select_kernel, dim3(a.nq), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace vk
