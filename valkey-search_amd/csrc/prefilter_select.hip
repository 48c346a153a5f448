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
#include "mfma_stage.hpp"
#include "prefilter_host.hpp"

#include <algorithm>

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

// ---- K8m: the distances of a shared list on the matrix cores ---------------------------------------------------------------
// K4's arithmetic (flat_gemm.hip) on gathered rows with a dense output.  The f32-input MFMA is a k-ordered fmaf chain, so one
// accumulator tile per lane class l, fed (chunk c, element l), (chunk c + 1, element l), ... in order, is chain l of
// quad_row_distance for 32 x 32 (query, entry) pairs at once; the 16 tiles are combined with quad_reduce16's tree.
//   block tile  = 128 list entries x tq queries (prefilter_mfma_tile_q); wave w owns entries [32w, 32w + 32) of the tile
//   operands    : A = queries, B = rows (a * b commutes: the bits are K4's), so a lane holds ONE entry for 16 queries and
//                 every output register is stored as 32 consecutive floats of one query's row of `out`
//   Q tile      : resident in LDS for the whole block, [tq][stride + 4] f32 (the pad keeps ds_read_b128 conflict free)
//   rows        : each wave gathers ITS 32 rows HBM -> registers -> its private LDS ring (3 stages of [32 rows][2 chunks], row
//                 stride 36 dwords) -> MFMA operands; no block barrier behind the Q tile's.  A lane reads its row slots once
//                 per tile and keeps the row bases in registers; the slots of the tile after the loader's are fetched a whole
//                 tile ahead, so the gather's dependent load never stands in front of a stage
//   grid        : nrp x nqt blocks, nrp (a multiple of 8) from the CU count; a block loads its query tile once and walks a
//                 contiguous range of row tiles; the nqt blocks of a range sit on one XCD, adjacent in dispatch order
// Entries past shared_len re-read the last valid one and are not stored; no row but idx[]'s is touched.
// (the stage helpers both matrix-core kernels share are in mfma_stage.hpp)
static_assert(kPrefilterMfmaRingBytes == 4 * kMfmaBufs * kMfmaBufFloats * 4, "prefilter_mfma_tile_q budgets this ring");

struct MfmaSlots { uint32_t s0, s1, s2, s3; };
struct MfmaBases { const char *b0, *b1, *b2, *b3; };

// the row slots of this lane's rows in tile `tile` (any tile: entries past the list re-read its last one)
template <bool kBf16>
__device__ __forceinline__ MfmaSlots mfma_tile_slots(const PrefilterDistArgs &a, uint32_t tile, uint32_t wave, uint32_t lane) {
  const uint32_t last = a.shared_len - 1;
  const uint32_t e = tile * kMfmaTile + wave * 32 + mfma_lane_row<kBf16>(lane);
  constexpr uint32_t step = kBf16 ? 16 : 8;
  MfmaSlots s;
  s.s0 = a.idx[e < last ? e : last];
  s.s1 = a.idx[e + step < last ? e + step : last];
  if constexpr (kBf16) {
    s.s2 = s.s0;
    s.s3 = s.s0;
  } else {
    s.s2 = a.idx[e + 2 * step < last ? e + 2 * step : last];
    s.s3 = a.idx[e + 3 * step < last ? e + 3 * step : last];
  }
  return s;
}
template <bool kBf16>
__device__ __forceinline__ MfmaBases mfma_bases(const PrefilterDistArgs &a, const MfmaSlots s, uint32_t lane) {
  const uint32_t piece = (kBf16 ? lane & 3 : lane & 7) * 16;
  MfmaBases b;
  b.b0 = row_base<kBf16>(a.rows, s.s0, a.row_stride_f) + piece;
  b.b1 = row_base<kBf16>(a.rows, s.s1, a.row_stride_f) + piece;
  b.b2 = row_base<kBf16>(a.rows, s.s2, a.row_stride_f) + piece;
  b.b3 = row_base<kBf16>(a.rows, s.s3, a.row_stride_f) + piece;
  return b;
}
// global -> registers, one stage (2 chunks) of the wave's 32 rows: one 64-bit add per 16-byte load
template <bool kBf16>
__device__ __forceinline__ MfmaStg mfma_stage_load(const MfmaBases b, uint32_t st) {
  const uint32_t off = st * (kBf16 ? 64u : 128u);
  MfmaStg s;
  s.v0 = *reinterpret_cast<const float4 *>(b.b0 + off);
  s.v1 = *reinterpret_cast<const float4 *>(b.b1 + off);
  if constexpr (kBf16) {
    s.v2 = s.v0;
    s.v3 = s.v0;
  } else {
    s.v2 = *reinterpret_cast<const float4 *>(b.b2 + off);
    s.v3 = *reinterpret_cast<const float4 *>(b.b3 + off);
  }
  return s;
}
// nrp row partitions (a multiple of 8) x nqt query tiles of tq; a.row_stride_f a multiple of 64, a.chunks = a.row_stride_f / 16
template <bool kBf16>
__global__ __launch_bounds__(256, 1) void prefilter_mfma_kernel(PrefilterDistArgs a, uint32_t nrp, uint32_t nqt, uint32_t tq) {
  extern __shared__ float4 mfma_lds[];
  float *lds = reinterpret_cast<float *>(mfma_lds);
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keep it in a scalar register
  const uint32_t li = lane & 31;   // query (A) / entry (B) index inside the 32-wide MFMA tile
  const uint32_t kk = lane >> 5;   // which of the two chunks of the stage this lane feeds
  const uint32_t width = a.row_stride_f;
  const uint32_t stages = width / 32;   // even: the ping-pong register sets keep their parity from tile to tile
  const uint32_t qstride = width + 4;
  // blocks b and b + 8 share an XCD: the nqt blocks that walk one row range are neighbours there (K8b's and K4's dealing)
  const uint32_t xcd = blockIdx.x & 7u, seq = blockIdx.x >> 3;
  const uint32_t rp = (seq / nqt) * 8u + xcd;
  const uint32_t q0 = (seq % nqt) * tq;
  const uint32_t n_tiles = (a.shared_len + kMfmaTile - 1) / kMfmaTile;
  const uint32_t t_base = n_tiles / nrp, t_rem = n_tiles % nrp;
  const uint32_t first_tile = rp * t_base + (rp < t_rem ? rp : t_rem);
  const uint32_t my_tiles = t_base + (rp < t_rem ? 1u : 0u);
  if (my_tiles == 0) return;   // (block-uniform) more partitions than tiles

  float *lds_q = lds;   // [tq][qstride], read-only behind the barrier
  float *lds_x = lds + (size_t)tq * qstride + (size_t)wave * kMfmaBufs * kMfmaBufFloats;
  // ---- Q tile -> LDS (queries past nq replicate the last one; their results are discarded)
  for (uint32_t i = tid; i < tq * (width / 4); i += 256) {
    const uint32_t q = i / (width / 4), c4 = i % (width / 4);
    const uint32_t gq = q0 + q < a.nq ? q0 + q : a.nq - 1;
    *reinterpret_cast<float4 *>(lds_q + (size_t)q * qstride + c4 * 4) = reinterpret_cast<const float4 *>(a.queries + (size_t)gq * a.q_stride_f)[c4];
  }

  // ---- the loader's place in this block's flattened (tile, stage) stream.  `rb` = its tile's row bases, `next` = the slots of
  // the tile behind it, requested when the loader entered its tile and looked at only when it leaves it.  The loader never moves
  // past the last stage of the stream: the prefetches issued behind the end re-read that stage and are not used.
  uint32_t ld_tile = first_tile, ld_st = 0, ld_left = my_tiles * stages;   // (< 2^32: at most 2^25 tiles of at most 52 stages)
  MfmaBases rb = mfma_bases<kBf16>(a, mfma_tile_slots<kBf16>(a, ld_tile, wave, lane), lane);
  MfmaSlots next = mfma_tile_slots<kBf16>(a, ld_tile + 1, wave, lane);
#define VK_PF_ADVANCE()                                            \
  if (ld_left > 1) { /* (wave-uniform, between two stages) */      \
    --ld_left;                                                     \
    if (++ld_st == stages) {                                       \
      ld_st = 0;                                                   \
      ++ld_tile;                                                   \
      rb = mfma_bases<kBf16>(a, next, lane);                       \
      next = mfma_tile_slots<kBf16>(a, ld_tile + 1, wave, lane);   \
    }                                                              \
  }
  // Software pipeline over the stream, iteration i = stage i (K4's): the global loads of stage i + 3 are issued at the top of
  // i, written to LDS at the bottom of i + 1, read LDS -> registers during i + 2, multiplied during i + 3.  Stage s lives in
  // ring buffer s % 3.  Unrolled by two with ping-pong register sets.
  MfmaStg stg_a, stg_b;
  stg_a = mfma_stage_load<kBf16>(rb, ld_st);
  mfma_stage_store<kBf16>(lds_x, lane, stg_a);
  VK_PF_ADVANCE()
  stg_a = mfma_stage_load<kBf16>(rb, ld_st);
  mfma_stage_store<kBf16>(lds_x + kMfmaBufFloats, lane, stg_a);
  VK_PF_ADVANCE()
  stg_a = mfma_stage_load<kBf16>(rb, ld_st);
  stg_b = stg_a;
  VK_PF_ADVANCE()
  __syncthreads();   // the shared Q tile is in place

  const uint32_t x_off = li * kMfmaXStride + kk * 16;
  const float *q_row = lds_q + (size_t)(li < tq ? li : tq - 1) * qstride;
  MfmaFrag f0 = mfma_frag_load(lds_x + x_off, q_row, 0, kk), f1 = f0;
  uint32_t rbuf = 1;   // buffer of stage done + 1
  uint32_t wbuf = 2;   // buffer of stage done + 2

  // one iteration: F = fragments of stage ST, NF receives the next stage's, SNEW the loads of stage done + 3, SOLD (the loads
  // of stage done + 2) goes to LDS; the memory operations are pinned between the 16 MFMAs as in K4 (VK_MFMA_STAGE_SCHED)
#define VK_PF_STAGE(ZERO, ST, F, NF, SNEW, SOLD)                                                  \
  {                                                                                               \
    const uint32_t nst = (ST) + 1 == stages ? 0u : (ST) + 1;                                      \
    SNEW = mfma_stage_load<kBf16>(rb, ld_st);                                                     \
    mfma_stage_mul<ZERO>(acc, F);                                                                 \
    NF = mfma_frag_load(lds_x + rbuf * kMfmaBufFloats + x_off, q_row, nst, kk);                   \
    mfma_stage_store<kBf16>(lds_x + wbuf * kMfmaBufFloats, lane, SOLD);                           \
    VK_MFMA_STAGE_SCHED()                                                                         \
    rbuf = rbuf == 2 ? 0u : rbuf + 1;                                                           \
    wbuf = wbuf == 2 ? 0u : wbuf + 1;                                                             \
    VK_PF_ADVANCE()                                                                               \
  }

  for (uint32_t t = 0; t < my_tiles; ++t) {
    f32x16 acc[16];
    VK_PF_STAGE(true, 0u, f0, f1, stg_b, stg_a)   // accumulators are born from a zero C operand
    VK_PF_STAGE(false, 1u, f1, f0, stg_a, stg_b)
    for (uint32_t st = 2; st < stages; st += 2) {
      VK_PF_STAGE(false, st, f0, f1, stg_b, stg_a)
      VK_PF_STAGE(false, st + 1, f1, f0, stg_a, stg_b)
    }
    // ---- tile done.  Per output register r (query (r & 3) + 8 (r >> 2) + 4 kk of the tile, this lane's entry): the 16 class
    // sums combined with _mm512_reduce_add_ps's pairing (l, l + 8) -> (l, l + 4) -> (l, l + 2) -> (0, 1), then 1 - dot
    const uint32_t e = (first_tile + t) * kMfmaTile + wave * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v[16];
#pragma unroll
      for (int l = 0; l < 16; ++l) v[l] = acc[l][r];
#pragma unroll
      for (int l = 0; l < 8; ++l) v[l] = v[l + 8] + v[l];
#pragma unroll
      for (int l = 0; l < 4; ++l) v[l] = v[l + 4] + v[l];
      const float dot = (v[0] + v[2]) + (v[1] + v[3]);
      const uint32_t qi = (uint32_t)((r & 3) + 8 * (r >> 2)) + 4 * kk;
      if (qi < tq && q0 + qi < a.nq && e < a.shared_len) a.out[(size_t)(q0 + qi) * a.shared_len + e] = 1.0f - dot;
      // keep the 16 gathers of one output register together: hoisting all 256 accumulator reads ahead of the adds would
      // need 256 more registers and spill into the pipelined loop (K4)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#undef VK_PF_STAGE
#undef VK_PF_ADVANCE
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

// K8m's launch: the grid from the CU count and the number of query tiles -- every CU one block while there are that many row
// tiles, and with nq <= tq every row leaves HBM once
hipError_t launch_prefilter_mfma(const PrefilterDistArgs &a, bool bf16, hipStream_t s) {
  uint32_t tq = prefilter_mfma_tile_q(a.row_stride_f);
  uint32_t nqt = (a.nq + tq - 1) / tq;
  const uint32_t n_tiles = (a.shared_len + kMfmaTile - 1) / kMfmaTile;
  int dev = 0, cus = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  uint32_t nrp = std::max<uint32_t>(8, ((uint32_t)(cus > 0 ? cus : 256) / nqt) & ~7u);
  nrp = std::min<uint32_t>(nrp, (n_tiles + 7) & ~7u);
  if ((uint64_t)nrp * nqt > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const size_t lds = (size_t)tq * (a.row_stride_f + 4) * 4 + kPrefilterMfmaRingBytes;
  const void *f = bf16 ? reinterpret_cast<const void *>(&prefilter_mfma_kernel<true>) : reinterpret_cast<const void *>(&prefilter_mfma_kernel<false>);
  hipError_t e = ensure_max_lds(f);
  if (e != hipSuccess) return e;
  PrefilterDistArgs args = a;
  void *params[] = {&args, &nrp, &nqt, &tq};
  return hipLaunchKernel(f, dim3(nrp * nqt), dim3(256), params, lds, s);
}

}  // namespace

uint32_t prefilter_tiles(uint64_t entries) { return (uint32_t)((entries + kTileEntries - 1) / kTileEntries); }

hipError_t launch_prefilter_distance(const PrefilterDistArgs &a, bool l2, bool bf16, hipStream_t s) {
  // K8m: the caller's wish and the drivers' own decision function; a launch it does not take runs K8b exactly as before
  if (prefilter_takes_mfma(a.mfma != 0, a.seg_begin == nullptr, l2, a.row_stride_f, a.nq) && a.shared_len != 0 &&
      a.chunks * 16 == a.row_stride_f && a.q_stride_f >= a.row_stride_f)
    return launch_prefilter_mfma(a, bf16, s);
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
