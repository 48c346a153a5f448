// flat_large_k.hip -- FLAT search with k > 1024 in ONE pass over the rows, gfx950 (option flat-large-k; FlatIndex::search_large_k).
// The paged path (FlatIndex::search_in_passes) scans the whole table once per 1024 results and query; here a chunk of queries
// costs one dense distance pass, a radix select of every query's k-th key over the distances it wrote, and a compaction of
// what lies at or below that key.  The host orders each hand-back and cuts it at k (flat_large_k_host.hpp) -- or, with option
// flat-large-k-device-sort, the device does: a tile sort and merge passes behind the emit (described where they stand).
//
//   flat_dense_distance_kernel   dist[q][row] for rows [0, count) and the qb queries of the block (grid.y = query groups,
//                                flat_scan_pick_qb's choice): the block's queries sit in LDS, a wave owns 16 rows at a time, one
//                                per quad, and every distance is quad_row_distance over the query's fragments -- the function
//                                and the lane layout of K8 / K8b, so the bits are the single-query path's.  A row tile is
//                                fetched from HBM once per block: the qb - 1 further walks over it come out of the cache.  A
//                                row that cannot be an answer (label kNoLabel, rejected by the bitmap) gets a NaN, and NaN is
//                                the one "not a candidate" class from there on: K3 never lists a NaN distance either
//                                (dist <= thr is false).  The waves stride over the row tiles; nothing at or beyond count is
//                                written.
//   flat_dense_mfma_kernel       the same matrix, bit for bit, from the matrix cores (option flat-large-k-mfma; IP / COSINE, chunks
//                                of five or more queries, strides that are a multiple of 64 floats up to 1664 -- large_k_takes_mfma
//                                of flat_large_k_host.hpp; everything else, L2 and a short last chunk included, stays on the
//                                kernel above).  128 rows x 32 / 24 / 16 queries per block, v_mfma_f32_32x32x2_f32 as sixteen
//                                k-ordered chains; described where it stands.
//   flat_large_k_hist_kernel    one digit of the select: grid (slices of kLargeKSlice entries) x (queries).  The block counts
//   flat_large_k_pick_kernel     the digit of every non-NaN entry whose higher digits equal the prefix chosen so far in LDS
//                                bins and adds the bins that are not empty into hist[q][] with one vector atomicAdd each; one
//                                wave per query then finds the bin that holds the k-th entry, extends the prefix, and clears
//                                the bins for the next digit.  Behind the last digit the state holds T (the key of the k-th
//                                smallest candidate, the largest key when there are fewer than k, 0 when there is none),
//                                n_less, n_eq, n_real, a zeroed emit counter and the overflow flag (n_less + n_eq > cap).
//   flat_large_k_emit_kernel     same grid: every candidate with key <= T goes out as (distance bits, labels[row]); a wave
//                                counts its entries over the whole slice first and takes its slots with ONE vector atomicAdd
//                                on the query's counter.  A flagged query writes nothing.
//
// The key is merge_key of flat_scan.hip: order-preserving u32 of the float, -0 and +0 sharing a key.
// Digits: 11 | 11 | 10 bits from the top.  Three digits instead of four (8 x 4) are three walks over the distances and six
// launches instead of four and eight; 2048 bins are 8 KB of LDS per block -- nineteen blocks' worth in a CU's 160 KB, so the
// bins never bound the occupancy -- and one wave still sums them in 32 loads per lane.  Wider digits (16 x 2) would need
// 256 KB of bins.  Distances of one query crowd into a few bins of the top digit; before the LDS atomics a wave takes out
// the lanes that share the first active lane's bin and adds their number once.
//
// No kernel waits for another block: no grid barrier, no spin loop, every loop bound is an argument or a constant.  Plain
// vector loads and stores, LDS, and vector atomics (LDS and global atomicAdd) only; the sort kernels use no atomics.
#include "device_common.hpp"
#include "flat_large_k_host.hpp"
#include "kernels.hpp"
#include "mfma_stage.hpp"

#include <algorithm>

namespace vk {

namespace {

constexpr uint32_t kLargeKThreads = 256;
constexpr uint32_t kLargeKPerThread = 16;
constexpr uint32_t kLargeKSlice = kLargeKThreads * kLargeKPerThread;   // 4096 entries per block of the histogram / emit launches
constexpr uint32_t kLargeKDistBlocks = 2048;                           // row blocks of the distance launch: eight per CU
constexpr int kLargeKDigits = 3;

// digit d covers key bits [shift, shift + width)
__host__ __device__ __forceinline__ uint32_t digit_shift(int d) { return d == 0 ? 21u : d == 1 ? 10u : 0u; }
__host__ __device__ __forceinline__ uint32_t digit_bins(int d) { return d == 2 ? 1024u : 2048u; }

__device__ __forceinline__ uint32_t large_k_dev_key(float f) {   // merge_key (flat_scan.hip)
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool kL2, bool kBf16>
__global__ __launch_bounds__(256) void flat_dense_distance_kernel(FlatLargeKArgs a, uint32_t qb) {
  extern __shared__ float4 qs[];   // [qb][chunks][4] float4 = qb padded queries
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int j = lane & 3;
  const int rq = lane >> 2;
  const uint32_t chunks = a.chunks;
  const uint32_t qbase = blockIdx.y * qb;
  const uint32_t per_q = chunks * 4;
  // queries past the chunk's end replicate its last one (never evaluated)
  for (uint32_t i = threadIdx.x; i < per_q * qb; i += blockDim.x) {
    const uint32_t qi = i / per_q, off = i - qi * per_q;
    const uint32_t q = qbase + qi < a.qc ? qbase + qi : a.qc - 1;
    qs[i] = reinterpret_cast<const float4 *>(a.queries + (size_t)q * a.q_stride_f)[off];
  }
  __syncthreads();
  const uint32_t n_q = a.qc - qbase < qb ? a.qc - qbase : qb;   // block-uniform
  const uint32_t total_waves = gridDim.x * 4;
  const uint32_t n_tiles = (a.count + kRowsPerWave - 1) / kRowsPerWave;
  for (uint32_t tile = blockIdx.x * 4 + wave; tile < n_tiles; tile += total_waves) {
    const uint32_t row = tile * kRowsPerWave + rq;
    const bool valid = row < a.count;
    const uint32_t lrow = valid ? row : a.count - 1;
    const char *__restrict__ base = row_base<kBf16>(a.rows, lrow, a.row_stride_f);
    const uint64_t lab = a.labels[lrow];
    const bool cand = lab != kNoLabel && allow_bit(a.allow_bits, a.allow_nbits, lab);
    for (uint32_t qi = 0; qi < n_q; ++qi) {
      const float d = quad_row_distance<kL2, kBf16>(base, qs + (size_t)qi * per_q, chunks, j);
      if (valid && j == 0) a.dist[(size_t)(qbase + qi) * a.ld + row] = cand ? d : __builtin_nanf("");
    }
  }
}

// ---- the dense distances on the matrix cores (option flat-large-k-mfma) -----------------------------------------------------------
// flat_dense_distance_kernel<false, kBf16>'s matrix for a chunk of five or more queries, bit for bit: K8m's arithmetic and pipeline
// (prefilter_select.hip; the stage helpers are shared, mfma_stage.hpp) over CONTIGUOUS rows.  The f32-input MFMA is a k-ordered
// fmaf chain: one accumulator tile per lane class l, fed (chunk c, element l), (chunk c + 1, element l), ... in order, is chain l
// of quad_row_distance for 32 x 32 (query, row) pairs; the 16 tiles are combined with quad_reduce16's tree, then 1 - dot.
//   block tile  = 128 rows x tq queries (prefilter_mfma_tile_q); wave w owns rows [32w, 32w + 32) of the tile; A = queries, B = rows
//   Q tile      : resident in LDS, [tq][stride + 4] f32; rows: HBM -> registers -> the wave's private ring (3 stages of [32 rows]
//                 [36 dwords]) -> MFMA operands, software pipeline unrolled by two, no block barrier behind the Q tile's
//   rows        : no slot list.  A lane's four (bf16: two) 16-byte loads of a stage are at tile base + a per-lane 32-bit offset +
//                 stage * 128 (64) bytes: the tile base is wave-uniform and moves by 128 rows at a tile boundary of the loader's
//                 flattened (tile, stage) stream; the offsets are per-lane constants -- (row in the tile) * row bytes + piece --
//                 except in a ragged last tile, where a row past count - 1 takes the offset of row count - 1 (re-read, not stored)
//   mask        : lane li owns row tile * 128 + wave * 32 + li for all 16 of its output registers: its label is requested when
//                 the tile starts and its allow bit behind the tile's first two stages, both looked at in the epilogue only, which
//                 stores NaN or 1 - dot
//   stores      : every output register is 32 consecutive floats of one query's row of dist, at (q0 + qi) * ld + row
//   grid        : nrp x nqt blocks, nrp (a multiple of 8) from the CU count; a block walks a contiguous range of row tiles; the
//                 nqt blocks of a range sit on one XCD, adjacent in dispatch order
// Nothing at or beyond count is read or written.  Plain vector loads and stores and LDS; every loop bound is an argument.
static_assert(kPrefilterMfmaRingBytes == 4 * kMfmaBufs * kMfmaBufFloats * 4, "prefilter_mfma_tile_q budgets this ring");

struct DenseOffs { uint32_t o0, o1, o2, o3; };   // by value, like the stage sets

// this lane's byte offsets from the first row of tile `tile` (< n_tiles) to the pieces it stages; at most 127 rows of at most
// 6656 bytes: 32 bits hold them
template <bool kBf16>
__device__ __forceinline__ DenseOffs dense_tile_offs(uint32_t count, uint32_t tile, uint32_t wave, uint32_t lane, uint32_t row_bytes) {
  const uint32_t lim = count - 1 - tile * kMfmaTile;   // the last row of the table, counted from the tile's first (wave-uniform)
  const uint32_t r = wave * 32 + mfma_lane_row<kBf16>(lane);
  const uint32_t piece = (kBf16 ? lane & 3 : lane & 7) * 16;
  constexpr uint32_t step = kBf16 ? 16 : 8;
  DenseOffs o;
  o.o0 = (r < lim ? r : lim) * row_bytes + piece;
  o.o1 = (r + step < lim ? r + step : lim) * row_bytes + piece;
  if constexpr (kBf16) {
    o.o2 = o.o0;
    o.o3 = o.o0;
  } else {
    o.o2 = (r + 2 * step < lim ? r + 2 * step : lim) * row_bytes + piece;
    o.o3 = (r + 3 * step < lim ? r + 3 * step : lim) * row_bytes + piece;
  }
  return o;
}
// global -> registers, one stage (2 chunks) of the wave's 32 rows: a uniform base, a 32-bit add per 16-byte load
template <bool kBf16>
__device__ __forceinline__ MfmaStg dense_stage_load(const char *tile_base, const DenseOffs o, uint32_t st) {
  const uint32_t off = st * (kBf16 ? 64u : 128u);
  MfmaStg s;
  s.v0 = *reinterpret_cast<const float4 *>(tile_base + (o.o0 + off));
  s.v1 = *reinterpret_cast<const float4 *>(tile_base + (o.o1 + off));
  if constexpr (kBf16) {
    s.v2 = s.v0;
    s.v3 = s.v0;
  } else {
    s.v2 = *reinterpret_cast<const float4 *>(tile_base + (o.o2 + off));
    s.v3 = *reinterpret_cast<const float4 *>(tile_base + (o.o3 + off));
  }
  return s;
}

// nrp row partitions (a multiple of 8) x nqt query tiles of tq; a.row_stride_f a multiple of 64, a.chunks = a.row_stride_f / 16
template <bool kBf16>
__global__ __launch_bounds__(256, 1) void flat_dense_mfma_kernel(FlatLargeKArgs a, uint32_t nrp, uint32_t nqt, uint32_t tq) {
  extern __shared__ float4 mfma_lds[];
  float *lds = reinterpret_cast<float *>(mfma_lds);
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: keep it in a scalar register
  const uint32_t li = lane & 31;   // query (A) / row (B) index inside the 32-wide MFMA tile
  const uint32_t kk = lane >> 5;   // which of the two chunks of the stage this lane feeds
  const uint32_t width = a.row_stride_f;
  const uint32_t stages = width / 32;   // even: the ping-pong register sets keep their parity from tile to tile
  const uint32_t qstride = width + 4;
  const uint32_t row_bytes = width * (kBf16 ? 2u : 4u);
  // blocks b and b + 8 share an XCD: the nqt blocks that walk one row range are neighbours there (K8m's and K4's dealing)
  const uint32_t xcd = blockIdx.x & 7u, seq = blockIdx.x >> 3;
  const uint32_t rp = (seq / nqt) * 8u + xcd;
  const uint32_t q0 = (seq % nqt) * tq;
  const uint32_t n_tiles = (uint32_t)(((uint64_t)a.count + kMfmaTile - 1) / kMfmaTile);
  const uint32_t t_base = n_tiles / nrp, t_rem = n_tiles % nrp;
  const uint32_t first_tile = rp * t_base + (rp < t_rem ? rp : t_rem);
  const uint32_t my_tiles = t_base + (rp < t_rem ? 1u : 0u);
  if (my_tiles == 0) return;   // (block-uniform) more partitions than tiles

  float *lds_q = lds;   // [tq][qstride], read-only behind the barrier
  float *lds_x = lds + (size_t)tq * qstride + (size_t)wave * kMfmaBufs * kMfmaBufFloats;
  // ---- Q tile -> LDS (queries past qc replicate the last one; their results are discarded)
  for (uint32_t i = tid; i < tq * (width / 4); i += 256) {
    const uint32_t q = i / (width / 4), c4 = i % (width / 4);
    const uint32_t gq = q0 + q < a.qc ? q0 + q : a.qc - 1;
    *reinterpret_cast<float4 *>(lds_q + (size_t)q * qstride + c4 * 4) = reinterpret_cast<const float4 *>(a.queries + (size_t)gq * a.q_stride_f)[c4];
  }

  // ---- the loader's place in this block's flattened (tile, stage) stream: its tile's first row and this lane's offsets from
  // there.  The loader never moves past the last stage of the stream: the prefetches issued behind the end re-read that stage
  // and are not used.
  uint32_t ld_tile = first_tile, ld_st = 0, ld_left = my_tiles * stages;   // (< 2^32: at most 2^25 tiles of at most 52 stages)
  const size_t tile_bytes = (size_t)kMfmaTile * row_bytes;
  const char *ld_base = static_cast<const char *>(a.rows) + (size_t)ld_tile * tile_bytes;
  DenseOffs ro = dense_tile_offs<kBf16>(a.count, ld_tile, wave, lane, row_bytes);
#define VK_LK_ADVANCE()                                                           \
  if (ld_left > 1) { /* (wave-uniform, between two stages) */                     \
    --ld_left;                                                                    \
    if (++ld_st == stages) {                                                      \
      ld_st = 0;                                                                  \
      ++ld_tile;                                                                  \
      ld_base += tile_bytes;                                                      \
      ro = dense_tile_offs<kBf16>(a.count, ld_tile, wave, lane, row_bytes);       \
    }                                                                             \
  }
  // Software pipeline over the stream, iteration i = stage i (K8m's, K4's): the global loads of stage i + 3 are issued at the top
  // of i, written to LDS at the bottom of i + 1, read LDS -> registers during i + 2, multiplied during i + 3.  Stage s lives in
  // ring buffer s % 3.  Unrolled by two with ping-pong register sets.
  MfmaStg stg_a, stg_b;
  stg_a = dense_stage_load<kBf16>(ld_base, ro, ld_st);
  mfma_stage_store<kBf16>(lds_x, lane, stg_a);
  VK_LK_ADVANCE()
  stg_a = dense_stage_load<kBf16>(ld_base, ro, ld_st);
  mfma_stage_store<kBf16>(lds_x + kMfmaBufFloats, lane, stg_a);
  VK_LK_ADVANCE()
  stg_a = dense_stage_load<kBf16>(ld_base, ro, ld_st);
  stg_b = stg_a;
  VK_LK_ADVANCE()
  __syncthreads();   // the shared Q tile is in place

  const uint32_t x_off = li * kMfmaXStride + kk * 16;
  const float *q_row = lds_q + (size_t)(li < tq ? li : tq - 1) * qstride;
  MfmaFrag f0 = mfma_frag_load(lds_x + x_off, q_row, 0, kk), f1 = f0;
  uint32_t rbuf = 1;   // buffer of stage done + 1
  uint32_t wbuf = 2;   // buffer of stage done + 2

  // one iteration: F = fragments of stage ST, NF receives the next stage's, SNEW the loads of stage done + 3, SOLD (the loads
  // of stage done + 2) goes to LDS; the memory operations are pinned between the 16 MFMAs (VK_MFMA_STAGE_SCHED)
#define VK_LK_STAGE(ZERO, ST, F, NF, SNEW, SOLD)                                                  \
  {                                                                                               \
    const uint32_t nst = (ST) + 1 == stages ? 0u : (ST) + 1;                                      \
    SNEW = dense_stage_load<kBf16>(ld_base, ro, ld_st);                                           \
    mfma_stage_mul<ZERO>(acc, F);                                                                 \
    NF = mfma_frag_load(lds_x + rbuf * kMfmaBufFloats + x_off, q_row, nst, kk);                   \
    mfma_stage_store<kBf16>(lds_x + wbuf * kMfmaBufFloats, lane, SOLD);                           \
    VK_MFMA_STAGE_SCHED()                                                                         \
    rbuf = rbuf == 2 ? 0u : rbuf + 1;                                                             \
    wbuf = wbuf == 2 ? 0u : wbuf + 1;                                                             \
    VK_LK_ADVANCE()                                                                               \
  }

  for (uint32_t t = 0; t < my_tiles; ++t) {
    // this lane's row of the tile: in the table while its place in the tile is at or below the table's last row's
    const uint32_t lim = a.count - 1 - (first_tile + t) * kMfmaTile;
    const uint32_t in_tile = wave * 32 + li;
    const bool valid = in_tile <= lim;
    const size_t row = (size_t)(first_tile + t) * kMfmaTile + (valid ? in_tile : lim);
    const uint64_t lab = a.labels[row];   // requested now, looked at in the epilogue
    __builtin_amdgcn_sched_barrier(0);    // (not one of the loads the first stage pins between its MFMAs)
    f32x16 acc[16];
    VK_LK_STAGE(true, 0u, f0, f1, stg_b, stg_a)   // accumulators are born from a zero C operand
    VK_LK_STAGE(false, 1u, f1, f0, stg_a, stg_b)
    const bool cand = lab != kNoLabel && allow_bit(a.allow_bits, a.allow_nbits, lab);   // (the label is here by now; the bit: epilogue)
    for (uint32_t st = 2; st < stages; st += 2) {
      VK_LK_STAGE(false, st, f0, f1, stg_b, stg_a)
      VK_LK_STAGE(false, st + 1, f1, f0, stg_a, stg_b)
    }
    // ---- tile done.  Per output register r (query (r & 3) + 8 (r >> 2) + 4 kk of the tile, this lane's row): the 16 class
    // sums combined with _mm512_reduce_add_ps's pairing (l, l + 8) -> (l, l + 4) -> (l, l + 2) -> (0, 1), then 1 - dot or NaN
    float *__restrict__ out = a.dist + row;
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
      if (qi < tq && q0 + qi < a.qc && valid) out[(size_t)(q0 + qi) * a.ld] = cand ? 1.0f - dot : __builtin_nanf("");
      // keep the 16 gathers of one output register together: hoisting all 256 accumulator reads ahead of the adds would
      // need 256 more registers and spill into the pipelined loop (K4)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#undef VK_LK_STAGE
#undef VK_LK_ADVANCE
}

// the thread's entry u of the block's slice: index, or count and beyond = none
__device__ __forceinline__ size_t slice_index(uint32_t u) {
  return (size_t)blockIdx.x * kLargeKSlice + (size_t)u * kLargeKThreads + threadIdx.x;
}

__global__ __launch_bounds__(256) void flat_large_k_hist_kernel(FlatLargeKArgs a, int digit) {
  __shared__ uint32_t s_bin[kLargeKBins];
  const uint32_t q = blockIdx.y;
  const int lane = threadIdx.x & 63;
  for (uint32_t b = threadIdx.x; b < kLargeKBins; b += kLargeKThreads) s_bin[b] = 0;
  __syncthreads();
  const uint32_t shift = digit_shift(digit), mask = digit_bins(digit) - 1u;
  const uint32_t hi_shift = digit == 0 ? 32u : digit == 1 ? 21u : 10u;   // the bits above the digit: they must equal the prefix's
  const uint32_t prefix = digit == 0 ? 0u : a.state[(size_t)q * kLargeKStateWords];
  const float *__restrict__ dist = a.dist + (size_t)q * a.ld;
#pragma unroll 4
  for (uint32_t u = 0; u < kLargeKPerThread; ++u) {
    const size_t i = slice_index(u);
    bool in = false;
    uint32_t bin = 0;
    if (i < a.count) {
      const float d = dist[i];
      const uint32_t key = large_k_dev_key(d);
      in = d == d && (hi_shift == 32u || (key >> hi_shift) == (prefix >> hi_shift));
      bin = (key >> shift) & mask;
    }
    // the lanes that share the first counted lane's bin are added once (one query's distances crowd into a few top digits)
    const uint64_t live = __ballot(in);
    if (live != 0) {
      const int first = __ffsll((unsigned long long)live) - 1;
      const uint32_t fbin = (uint32_t)__builtin_amdgcn_readlane((int)bin, first);
      const uint64_t same = __ballot(in && bin == fbin);
      if (lane == first) atomicAdd(&s_bin[fbin], (uint32_t)__popcll(same));
      else if (in && bin != fbin) atomicAdd(&s_bin[bin], 1u);
    }
  }
  __syncthreads();
  uint32_t *__restrict__ h = a.hist + (size_t)q * kLargeKBins;
  for (uint32_t b = threadIdx.x; b <= mask; b += kLargeKThreads) {
    const uint32_t c = s_bin[b];
    if (c) atomicAdd(&h[b], c);
  }
}

// inclusive prefix over the wave's 64 lanes
__device__ __forceinline__ uint32_t large_k_wave_sum(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// one wave per query: lane l owns bins [l * per, (l + 1) * per)
__global__ __launch_bounds__(64) void flat_large_k_pick_kernel(FlatLargeKArgs a, int digit) {
  const uint32_t q = blockIdx.x;
  const int lane = threadIdx.x;
  uint32_t *__restrict__ h = a.hist + (size_t)q * kLargeKBins;
  uint32_t *__restrict__ st = a.state + (size_t)q * kLargeKStateWords;
  const uint32_t per = digit_bins(digit) / 64u;
  uint32_t sum = 0;
  for (uint32_t i = 0; i < per; ++i) sum += h[lane * per + i];
  const uint32_t inc = large_k_wave_sum(sum, lane);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  uint32_t prefix = 0, want = a.k, n_less = 0, n_real = total;
  if (digit != 0) {
    prefix = st[0];
    want = st[1];
    n_less = st[2];
    n_real = st[4];
  }
  if (want > total) want = total;   // (digit 0: fewer candidates than k -> the last of them; later digits: never)
  uint32_t bin = 0, below = 0, in_bin = 0;
  if (total != 0) {   // want >= 1
    const uint64_t reach = __ballot(inc >= want);
    const int owner = __ffsll((unsigned long long)reach) - 1;
    if (lane == owner) {
      uint32_t run = inc - sum;
      for (uint32_t i = 0; i < per; ++i) {
        const uint32_t c = h[lane * per + i];
        if (run + c >= want) { bin = lane * per + i; below = run; in_bin = c; break; }
        run += c;
      }
    }
    bin = (uint32_t)__shfl((int)bin, owner);
    below = (uint32_t)__shfl((int)below, owner);
    in_bin = (uint32_t)__shfl((int)in_bin, owner);
  }
  for (uint32_t i = 0; i < per; ++i) h[lane * per + i] = 0;   // the next digit's (the next chunk's) bins
  if (lane == 0) {
    const bool last = digit == kLargeKDigits - 1;
    n_less += below;
    st[0] = prefix | (bin << digit_shift(digit));
    st[1] = want - below;
    st[2] = n_less;
    st[3] = last ? in_bin : 0u;
    st[4] = n_real;
    st[5] = 0;
    st[6] = last && (uint64_t)n_less + in_bin > a.cap ? 1u : 0u;
    st[7] = 0;
  }
}

__global__ __launch_bounds__(256) void flat_large_k_emit_kernel(FlatLargeKArgs a) {
  const uint32_t q = blockIdx.y;
  const int lane = threadIdx.x & 63;
  uint32_t *__restrict__ st = a.state + (size_t)q * kLargeKStateWords;
  if (st[6] != 0) return;   // too many ties at the k-th key: the paged path answers this query
  const uint32_t T = st[0];
  const float *__restrict__ dist = a.dist + (size_t)q * a.ld;
  uint32_t bits[kLargeKPerThread];
  uint32_t sel = 0, mine = 0;
#pragma unroll
  for (uint32_t u = 0; u < kLargeKPerThread; ++u) {
    const size_t i = slice_index(u);
    bits[u] = 0;
    if (i < a.count) {
      const float d = dist[i];
      bits[u] = __float_as_uint(d);
      if (d == d && large_k_dev_key(d) <= T) { sel |= 1u << u; ++mine; }
    }
  }
  const uint32_t inc = large_k_wave_sum(mine, lane);
  const uint32_t wave_total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
  if (wave_total == 0) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&st[5], wave_total);
  uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)base) + inc - mine;
  uint32_t *__restrict__ ob = a.out_bits + (size_t)q * a.cap;
  uint64_t *__restrict__ ol = a.out_label + (size_t)q * a.cap;
#pragma unroll
  for (uint32_t u = 0; u < kLargeKPerThread; ++u) {
    if ((sel >> u) & 1u) {
      if (at < a.cap) {   // (always: the query is not flagged, so n_less + n_eq <= cap slots are taken in all)
        ob[at] = bits[u];
        ol[at] = a.labels[slice_index(u)];
      }
      ++at;
    }
  }
}

// ---- the device sort of the hand-back (option flat-large-k-device-sort) ---------------------------------------------------------
// A block's 4096 entries live in LDS as two arrays, distance bits (u32) and labels (u64); entry i sits in slot i + i / 16, so
// the 16 consecutive entries a thread takes into registers start 17 slots apart: a wave's loads of "my e-th entry" fall on
// 64 different words instead of on two banks.  4352 slots x 12 B = 51 KB per block, three blocks per CU.
constexpr uint32_t kSortSlots = kLargeKSlice + kLargeKSlice / kLargeKPerThread;
constexpr uint32_t kSortNoBits = 0x7FFFFFFFu;   // the sentinel's distance bits: key 0xFFFFFFFF, above +inf's 0xFF800000
constexpr uint32_t kSortTileLog2 = 12;
static_assert(kLargeKSortTile == kLargeKSlice && (1u << kSortTileLog2) == kLargeKSlice && kLargeKPerThread == 16,
              "the sort's tile is the slice, 16 entries per thread");

__device__ __forceinline__ uint32_t sort_slot(uint32_t i) { return i + (i >> 4); }
__device__ __forceinline__ bool sort_before(uint32_t ka, uint64_t la, uint32_t kb, uint64_t lb) { return ka < kb || (ka == kb && la < lb); }

// the entries a thread holds: key = large_k_dev_key(bits), kept next to the bits (-0 and +0 share a key, the bits differ)
struct SortRegs {
  uint32_t key[kLargeKPerThread], bits[kLargeKPerThread];
  uint64_t lab[kLargeKPerThread];
};
__device__ __forceinline__ void sort_cx(SortRegs &r, uint32_t i, uint32_t l) {   // i < l, constants once unrolled: the smaller one to i
  const bool sw = sort_before(r.key[l], r.lab[l], r.key[i], r.lab[i]);
  const uint32_t ki = r.key[i], bi = r.bits[i];
  const uint64_t li = r.lab[i];
  r.key[i] = sw ? r.key[l] : ki;
  r.bits[i] = sw ? r.bits[l] : bi;
  r.lab[i] = sw ? r.lab[l] : li;
  r.key[l] = sw ? ki : r.key[l];
  r.bits[l] = sw ? bi : r.bits[l];
  r.lab[l] = sw ? li : r.lab[l];
}
// the bitonic network in its all-ascending form: a run of `size` entries is made of two sorted halves by comparing entry i with
// its mirror image in the run (the flip), then by half-cleaners of strides size / 4 ... 1
template <uint32_t kStride>
__device__ __forceinline__ void sort_regs_clean(SortRegs &r) {   // the half-cleaners of strides kStride ... 1 over the 16 entries
  if constexpr (kStride != 0) {
#pragma unroll
    for (uint32_t e = 0; e < kLargeKPerThread; ++e)
      if ((e & kStride) == 0) sort_cx(r, e, e | kStride);
    sort_regs_clean<kStride / 2>(r);
  }
}
template <uint32_t kSize>
__device__ __forceinline__ void sort_regs_all(SortRegs &r) {   // sorts the 16 entries: runs of 2, 4, 8, 16
  if constexpr (kSize <= kLargeKPerThread) {
#pragma unroll
    for (uint32_t e = 0; e < kLargeKPerThread; ++e)
      if ((e ^ (kSize - 1)) > e) sort_cx(r, e, e ^ (kSize - 1));
    sort_regs_clean<kSize / 4>(r);
    sort_regs_all<kSize * 2>(r);
  }
}
// one compare-exchange between two slots of LDS, i < l: the labels are looked at only when the keys do not settle it
__device__ __forceinline__ void sort_lds_cx(uint32_t *s_bits, uint64_t *s_lab, uint32_t i, uint32_t l) {
  const uint32_t si = sort_slot(i), sl = sort_slot(l);
  const uint32_t bi = s_bits[si], bl = s_bits[sl];
  const uint32_t ki = large_k_dev_key(__uint_as_float(bi)), kl = large_k_dev_key(__uint_as_float(bl));
  if (kl <= ki) {
    const uint64_t li = s_lab[si], ll = s_lab[sl];
    if (kl < ki || ll < li) {
      s_bits[si] = bl;
      s_bits[sl] = bi;
      s_lab[si] = ll;
      s_lab[sl] = li;
    }
  }
}
__device__ __forceinline__ void sort_regs_from_lds(SortRegs &r, const uint32_t *s_bits, const uint64_t *s_lab) {
  const uint32_t base = threadIdx.x * (kLargeKPerThread + 1);   // sort_slot(threadIdx.x * 16)
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    r.bits[e] = s_bits[base + e];
    r.key[e] = large_k_dev_key(__uint_as_float(r.bits[e]));
    r.lab[e] = s_lab[base + e];
  }
}
__device__ __forceinline__ void sort_regs_to_lds(const SortRegs &r, uint32_t *s_bits, uint64_t *s_lab) {
  const uint32_t base = threadIdx.x * (kLargeKPerThread + 1);
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    s_bits[base + e] = r.bits[e];
    s_lab[base + e] = r.lab[e];
  }
}
// a query's entries as the sort sees them: 0 for a flagged query, never beyond cap
__device__ __forceinline__ uint32_t sort_entries(const uint32_t *__restrict__ st, uint32_t cap) {
  if (st[6] != 0) return 0;
  const uint64_t n = (uint64_t)st[2] + st[3];
  return n < cap ? (uint32_t)n : cap;
}

// Tile sort: grid (tiles of 4096 over cap) x (queries).  The block takes entries [tile * 4096, ...) of its query, coalesced
// (which thread starts with which entry does not matter to a sort), sentinels behind n; every thread sorts its 16 in
// registers; the runs of 32 ... 4096 are then made by the flip and the half-cleaners of strides >= 16 on LDS -- eight
// compare-exchanges per thread and step, a barrier behind each -- and the strides 8 ... 1 in registers again.  The sentinels end
// up behind the entries, so the first n - tile * 4096 slots go back where they came from, coalesced; or, with `dense` (cap is
// within one tile: this is the last launch), the first min(k, n) into the dense hand-back.
__global__ __launch_bounds__(256) void flat_large_k_tile_sort_kernel(FlatLargeKSortArgs a, int dense) {
  __shared__ uint32_t s_bits[kSortSlots];
  __shared__ uint64_t s_lab[kSortSlots];
  const uint32_t q = blockIdx.y;
  const uint32_t n = sort_entries(a.state + (size_t)q * kLargeKStateWords, a.cap);
  const uint64_t tile0 = (uint64_t)blockIdx.x * kLargeKSlice;
  if (tile0 >= n) return;   // (a flagged query, a tile behind the entries)
  const uint32_t m = n - (uint32_t)tile0 < kLargeKSlice ? n - (uint32_t)tile0 : kLargeKSlice;   // entries of this tile
  uint32_t *__restrict__ gb = a.bits + (size_t)q * a.cap + tile0;
  uint64_t *__restrict__ gl = a.label + (size_t)q * a.cap + tile0;
  SortRegs r;
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const uint32_t i = e * kLargeKThreads + threadIdx.x;
    r.bits[e] = i < m ? gb[i] : kSortNoBits;
    r.lab[e] = i < m ? gl[i] : kNoLabel;
    r.key[e] = large_k_dev_key(__uint_as_float(r.bits[e]));
  }
  sort_regs_all<2>(r);
  sort_regs_to_lds(r, s_bits, s_lab);
  __syncthreads();
  for (uint32_t size = 2 * kLargeKPerThread; size <= kLargeKSlice; size <<= 1) {
    const uint32_t half = size >> 1;
#pragma unroll 2
    for (uint32_t u = 0; u < kLargeKPerThread / 2; ++u) {   // the flip: entry r of a run's lower half against entry size - 1 - r of the run
      const uint32_t p = u * kLargeKThreads + threadIdx.x, in = p & (half - 1), run0 = (p - in) << 1;
      sort_lds_cx(s_bits, s_lab, run0 + in, run0 + size - 1 - in);
    }
    __syncthreads();
    for (uint32_t stride = size >> 2; stride >= kLargeKPerThread; stride >>= 1) {
#pragma unroll 2
      for (uint32_t u = 0; u < kLargeKPerThread / 2; ++u) {
        const uint32_t p = u * kLargeKThreads + threadIdx.x, in = p & (stride - 1), i = ((p - in) << 1) | in;
        sort_lds_cx(s_bits, s_lab, i, i + stride);
      }
      __syncthreads();
    }
    sort_regs_from_lds(r, s_bits, s_lab);
    sort_regs_clean<kLargeKPerThread / 2>(r);
    sort_regs_to_lds(r, s_bits, s_lab);
    __syncthreads();
  }
  const uint32_t lim = dense ? (a.k < m ? a.k : m) : m;
  uint32_t *__restrict__ ob = dense ? a.dense_bits + (size_t)q * a.k : gb;
  uint64_t *__restrict__ ol = dense ? a.dense_label + (size_t)q * a.k : gl;
#pragma unroll 4
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const uint32_t i = e * kLargeKThreads + threadIdx.x;
    if (i < lim) {
      ob[i] = s_bits[sort_slot(i)];
      ol[i] = s_lab[sort_slot(i)];
    }
  }
}

// Merge path: of the first o entries of the merge of two sorted runs A (la entries) and B (lb), how many come from A -- an
// entry of A going before an entry of B unless B's is smaller.  at_a / at_b give (key, label) of an entry.  At most 32 steps.
template <class FA, class FB>
__device__ __forceinline__ uint32_t sort_co_rank(uint32_t o, uint32_t la, uint32_t lb, FA at_a, FB at_b) {
  uint32_t lo = o > lb ? o - lb : 0, hi = o < la ? o : la;
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const uint32_t mid = lo + ((hi - lo) >> 1);   // lo <= mid < hi <= la, and 0 <= o - mid - 1 < lb
    uint32_t ka, kb;
    uint64_t xa, xb;
    at_a(mid, ka, xa);
    at_b(o - mid - 1, kb, xb);
    if (sort_before(kb, xb, ka, xa)) hi = mid;   // B's entry is taken before A[mid]: A gives at most mid
    else lo = mid + 1;
  }
  return lo;
}

// Merge pass: grid as the tile sort's.  The sorted runs of run = 4096 << pass entries of src are merged in neighbouring pairs
// into dst; block b owns outputs [b * 4096, (b + 1) * 4096) of its query.  Two threads find the ends of that range in the
// pair's two runs by the merge path over HBM, the block brings the at most 4096 inputs into LDS (A's part in front, B's behind
// it), every thread finds its own 16 outputs' start the same way in LDS and merges them serially into registers; they go
// through LDS once more to leave coalesced.  A run without a partner is the same with an empty B: a copy.  With `last` (one
// pair spans cap) the outputs below min(k, n) go to the dense hand-back and the blocks behind them leave.
__global__ __launch_bounds__(256) void flat_large_k_merge_kernel(FlatLargeKSortArgs a, const uint32_t *__restrict__ src_bits,
                                                                 const uint64_t *__restrict__ src_lab, uint32_t *__restrict__ dst_bits,
                                                                 uint64_t *__restrict__ dst_lab, uint32_t run_log2, int last) {
  __shared__ uint32_t s_bits[kSortSlots];
  __shared__ uint64_t s_lab[kSortSlots];
  __shared__ uint32_t s_cut[2];
  const uint32_t q = blockIdx.y;
  const uint32_t n = sort_entries(a.state + (size_t)q * kLargeKStateWords, a.cap);
  const uint32_t lim = last && a.k < n ? a.k : n;   // outputs anybody wants
  const uint64_t out0 = (uint64_t)blockIdx.x * kLargeKSlice;
  if (out0 >= lim) return;
  const uint64_t pair0 = (out0 >> (run_log2 + 1)) << (run_log2 + 1);   // where this block's pair of runs starts
  const uint64_t run = (uint64_t)1 << run_log2;
  const uint32_t la = (uint32_t)(pair0 + run < n ? run : n - pair0);
  const uint32_t lb = (uint32_t)(pair0 + run >= n ? 0 : (pair0 + 2 * run < n ? run : n - pair0 - run));
  const uint32_t o0 = (uint32_t)(out0 - pair0);
  const uint32_t o1 = (uint64_t)o0 + kLargeKSlice < (uint64_t)la + lb ? o0 + kLargeKSlice : la + lb;   // o0 < la + lb: out0 < n
  const uint32_t *__restrict__ ab = src_bits + (size_t)q * a.cap + pair0;
  const uint64_t *__restrict__ al = src_lab + (size_t)q * a.cap + pair0;
  auto g_a = [&](uint32_t i, uint32_t &key, uint64_t &lab) { key = large_k_dev_key(__uint_as_float(ab[i])); lab = al[i]; };
  auto g_b = [&](uint32_t i, uint32_t &key, uint64_t &lab) { key = large_k_dev_key(__uint_as_float(ab[la + i])); lab = al[la + i]; };
  if (threadIdx.x == 0) s_cut[0] = sort_co_rank(o0, la, lb, g_a, g_b);
  if (threadIdx.x == 64) s_cut[1] = sort_co_rank(o1, la, lb, g_a, g_b);
  __syncthreads();
  // (the cuts of sorted runs are in order and tot apart at most; the clamps keep every index in range whatever the runs hold)
  const uint32_t a0 = s_cut[0], b0 = o0 - a0, tot = o1 - o0;
  const uint32_t na = s_cut[1] < a0 ? 0 : (s_cut[1] - a0 < tot ? s_cut[1] - a0 : tot), nb = tot - na;
#pragma unroll 4
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const uint32_t i = e * kLargeKThreads + threadIdx.x;
    if (i < tot) {
      uint32_t g = i < na ? a0 + i : la + b0 + (i - na);
      g = g < la + lb ? g : la + lb - 1;
      s_bits[sort_slot(i)] = ab[g];
      s_lab[sort_slot(i)] = al[g];
    }
  }
  __syncthreads();
  auto at = [&](uint32_t i, uint32_t &key, uint64_t &lab) { key = large_k_dev_key(__uint_as_float(s_bits[sort_slot(i)])); lab = s_lab[sort_slot(i)]; };
  auto s_a = [&](uint32_t i, uint32_t &key, uint64_t &lab) { at(i, key, lab); };
  auto s_b = [&](uint32_t i, uint32_t &key, uint64_t &lab) { at(na + i, key, lab); };
  const uint32_t mine0 = threadIdx.x * kLargeKPerThread < tot ? threadIdx.x * kLargeKPerThread : tot;
  const uint32_t mine = tot - mine0 < kLargeKPerThread ? tot - mine0 : kLargeKPerThread;
  uint32_t ia = sort_co_rank(mine0, na, nb, s_a, s_b), ib = mine0 - ia;
  // the two heads; a side that has run out shows the sentinel, which no entry reaches
  uint32_t ka = 0xFFFFFFFFu, kb = 0xFFFFFFFFu, ba = kSortNoBits, bb = kSortNoBits;
  uint64_t xa = kNoLabel, xb = kNoLabel;
  if (ia < na) { ba = s_bits[sort_slot(ia)]; at(ia, ka, xa); }
  if (ib < nb) { bb = s_bits[sort_slot(na + ib)]; at(na + ib, kb, xb); }
  uint32_t out_bits[kLargeKPerThread];
  uint64_t out_lab[kLargeKPerThread];
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const bool from_b = sort_before(kb, xb, ka, xa);
    out_bits[e] = from_b ? bb : ba;
    out_lab[e] = from_b ? xb : xa;
    if (from_b) {
      ++ib;
      kb = 0xFFFFFFFFu, bb = kSortNoBits, xb = kNoLabel;
      if (ib < nb) { bb = s_bits[sort_slot(na + ib)]; at(na + ib, kb, xb); }
    } else {
      ++ia;
      ka = 0xFFFFFFFFu, ba = kSortNoBits, xa = kNoLabel;
      if (ia < na) { ba = s_bits[sort_slot(ia)]; at(ia, ka, xa); }
    }
  }
  __syncthreads();   // every thread has read its inputs: the slots take the outputs
  const uint32_t base = threadIdx.x * (kLargeKPerThread + 1);
#pragma unroll
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    if (e < mine) {
      s_bits[base + e] = out_bits[e];
      s_lab[base + e] = out_lab[e];
    }
  }
  __syncthreads();
  uint32_t *__restrict__ ob = last ? a.dense_bits + (size_t)q * a.k : dst_bits + (size_t)q * a.cap;
  uint64_t *__restrict__ ol = last ? a.dense_label + (size_t)q * a.k : dst_lab + (size_t)q * a.cap;
#pragma unroll 4
  for (uint32_t e = 0; e < kLargeKPerThread; ++e) {
    const uint32_t i = e * kLargeKThreads + threadIdx.x;
    const uint64_t g = out0 + i;
    if (i < tot && g < lim) {
      ob[g] = s_bits[sort_slot(i)];
      ol[g] = s_lab[sort_slot(i)];
    }
  }
}

bool large_k_args_ok(const FlatLargeKArgs &a) {
  return a.count != 0 && a.qc != 0 && a.qc <= kLargeKMaxChunkQueries && a.k != 0 && a.ld >= a.count && a.dist && a.state;
}

}  // namespace

uint32_t flat_large_k_slice() { return kLargeKSlice; }
uint32_t flat_large_k_dist_blocks() { return kLargeKDistBlocks; }

hipError_t launch_flat_large_k_distance(const FlatLargeKArgs &a, bool l2, bool bf16, int qb, hipStream_t s) {
  if (!large_k_args_ok(a) || !a.rows || !a.labels || !a.queries || a.chunks == 0 || a.chunks * 16 != a.row_stride_f || a.q_stride_f < a.row_stride_f ||
      (qb != 1 && qb != 2 && qb != 4 && qb != 8))
    return hipErrorInvalidValue;
  const size_t lds = (size_t)qb * a.chunks * 64;
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  const void *f = l2 ? (bf16 ? reinterpret_cast<const void *>(&flat_dense_distance_kernel<true, true>)
                             : reinterpret_cast<const void *>(&flat_dense_distance_kernel<true, false>))
                     : (bf16 ? reinterpret_cast<const void *>(&flat_dense_distance_kernel<false, true>)
                             : reinterpret_cast<const void *>(&flat_dense_distance_kernel<false, false>));
  if (lds > 48 * 1024) {
    hipError_t e = ensure_max_lds(f);
    if (e != hipSuccess) return e;
  }
  const uint32_t tiles = (a.count + kRowsPerWave - 1) / kRowsPerWave;
  const uint32_t nqg = (a.qc + (uint32_t)qb - 1) / (uint32_t)qb;
  uint32_t blocks = (tiles + 3) / 4;
  if (blocks > kLargeKDistBlocks) blocks = kLargeKDistBlocks;
  FlatLargeKArgs args = a;
  uint32_t qb_arg = (uint32_t)qb;
  void *params[] = {&args, &qb_arg};
  return hipLaunchKernel(f, dim3(blocks, nqg), dim3(256), params, lds, s);
}

// the matrix-core launch's grid: every CU one block while there are that many row tiles, and with qc <= tq every row leaves HBM
// once (K8m's rule)
static void dense_mfma_grid(uint32_t count, uint32_t stride_f, uint32_t qc, uint32_t *nrp, uint32_t *nqt, uint32_t *tq) {
  *tq = prefilter_mfma_tile_q(stride_f);
  *nqt = (qc + *tq - 1) / *tq;
  const uint32_t n_tiles = (uint32_t)(((uint64_t)count + kMfmaTile - 1) / kMfmaTile);
  int dev = 0, cus = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  *nrp = std::max<uint32_t>(8, ((uint32_t)(cus > 0 ? cus : 256) / *nqt) & ~7u);
  *nrp = std::min<uint32_t>(*nrp, (n_tiles + 7) & ~7u);
}

uint32_t flat_large_k_mfma_row_partitions(uint32_t count, uint32_t stride_f, uint32_t qc) {
  if (count == 0 || !large_k_takes_mfma(true, false, stride_f, qc)) return 0;
  uint32_t nrp, nqt, tq;
  dense_mfma_grid(count, stride_f, qc, &nrp, &nqt, &tq);
  return nrp;
}

hipError_t launch_flat_large_k_distance_mfma(const FlatLargeKArgs &a, bool bf16, hipStream_t s) {
  if (!large_k_args_ok(a) || !a.rows || !a.labels || !a.queries || a.chunks == 0 || a.chunks * 16 != a.row_stride_f || a.q_stride_f < a.row_stride_f ||
      !large_k_takes_mfma(true, false, a.row_stride_f, a.qc))
    return hipErrorInvalidValue;
  uint32_t nrp, nqt, tq;
  dense_mfma_grid(a.count, a.row_stride_f, a.qc, &nrp, &nqt, &tq);
  const size_t lds = (size_t)tq * (a.row_stride_f + 4) * 4 + kPrefilterMfmaRingBytes;
  const void *f = bf16 ? reinterpret_cast<const void *>(&flat_dense_mfma_kernel<true>) : reinterpret_cast<const void *>(&flat_dense_mfma_kernel<false>);
  hipError_t e = ensure_max_lds(f);
  if (e != hipSuccess) return e;
  e = ensure_scratch(f, s);   // (no scratch as built; a build that spills is refused where the device cannot hold it)
  if (e != hipSuccess) return e;
  FlatLargeKArgs args = a;
  void *params[] = {&args, &nrp, &nqt, &tq};
  return hipLaunchKernel(f, dim3(nrp * nqt), dim3(256), params, lds, s);
}

hipError_t launch_flat_large_k_select(const FlatLargeKArgs &a, hipStream_t s) {
  if (!large_k_args_ok(a) || !a.hist) return hipErrorInvalidValue;
  const uint32_t slices = (uint32_t)(((uint64_t)a.count + kLargeKSlice - 1) / kLargeKSlice);
  for (int d = 0; d < kLargeKDigits; ++d) {
    hipLaunchKernelGGL(flat_large_k_hist_kernel, dim3(slices, a.qc), dim3(kLargeKThreads), 0, s, a, d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(flat_large_k_pick_kernel, dim3(a.qc), dim3(64), 0, s, a, d);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t launch_flat_large_k_emit(const FlatLargeKArgs &a, hipStream_t s) {
  if (!large_k_args_ok(a) || !a.labels || !a.out_bits || !a.out_label || a.cap == 0) return hipErrorInvalidValue;
  const uint32_t slices = (uint32_t)(((uint64_t)a.count + kLargeKSlice - 1) / kLargeKSlice);
  hipLaunchKernelGGL(flat_large_k_emit_kernel, dim3(slices, a.qc), dim3(kLargeKThreads), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_flat_large_k_sort(const FlatLargeKSortArgs &a, hipStream_t s) {
  if (!a.state || !a.bits || !a.label || !a.dense_bits || !a.dense_label || a.cap == 0 || a.k == 0 || a.qc == 0 || a.qc > kLargeKMaxChunkQueries)
    return hipErrorInvalidValue;
  const uint32_t passes = large_k_sort_passes(a.cap);
  if (passes != 0 && (!a.bits2 || !a.label2)) return hipErrorInvalidValue;
  const uint32_t tiles = (uint32_t)(((uint64_t)a.cap + kLargeKSlice - 1) / kLargeKSlice);
  hipLaunchKernelGGL(flat_large_k_tile_sort_kernel, dim3(tiles, a.qc), dim3(kLargeKThreads), 0, s, a, passes == 0 ? 1 : 0);
  hipError_t e = hipGetLastError();
  for (uint32_t p = 0; p < passes && e == hipSuccess; ++p) {
    const bool odd = (p & 1u) != 0, last = p + 1 == passes;
    // the last pass writes the dense hand-back only: no block beyond min(k, cap) outputs has anything to do
    const uint32_t blocks = last && a.k < a.cap ? (uint32_t)(((uint64_t)a.k + kLargeKSlice - 1) / kLargeKSlice) : tiles;
    hipLaunchKernelGGL(flat_large_k_merge_kernel, dim3(blocks, a.qc), dim3(kLargeKThreads), 0, s, a, odd ? a.bits2 : a.bits,
                       odd ? a.label2 : a.label, odd ? a.bits : a.bits2, odd ? a.label : a.label2, kSortTileLog2 + p, last ? 1 : 0);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace vk
