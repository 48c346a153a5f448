// flat_l2_gemm.hip -- K4e: exact batched FLAT search under L2 (squared Euclidean distance) whose dense work is ONE plain f32
// GEMM on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32).  Option flat-l2-gemm; answers carry the bits of K3 and the oracle.
//
// Why a bound and not the answer.  The reference distance is SimSIMD's 16-chain f32 sum of (x_i - q_i)^2: not a product of the
// inputs, so no MFMA reproduces its bits (K4's header).  But  d = |x|^2 + |q|^2 - 2 x.q  in real numbers, and a value `a`
// computed that way in f32 is within a known distance E of d.  A pair whose  a - E  already exceeds the query's pruning bound
// cannot enter the top-k; every other pair gets the exact SimSIMD-order distance from quad_row_distance<true> -- K3's own
// routine -- and only those values ever reach a list.  The GEMM needs no lane-class separation, so one accumulator tile per
// 32 x 32 sub-tile does what K4 spends sixteen on.
//
// The error term E, every piece named.  u = 2^-24, gamma(n) = n u / (1 - n u), Dp = the padded dimension (row stride), all
// sums over Dp terms (the padding is zeros and adds nothing).
//   (1) nx = fl(|x|^2), nq = fl(|q|^2): fma chains and a reduction tree in some order; a term passes through at most Dp
//       roundings and all terms are >= 0, so  nx = |x|^2 (1 + t), |t| <= gamma(Dp), likewise nq.
//   (2) p = fl(x.q) from the matrix cores: K steps of fused multiply-adds in some order, at most Dp roundings per term:
//       |p - x.q| <= gamma(Dp) sum |x_i q_i| <= gamma(Dp) |x| |q|.
//   (3) s = fl(nx + nq), a = fl(s - 2 p) (2 p is exact): two more roundings.  With gamma(k)(1 + u) + u <= gamma(k + 2):
//       |a - d| <= gamma(Dp + 3) (|x|^2 + |q|^2 + 2 |x| |q|) <= gamma(Dp + 3) * 2 (|x|^2 + |q|^2)
//               <= 2 gamma(Dp + 3) / (1 - gamma(Dp)) * (nx + nq)                      [by (1); no square root needed]
//   (4) the reference value r: t_i = fl(x_i - q_i) = (x_i - q_i)(1 + e), then 16 fma chains of Dp / 16 steps and a tree of 4
//       adds.  Every term is >= 0 and passes through at most 2 + Dp / 16 + 4 factors (1 - u), so  r >= d (1 - gamma(m)),
//       m = Dp / 16 + 6: the reference may lie BELOW d, by a relative amount.
//   (5) together, for a - gamma(..) >= 0:  r >= (a - (3)) (1 - gamma(m)) >= a - (3) - gamma(m) |a|;  otherwise r >= 0 > that.
//   (6) the gate computes fl(a - E) and that rounding may add u |a|: E carries 2 u |a| more (one for the rounding, one so
//       that the margin is strict).
//   (7) products or squares below the normal range may be flushed or lose bits in (1), (2) and (4): at most Dp 2^-123 in all.
//   E = cS (nx + nq) + cA |a| + cAbs,  cS = 2 gamma(Dp + 3) / (1 - gamma(Dp)),  cA = gamma(Dp / 16 + 6) + 2 u,  cAbs = Dp 2^-123,
//   the three constants computed by the host in double, inflated by (1 + 2^-20) for the three roundings of E's own evaluation
//   and of s, and rounded UP to f32.  Nothing here is tuned by experiment.
// A pair is pruned iff  fl(a - E) > bound_q, where bound_q is an exact k-th best distance of k entries some list holds (or
// the pre-pass bound): then r > bound_q strictly and the pair is beyond k others, ties included.  Written as !(a - E > bound) the
// test lets a NaN through: a NaN or inf in a row or query (a, E or both non-finite) reaches the exact path and gets K3's answer.
//
// Tiling (256-thread blocks, one resident per CU, 4 waves = one per SIMD):
//   block tile   = 256 rows x tile_q queries; wave w owns rows [64w, 64w + 64) x all tile_q queries: 2 x (tile_q / 32)
//                  accumulator tiles (64 registers at tile_q = 64) that share every Q fragment read from LDS
//   Q tile       : resident in LDS as f32 for the block's life, [tile_q][Dp + 4] (16-byte rows, conflict-free pad as K4);
//                  tile_q = 64 where that fits in 160 KB next to the rest, else 32 / 24 / 16 (flat_l2_gemm_host.hpp)
//   X rows       : each wave streams ITS 64 rows HBM -> registers -> its private LDS buffer -> MFMA operands in pairs of
//                  chunks (32 floats, 128 B per row and load); bf16 rows are widened on the way in (exact).  No block
//                  barrier in the main loop.
//   |q|^2        : once per block from the LDS tile;  |x|^2: by the wave from its staged registers (one fma per element,
//                  VALU, under the MFMAs), reduced at the tile's end.  No row statistics, no image.
//   per tile     : gate all pairs, survivors -> the wave's LDS queue of (row, query) by ballot and prefix count; the queue is
//                  drained 16 pairs at a time, one per quad, the rows read again from HBM (L2-resident: just streamed), the
//                  query from the LDS tile; results go to the list of (block, wave, query) in HBM scratch, owned by lane
//                  `query` of the wave, with K4's rules (topk_insert, flat_topk_list.hpp); a list that fills lowers the
//                  shared bound qbound[q], which every wave re-reads once per tile
// Grid: nrp x nqt blocks, XCD-aware decode as K4 (the sharers of a row panel on one XCD).  The host picks nrp so that the grid
// is about one block per CU -- persistent -- while nqt <= 32 (2048 queries at tile_q = 64, 512 at 16); beyond that nrp stays at
// its floor of 8 and the grid grows with nqt without a cap: blocks then queue for the CUs, each loads its Q tile once more,
// and the scratch lists (nq * nrp * 4 * k entries) grow with it.  Nothing waits on another block, so any grid is correct.
// Where this departs from the intended design, and why:
//   * one staged pair per wave instead of a ring: the operand fragments are double-buffered in REGISTERS (the 192 registers K4
//     spends on class accumulators are free), so the buffer can be overwritten as soon as its reads are issued -- 36 KB of LDS
//     instead of 55, which is what lets 32 queries of 768 floats and 16 of 1856 stay resident
//   * the placement of a stage's memory operations between its 32 .. 64 MFMAs is left to the compiler: a stage is 4096 matrix
//     cycles against 24 LDS and 8 global instructions, there is nothing to pin
//   * no lockstep window among the sharers of a row panel: not measured here, left out rather than guessed
//   * row loads are clamped to the last row instead of relying on the row store's slack
// Roofline: MFMA-bound, 2 * rows * Dp * B FLOPs against the f32 matrix peak, plus the exact evaluations of the survivors.
#include <math.h>

#include "device_common.hpp"
#include "flat_l2_gemm_host.hpp"
#include "flat_topk_list.hpp"
#include "kernels.hpp"

namespace vk {

struct L2GemmParams {
  FlatL2GemmArgs a;
  float c_s, c_a, c_abs;   // the constants of E (header)
};

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr uint32_t kPairWords = 64 * kL2GemmXStride;   // one staged pair of chunks of one wave's 64 rows

// register-resident sets are plain structs handled BY VALUE (K4's note)
struct L2Stg { float4 v[8]; };                       // one pair of one wave: f32 rows 8 pieces per lane, bf16 rows 4
template <int kNQS> struct L2Frag { float4 x[2][4], q[kNQS][4]; };

// position in this wave's flattened (tile, pair) stream; never moves past the last pair (the loads issued behind the end
// re-read it and are unused)
struct L2Pos {
  uint32_t row0;   // first of the wave's 64 rows in the tile
  uint32_t pr;     // pair inside the tile
  uint32_t left;   // pairs still to come, this one included
};
__device__ __forceinline__ void l2_advance(L2Pos &p, uint32_t pairs) {
  const bool go = p.left > 1;
  const bool wrap = go && p.pr + 1 == pairs;
  p.left -= p.left != 0 ? 1u : 0u;
  p.pr = wrap ? 0u : p.pr + (go ? 1u : 0u);
  p.row0 += wrap ? kL2GemmRows : 0u;
}

// HBM -> registers.  f32: 64 rows x 8 pieces of 16 B, piece lane % 8 of rows lane / 8 + 8 u; bf16: 64 rows x 4 pieces of 16 B
// (8 elements), piece lane % 4 of rows lane / 4 + 16 u.  Rows at or past n_rows read the last row (their pairs are masked).
template <bool kBf16>
__device__ __forceinline__ L2Stg l2_load(const FlatL2GemmArgs &a, uint32_t lane, const L2Pos p) {
  L2Stg s;
  const uint32_t last = a.n_rows - 1;
  if constexpr (kBf16) {
    const uint16_t *base = static_cast<const uint16_t *>(a.rows) + p.pr * 32 + (lane & 3) * 8;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t r = p.row0 + (lane >> 2) + 16 * u;
      s.v[u] = *reinterpret_cast<const float4 *>(base + (size_t)(r < last ? r : last) * a.row_stride_f);
    }
#pragma unroll
    for (int u = 4; u < 8; ++u) s.v[u] = s.v[0];
  } else {
    const float *base = static_cast<const float *>(a.rows) + p.pr * 32 + (lane & 7) * 4;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t r = p.row0 + (lane >> 3) + 8 * u;
      s.v[u] = *reinterpret_cast<const float4 *>(base + (size_t)(r < last ? r : last) * a.row_stride_f);
    }
  }
  return s;
}

__device__ __forceinline__ float sq4(const float4 v, float acc) {
  return fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, acc))));
}
__device__ __forceinline__ void l2_widen8(const float4 raw, float4 &lo, float4 &hi) {   // eight bf16 -> two float4, exact
  const uint32_t w0 = __float_as_uint(raw.x), w1 = __float_as_uint(raw.y), w2 = __float_as_uint(raw.z), w3 = __float_as_uint(raw.w);
  lo = float4{__uint_as_float(w0 << 16), __uint_as_float(w0 & 0xffff0000u), __uint_as_float(w1 << 16), __uint_as_float(w1 & 0xffff0000u)};
  hi = float4{__uint_as_float(w2 << 16), __uint_as_float(w2 & 0xffff0000u), __uint_as_float(w3 << 16), __uint_as_float(w3 & 0xffff0000u)};
}

// registers -> the wave's LDS buffer, and this lane's share of the rows' squared norms (np[u]: the row of load u)
template <bool kBf16>
__device__ __forceinline__ void l2_store(float *buf, uint32_t lane, const L2Stg s, float (&np)[8]) {
  if constexpr (kBf16) {
    float *p = buf + (lane >> 2) * kL2GemmXStride + (lane & 3) * 8;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float4 lo, hi;
      l2_widen8(s.v[u], lo, hi);
      *reinterpret_cast<float4 *>(p + 16 * u * kL2GemmXStride) = lo;
      *reinterpret_cast<float4 *>(p + 16 * u * kL2GemmXStride + 4) = hi;
      np[u] = sq4(hi, sq4(lo, np[u]));
    }
  } else {
    float *p = buf + (lane >> 3) * kL2GemmXStride + (lane & 7) * 4;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      *reinterpret_cast<float4 *>(p + 8 * u * kL2GemmXStride) = s.v[u];
      np[u] = sq4(s.v[u], np[u]);
    }
  }
}

// the tile's 64 row norms -> wn[row in the wave's tile]; the partial sums start over
template <bool kBf16>
__device__ __forceinline__ void l2_norms_out(float *wn, uint32_t lane, float (&np)[8]) {
#pragma unroll
  for (int u = 0; u < (kBf16 ? 4 : 8); ++u) {
    float s = np[u];
    s += dpp_quad_xor1(s);
    s += dpp_quad_xor2(s);
    if constexpr (!kBf16) s += __shfl_xor(s, 4);
    if constexpr (kBf16) {
      if ((lane & 3) == 0) wn[(lane >> 2) + 16 * u] = s;
    } else {
      if ((lane & 7) == 0) wn[(lane >> 3) + 8 * u] = s;
    }
    np[u] = 0.f;
  }
}

// LDS -> registers: this lane's row (A) and query (B) operands of one pair; lane = (row or query lane & 31, chunk lane >> 5).
// xb = the wave's buffer + (lane & 31) * 36 + (lane >> 5) * 16;  qp = the lane's query row(s) + (lane >> 5) * 16
template <int kNQS>
__device__ __forceinline__ L2Frag<kNQS> l2_frag(const float *xb, const float *qp0, const float *qp1, uint32_t pr) {
  L2Frag<kNQS> f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    f.x[0][c] = *reinterpret_cast<const float4 *>(xb + c * 4);
    f.x[1][c] = *reinterpret_cast<const float4 *>(xb + 32 * kL2GemmXStride + c * 4);
    f.q[0][c] = *reinterpret_cast<const float4 *>(qp0 + pr * 32 + c * 4);
    if constexpr (kNQS == 2) f.q[1][c] = *reinterpret_cast<const float4 *>(qp1 + pr * 32 + c * 4);
  }
  return f;
}

// the 16 K-steps of one pair for every accumulator tile; dependent MFMAs are 2 or 4 instructions apart
template <int kNQS>
__device__ __forceinline__ void l2_mul(f32x16 (&acc)[2][kNQS], const L2Frag<kNQS> f) {
#define VK_L2_STEP(C, M)                                                                                           \
  _Pragma("unroll") for (int rt = 0; rt < 2; ++rt) _Pragma("unroll") for (int qs = 0; qs < kNQS; ++qs)             \
      acc[rt][qs] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.x[rt][C].M, f.q[qs][C].M, acc[rt][qs], 0, 0, 0);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    VK_L2_STEP(c, x)
    VK_L2_STEP(c, y)
    VK_L2_STEP(c, z)
    VK_L2_STEP(c, w)
  }
#undef VK_L2_STEP
}

// n <= 16 queued pairs [first, first + n): one pair per quad gets K3's distance, then the inserts are applied one after
// another, each by the lane that owns the query's list (two quads may hit the same list)
template <bool kBf16>
__device__ __forceinline__ LaneTop l2_drain(const FlatL2GemmArgs &a, const uint32_t *que_row, const uint32_t *que_q, uint32_t first,
                                         uint32_t n, const float *lds_q, uint32_t qstride, uint32_t lane, float *list_d,
                                         uint64_t *list_l, uint32_t *qbound_tile, LaneTop top) {
  const uint32_t g = lane >> 2;
  const uint32_t e = first + (g < n ? g : n - 1);   // quads past n repeat the last pair (unused)
  const uint32_t row = que_row[e], q = que_q[e];
  const float d = quad_row_distance<true, kBf16>(row_base<kBf16>(a.rows, row, a.row_stride_f),
                                                 reinterpret_cast<const float4 *>(lds_q + (size_t)q * qstride), a.chunks, (int)(lane & 3));
  for (uint32_t i = 0; i < n; ++i) {
    const float di = readlane_f32(d, (int)(4 * i));
    const uint32_t ri = (uint32_t)__builtin_amdgcn_readlane((int)row, (int)(4 * i));
    const uint32_t qi = (uint32_t)__builtin_amdgcn_readlane((int)q, (int)(4 * i));
    // distance gate first, filter second (topk_insert) -- K3's order; a NaN distance enters no list, as in K3
    if (lane == qi && di <= top.thr_d)
      top = topk_insert(a.labels, a.allow_bits, a.allow_nbits, a.k, di, ri, list_d, list_l, qbound_tile + qi, top);
  }
  return top;
}

}  // namespace

template <bool kBf16, int kNQS>
__global__ __launch_bounds__(256, 1) void flat_l2_gemm_kernel(L2GemmParams prm) {
  extern __shared__ float lds[];
  const FlatL2GemmArgs &a = prm.a;
  if (launch_skipped(a.run_flag, a.run_if, a.run_hi)) return;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t li = lane & 31, kk = lane >> 5;
  const uint32_t pairs = a.row_stride_f / 32;          // even: the stride is a multiple of 64 floats
  const uint32_t qstride = a.row_stride_f + 4;
  const uint32_t tq = a.tile_q;

  float *lds_q = lds;                                                 // [tq][qstride]
  float *lds_x = lds + (size_t)tq * qstride + wave * kPairWords;      // this wave's staged pair [64][36]
  float *lds_base2 = lds + (size_t)tq * qstride + 4 * kPairWords;
  float *wn = lds_base2 + wave * 64;                                  // this wave's 64 row norms
  uint32_t *que_row = reinterpret_cast<uint32_t *>(lds_base2 + 4 * 64) + wave * kL2GemmQueue;
  uint32_t *que_q = reinterpret_cast<uint32_t *>(lds_base2 + 4 * 64 + 4 * kL2GemmQueue) + wave * kL2GemmQueue;
  float *lds_nq = lds_base2 + 4 * 64 + 8 * kL2GemmQueue;              // [64] query norms
  unsigned long long *lds_cnt = reinterpret_cast<unsigned long long *>(lds_nq + 64);   // [4] pairs each wave evaluated

  const uint32_t xcd = blockIdx.x & 7u, seq = blockIdx.x >> 3;
  const uint32_t rp = (seq / a.nqt) * 8u + xcd;
  const uint32_t qt = seq % a.nqt;
  const uint32_t q0 = qt * tq;

  // ---- lane `q` of every wave owns the wave's list of query q0 + q
  const bool own = lane < tq && q0 + lane < a.nq;
  const size_t list_base = ((((size_t)(own ? q0 + lane : 0)) * a.nrp + rp) * 4 + wave) * a.k;
  float *list_d = a.part_dist + list_base;
  uint64_t *list_l = a.part_label + list_base;
  if (own)
    for (uint32_t i = 0; i < a.k; ++i) { list_d[i] = __builtin_inff(); list_l[i] = kNoLabel; }
  LaneTop top{__builtin_inff(), kNoLabel, 0u, 0u};

  // row tiles of this partition: a contiguous range
  const uint32_t n_tiles = (a.n_rows + kL2GemmRows - 1) / kL2GemmRows;
  const uint32_t t_base = n_tiles / a.nrp, t_rem = n_tiles % a.nrp;
  const uint32_t first_tile = rp * t_base + (rp < t_rem ? rp : t_rem);
  const uint32_t my_tiles = t_base + (rp < t_rem ? 1u : 0u);
  if (my_tiles == 0) return;   // more partitions than tiles: this block only owes the merge its empty lists

  // ---- Q tile -> LDS (queries past nq replicate the last one; their pairs are masked), then the query norms
  for (uint32_t i = tid; i < tq * (a.row_stride_f / 4); i += 256) {
    const uint32_t q = i / (a.row_stride_f / 4), c4 = i % (a.row_stride_f / 4);
    const uint32_t gq = q0 + q < a.nq ? q0 + q : a.nq - 1;
    *reinterpret_cast<float4 *>(lds_q + (size_t)q * qstride + c4 * 4) = reinterpret_cast<const float4 *>(a.queries + (size_t)gq * a.q_stride_f)[c4];
  }
  __syncthreads();
  {
    const uint32_t q = tid >> 2, part = tid & 3;   // 64 queries x 4 lanes
    float s = 0.f;
    if (q < tq)
      for (uint32_t c4 = part; c4 < a.row_stride_f / 4; c4 += 4) s = sq4(*reinterpret_cast<const float4 *>(lds_q + (size_t)q * qstride + c4 * 4), s);
    s += dpp_quad_xor1(s);
    s += dpp_quad_xor2(s);
    if (part == 0) lds_nq[q] = s;
  }
  __syncthreads();

  // this lane's query columns in the gate: column li of sub-tile qs is query qs * 32 + li of the tile
  const float *qp[2];
  float nq[2];
  bool qv[2];
  uint32_t *qb[2];
#pragma unroll
  for (int qs = 0; qs < 2; ++qs) {
    const uint32_t qin = (uint32_t)qs * 32 + li, qc = qin < tq ? qin : tq - 1;
    qp[qs] = lds_q + (size_t)qc * qstride + kk * 16;
    nq[qs] = lds_nq[qc];
    qv[qs] = qs < kNQS && qin < tq && q0 + qin < a.nq;
    qb[qs] = a.qbound + (qv[qs] ? q0 + qin : q0);
  }
  const float *xb = lds_x + li * kL2GemmXStride + kk * 16;

  // Software pipeline over the wave's stream of pairs, iteration i: the registers loaded for pair i + 1 go to the LDS buffer
  // (the fragments of pair i left it an iteration ago) and into the norms, the fragments of pair i + 1 are requested, the
  // loads of pair i + 2 are issued, the MFMAs of pair i run.  Fragments ping-pong between two register sets.
  L2Pos ld{first_tile * kL2GemmRows + wave * 64, 0, my_tiles * pairs};
  float np[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) np[u] = 0.f;
  L2Stg stg = l2_load<kBf16>(a, lane, ld);
  l2_advance(ld, pairs);
  l2_store<kBf16>(lds_x, lane, stg, np);
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  L2Frag<kNQS> f0 = l2_frag<kNQS>(xb, qp[0], qp[1], 0), f1 = f0;
  stg = l2_load<kBf16>(a, lane, ld);
  l2_advance(ld, pairs);

#define VK_L2_STAGE(PR, F, NF, LAST)                                                   \
  {                                                                                    \
    const uint32_t npr = (PR) + 1 == pairs ? 0u : (PR) + 1;                            \
    if (LAST) l2_norms_out<kBf16>(wn, lane, np); /* the tile's norms are complete */   \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                             \
    l2_store<kBf16>(lds_x, lane, stg, np);                                             \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                             \
    NF = l2_frag<kNQS>(xb, qp[0], qp[1], npr);                                         \
    stg = l2_load<kBf16>(a, lane, ld);                                                 \
    l2_advance(ld, pairs);                                                             \
    l2_mul<kNQS>(acc, F);                                                              \
  }

  uint32_t row_w = first_tile * kL2GemmRows + wave * 64;   // first of the wave's rows in the current tile
  uint32_t qcnt = 0;                                       // pairs waiting in the queue (wave-uniform)
  unsigned long long evaluated = 0;
  for (uint32_t t = 0; t < my_tiles; ++t) {
    uint32_t cancel_now = 0;
    if (a.cancel && (t % kCancelPollTiles) == 0) cancel_now = __hip_atomic_load(a.cancel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // the queries' shared pruning bounds, fetched now and used in the epilogue
    const uint32_t bkey0 = __hip_atomic_load(qb[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t bkey1 = kNQS == 2 ? __hip_atomic_load(qb[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : bkey0;
    f32x16 acc[2][kNQS];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int qs = 0; qs < kNQS; ++qs)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rt][qs][r] = 0.f;
    for (uint32_t pr = 0; pr < pairs; pr += 2) {
      VK_L2_STAGE(pr, f0, f1, false)
      VK_L2_STAGE(pr + 1, f1, f0, pr + 2 == pairs)
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // wn is in place
    // ---- gate: bit (rt * kNQS + qs) * 16 + r of `mask` = the pair of this lane's accumulator element survives
    const float bound[2] = {key_f32(bkey0), key_f32(bkey1)};
    uint64_t mask = 0;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int qs = 0; qs < kNQS; ++qs)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const uint32_t rit = (uint32_t)rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
          const float s = wn[rit] + nq[qs];
          const float av = s - 2.0f * acc[rt][qs][r];
          const float E = fmaf(prm.c_s, s, fmaf(prm.c_a, fabsf(av), prm.c_abs));
          const bool surv = qv[qs] && row_w + rit < a.n_rows && !(av - E > bound[qs]);
          mask |= (uint64_t)(surv ? 1u : 0u) << ((rt * kNQS + qs) * 16 + r);
        }
    // ---- survivors -> queue, 64 at most per step; the queue is drained whenever it holds 16
    for (uint32_t b = 0; b < 32u * kNQS; ++b) {
      const bool mine = (mask >> b) & 1ull;
      const uint64_t bal = __builtin_amdgcn_ballot_w64(mine);
      if (bal == 0) continue;
      if (mine) {
        const uint32_t at = qcnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        const uint32_t r = b & 15u, sub = b >> 4;
        que_row[at] = row_w + (sub / kNQS) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kk;
        que_q[at] = (sub % kNQS) * 32 + li;
      }
      qcnt += (uint32_t)__popcll(bal);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      while (qcnt >= 16) {
        qcnt -= 16;
        top = l2_drain<kBf16>(a, que_row, que_q, qcnt, 16, lds_q, qstride, lane, list_d, list_l, a.qbound + q0, top);
        evaluated += 16;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    row_w += kL2GemmRows;
    if (cancel_now) break;   // the lists keep what they hold
  }
#undef VK_L2_STAGE
  if (qcnt != 0) {   // the end of the stream: what is left, fewer than 16
    top = l2_drain<kBf16>(a, que_row, que_q, 0, qcnt, lds_q, qstride, lane, list_d, list_l, a.qbound + q0, top);
    evaluated += qcnt;
  }
  // ---- the gate counter: once per block
  if (lane == 0) lds_cnt[wave] = evaluated;
  __syncthreads();
  if (tid == 0 && a.evaluated != nullptr) atomicAdd(a.evaluated, lds_cnt[0] + lds_cnt[1] + lds_cnt[2] + lds_cnt[3]);
}

namespace {

// x rounded up to f32
float f32_up(double x) {
  float f = (float)x;
  return (double)f >= x ? f : nextafterf(f, INFINITY);
}

}  // namespace

uint32_t flat_l2_gemm_tile_q(uint32_t row_stride_f) { return l2_gemm_tile_q(row_stride_f); }
bool flat_l2_gemm_supported(uint32_t row_stride_f, uint64_t k) { return l2_gemm_supported(row_stride_f, k); }

hipError_t launch_flat_l2_gemm(const FlatL2GemmArgs &a, hipStream_t s) {
  if (!l2_gemm_supported(a.row_stride_f, a.k) || a.tile_q != l2_gemm_tile_q(a.row_stride_f) || a.nrp == 0 || (a.nrp & 7u) || a.n_rows == 0 ||
      a.nq == 0 || a.nqt != (a.nq + a.tile_q - 1) / a.tile_q || a.chunks != a.row_stride_f / 16 || a.q_stride_f < a.row_stride_f || (a.q_stride_f & 3u))
    return hipErrorInvalidValue;
  const size_t lds = l2_gemm_lds_bytes(a.row_stride_f, a.tile_q);
  const bool two = a.tile_q == 64;
  const void *fn = a.bf16 ? (two ? reinterpret_cast<const void *>(&flat_l2_gemm_kernel<true, 2>) : reinterpret_cast<const void *>(&flat_l2_gemm_kernel<true, 1>))
                          : (two ? reinterpret_cast<const void *>(&flat_l2_gemm_kernel<false, 2>) : reinterpret_cast<const void *>(&flat_l2_gemm_kernel<false, 1>));
  hipError_t e = ensure_max_lds(fn);
  if (e != hipSuccess) return e;
  // the constants of E (header), in double, inflated for E's own roundings, rounded up
  const double u = ldexp(1.0, -24), dp = (double)a.row_stride_f, infl = 1.0 + ldexp(1.0, -20);
  auto gamma = [u](double n) { return n * u / (1.0 - n * u); };
  L2GemmParams prm;
  prm.a = a;
  prm.c_s = f32_up(2.0 * gamma(dp + 3.0) / (1.0 - gamma(dp)) * infl);
  prm.c_a = f32_up((gamma(dp / 16.0 + 6.0) + 2.0 * u) * infl);
  prm.c_abs = f32_up(dp * ldexp(1.0, -123));
  void *params[] = {&prm};
  return hipLaunchKernel(fn, dim3(a.nrp * a.nqt), dim3(256), params, lds, s);
}

}  // namespace vk
