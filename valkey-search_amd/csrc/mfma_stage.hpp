// mfma_stage.hpp -- the register-staging helpers of the exact f32 matrix-core kernels that take their rows HBM -> registers -> a
// per-wave LDS ring -> MFMA operands: K8m (prefilter_mfma_kernel, prefilter_select.hip: gathered rows) and the dense pass of the
// one-pass search for k > 1024 (flat_dense_mfma_kernel, flat_large_k.hip: contiguous rows).  What differs between the two -- where
// a lane's rows are -- stays with each kernel; what is here is the same for both: the stage's place in LDS, the operand
// fragments, the sixteen k-ordered chains, and the pinned interleave of a stage's memory operations with its MFMAs.
// Device code only; each translation unit gets its own copy (anonymous namespace).
#pragma once
#include "device_common.hpp"

namespace vk {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr uint32_t kMfmaTile = 128;
constexpr uint32_t kMfmaXStride = 36;                     // dwords per staged row: 2 chunks + 4 pad
constexpr uint32_t kMfmaBufFloats = 32 * kMfmaXStride;    // one stage of one wave
constexpr uint32_t kMfmaBufs = 3;

// register-resident sets are plain structs handled BY VALUE (K4's note: arrays by reference end up in scratch)
struct MfmaStg { float4 v0, v1, v2, v3; };
struct MfmaFrag { float4 q0, q1, q2, q3, x0, x1, x2, x3; };

// which rows of its wave's 32 a lane stages.  f32: a stage of a row is 8 pieces of 16 B, lane -> row lane / 8 (+ 8, 16, 24),
// piece lane % 8.  bf16: 4 pieces, lane -> a row of the first 16 (+ 16), piece lane % 4; the 16 lanes of a store pass take rows
// {2G, 2G + 1, 2G + 8, 2G + 9} so that their stores land in 16 different bank groups (K4's bf16_lane_row)
template <bool kBf16>
__device__ __forceinline__ uint32_t mfma_lane_row(uint32_t lane) {
  if constexpr (kBf16) {
    const uint32_t G = lane >> 4, rr = (lane >> 2) & 3;
    return 2 * G + (rr & 1) + 8 * (rr >> 1);
  } else {
    return lane >> 3;
  }
}
// eight bf16 (one 16-byte piece) -> two float4: a 16-bit shift, exact
__device__ __forceinline__ void mfma_widen8(const float4 raw, float4 &lo, float4 &hi) {
  const uint32_t w0 = __float_as_uint(raw.x), w1 = __float_as_uint(raw.y), w2 = __float_as_uint(raw.z), w3 = __float_as_uint(raw.w);
  lo = float4{__uint_as_float(w0 << 16), __uint_as_float(w0 & 0xffff0000u), __uint_as_float(w1 << 16), __uint_as_float(w1 & 0xffff0000u)};
  hi = float4{__uint_as_float(w2 << 16), __uint_as_float(w2 & 0xffff0000u), __uint_as_float(w3 << 16), __uint_as_float(w3 & 0xffff0000u)};
}
template <bool kBf16>
__device__ __forceinline__ void mfma_stage_store(float *buf, uint32_t lane, const MfmaStg s) {
  if constexpr (kBf16) {
    // the raw pieces are made opaque HERE, one stage after their load was issued: otherwise the compiler widens a piece right
    // behind its load and every stage waits for the round trip it has just started (K4)
    float4 r0 = s.v0, r1 = s.v1;
    asm volatile("" : "+v"(r0.x), "+v"(r0.y), "+v"(r0.z), "+v"(r0.w), "+v"(r1.x), "+v"(r1.y), "+v"(r1.z), "+v"(r1.w));
    float4 a0, a1, b0, b1;
    mfma_widen8(r0, a0, a1);
    mfma_widen8(r1, b0, b1);
    float *p0 = buf + mfma_lane_row<true>(lane) * kMfmaXStride + (lane & 3) * 8;
    float *p1 = p0 + 16 * kMfmaXStride;
    *reinterpret_cast<float4 *>(p0) = a0;
    *reinterpret_cast<float4 *>(p0 + 4) = a1;
    *reinterpret_cast<float4 *>(p1) = b0;
    *reinterpret_cast<float4 *>(p1 + 4) = b1;
  } else {
    float *p = buf + (lane >> 3) * kMfmaXStride + (lane & 7) * 4;
    *reinterpret_cast<float4 *>(p) = s.v0;
    *reinterpret_cast<float4 *>(p + 8 * kMfmaXStride) = s.v1;
    *reinterpret_cast<float4 *>(p + 16 * kMfmaXStride) = s.v2;
    *reinterpret_cast<float4 *>(p + 24 * kMfmaXStride) = s.v3;
  }
}
// LDS -> registers: this lane's query (A) and row (B) operands of one stage: lane = (query or entry lane & 31, chunk lane >> 5)
__device__ __forceinline__ MfmaFrag mfma_frag_load(const float *xb, const float *q_row, uint32_t st, uint32_t kk) {
  const float *qb = q_row + (st * 2 + kk) * 16;
  MfmaFrag f;
  f.x0 = *reinterpret_cast<const float4 *>(xb);
  f.x1 = *reinterpret_cast<const float4 *>(xb + 4);
  f.x2 = *reinterpret_cast<const float4 *>(xb + 8);
  f.x3 = *reinterpret_cast<const float4 *>(xb + 12);
  f.q0 = *reinterpret_cast<const float4 *>(qb);
  f.q1 = *reinterpret_cast<const float4 *>(qb + 4);
  f.q2 = *reinterpret_cast<const float4 *>(qb + 8);
  f.q3 = *reinterpret_cast<const float4 *>(qb + 12);
  return f;
}

#define VK_PF_MFMA4(P, QV, XV)                                                                                \
  acc[4 * P + 0] = __builtin_amdgcn_mfma_f32_32x32x2f32(QV.x, XV.x, kZeroC ? zero : acc[4 * P + 0], 0, 0, 0); \
  acc[4 * P + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(QV.y, XV.y, kZeroC ? zero : acc[4 * P + 1], 0, 0, 0); \
  acc[4 * P + 2] = __builtin_amdgcn_mfma_f32_32x32x2f32(QV.z, XV.z, kZeroC ? zero : acc[4 * P + 2], 0, 0, 0); \
  acc[4 * P + 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(QV.w, XV.w, kZeroC ? zero : acc[4 * P + 3], 0, 0, 0);
template <bool kZeroC>
__device__ __forceinline__ void mfma_stage_mul(f32x16 (&acc)[16], const MfmaFrag f) {
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  VK_PF_MFMA4(0, f.q0, f.x0)
  VK_PF_MFMA4(1, f.q1, f.x1)
  VK_PF_MFMA4(2, f.q2, f.x2)
  VK_PF_MFMA4(3, f.q3, f.x3)
}
#undef VK_PF_MFMA4

// The memory operations of one pipelined stage pinned between its 16 MFMAs, as in K4 (kBf16 of the kernel in scope):
//   M V M V M V M V | R R R R | M M M M | R R | M W M W M W M W | R R | M M M M
// (V = a global load of the stage three ahead, R = an LDS read of the next stage's fragments, W = an LDS write of the stage two
// ahead -- with bf16 rows behind the four VALU operations that widen one float4)
#define VK_MFMA_STAGE_SCHED()                                                                   \
  _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                               \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                          \
    __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);                                          \
  }                                                                                             \
  __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                                            \
  __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                            \
  __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                            \
  _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                               \
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                                          \
    if constexpr (kBf16) __builtin_amdgcn_sched_group_barrier(0x002, 4, 0); /* widen a float4 */ \
    __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);                                          \
  }                                                                                             \
  __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);                                            \
  __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                            \
  __builtin_amdgcn_sched_barrier(0);

}  // namespace

}  // namespace vk
