// flat_topk_list.hpp -- the HBM-resident top-k list of ONE lane, shared by the exact matrix-core FLAT kernels: K4
// (flat_gemm.hip, inner-product space, k > 10) and K4e (flat_l2_gemm.hip, L2).  The list itself lives in scratch memory the host
// provides; the lane keeps its worst entry, and a list that has filled publishes that entry's distance for every other list of
// the query.  Device code only.
#pragma once
#include "device_common.hpp"

namespace vk {

struct LaneTop {          // one lane's running top-k state; the list itself lives in HBM scratch
  float thr_d;            // worst kept distance, +inf while the list is not full
  uint64_t thr_l;
  uint32_t thr_i, cnt;
};

// order-preserving f32 <-> u32 (larger float = larger key), for atomicMin on the shared bound
__device__ __forceinline__ uint32_t f32_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// rare path: a (distance,row) that passed the lane's distance gate
__device__ __forceinline__ LaneTop topk_insert(const uint64_t *__restrict__ labels, const uint64_t *__restrict__ allow_bits,
                                            uint64_t allow_nbits, uint32_t k, float dist, uint32_t row, float *list_d,
                                            uint64_t *list_l, uint32_t *qbound_q, LaneTop t) {
  const uint64_t lab = labels[row];
  if (!allow_bit(allow_bits, allow_nbits, lab)) return t;
  if (t.cnt >= k && !dl_less(dist, lab, t.thr_d, t.thr_l)) return t;
  const uint32_t at = t.cnt < k ? t.cnt++ : t.thr_i;
  list_d[at] = dist;
  list_l[at] = lab;
  if (t.cnt == k) {   // recompute this lane's worst entry
    float wd = list_d[0];
    uint64_t wl = list_l[0];
    uint32_t wi = 0;
    for (uint32_t i = 1; i < k; ++i) {
      const float di = list_d[i];
      const uint64_t lv = list_l[i];
      if (dl_less(wd, wl, di, lv)) { wd = di; wl = lv; wi = i; }
    }
    t.thr_d = wd;
    t.thr_l = wl;
    t.thr_i = wi;
    // k kept entries are all <= wd: nothing beyond wd can reach this query's final top-k, whichever
    // list it would land in -- publish it for every other lane working on the query
    __hip_atomic_fetch_min(qbound_q, f32_key(wd), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  return t;
}

}  // namespace vk
