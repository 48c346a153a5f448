// hnsw_relink_order.hpp -- the order in which hnsw_relink_kernel (hnsw_build.hip, K9) hands a full node's candidates (old
// neighbours + the batch's additions) to the heuristic.  No HIP call in here, and the same text compiles for the host:
// tests/helpers/san_relink_order_main.cc drives it with plain memory under the sanitizers.
//
// The kernel sorts by counting: entry i goes to slot rank(i) = the number of entries that come before it.  Every slot of
// [0, total) is written exactly once only if "comes before" is a strict TOTAL order, so it is one, over three keys in turn:
//   1. relink_order_key(distance): u32 order == float order; -0 and +0 share one key (they compare equal, the id decides
//      between them, as `<` / `==` on the floats did); every NaN, of either sign and any payload, has the one key
//      0xFFFFFFFF, above +inf (0xFF800000): a candidate whose distance is not a number is the last the heuristic looks at;
//   2. the id, smaller first (hnswlib's heap pops the LARGER id of a tie first -- this order is the kernel's own);
//   3. the position in the candidate array: two entries with equal (distance, id) still get two ranks.
// On candidates without NaN and without repeated (distance, id) pairs this is the order `d < d' || (d == d' && id < id')`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VK_RELINK_HD __host__ __device__ inline
#else
#define VK_RELINK_HD inline
#endif

namespace vk {

VK_RELINK_HD uint32_t relink_order_key(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;   // NaN, either sign: last
  if (u == 0x80000000u) u = 0;                               // -0 -> +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// does candidate a = (key, id, position) come before candidate b?
VK_RELINK_HD bool relink_before(uint32_t ka, uint32_t ia, uint32_t pa, uint32_t kb, uint32_t ib, uint32_t pb) {
  if (ka != kb) return ka < kb;
  if (ia != ib) return ia < ib;
  return pa < pb;
}

// slot of candidate i among d[0..total) / id[0..total): the ranks of i = 0..total-1 are a permutation of 0..total-1
VK_RELINK_HD uint32_t relink_rank(const float *d, const uint32_t *id, uint32_t total, uint32_t i) {
  const uint32_t ki = relink_order_key(d[i]), ii = id[i];
  uint32_t rank = 0;
  for (uint32_t o = 0; o < total; ++o) rank += relink_before(relink_order_key(d[o]), id[o], o, ki, ii, i) ? 1u : 0u;
  return rank;
}

}  // namespace vk
