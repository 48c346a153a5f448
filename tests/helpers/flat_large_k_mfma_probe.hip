// flat_large_k_mfma_probe.hip -- TEST INFRASTRUCTURE (tests/test_flat_large_k_mfma_kernels_gpu.py), not part of libvkindex.so.
//
// The two distance launchers of the one-pass FLAT search for k > 1024: the vector kernel and the matrix-core kernel of option
// flat-large-k-mfma.  This probe includes valkey-search_amd/csrc/flat_large_k.hip itself (compile with -I valkey-search_amd/csrc
// and the library's flags), so the product's kernels and launchers are what runs.  The row table is allocated to the byte; the
// distance buffer is filled with a word of the caller's choice and comes back WHOLE; the stream is polled under a time limit.
#include "flat_large_k.hip"

#include "probe_common.hpp"

namespace vk {
hipError_t ensure_max_lds(const void *fn) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
}  // namespace vk

// flat_large_k_host.hpp's decision for an IP / COSINE chunk, and the row partitions the matrix-core launch takes for it
extern "C" int lkm_probe_takes(uint32_t stride_f, uint32_t qc) { return vk::large_k_takes_mfma(true, false, stride_f, qc) ? 1 : 0; }
extern "C" uint32_t lkm_probe_nrp(uint32_t count, uint32_t stride_f, uint32_t qc) { return vk::flat_large_k_mfma_row_partitions(count, stride_f, qc); }

// rows: count rows of stride_f elements (f32, or bf16 with bf16 != 0); queries [qc][stride_f] f32; allow: allow_words words or
// NULL; out: dist_words words = [qc][ld] and whatever the test adds behind it.  mfma != 0: launch_flat_large_k_distance_mfma,
// else launch_flat_large_k_distance with qb.  Returns 0, 1 = refused, 2 = time limit, else the source line of a HIP error.
extern "C" int lkm_probe_distance(uint32_t fill, int mfma, int bf16, int qb, const void *rows, uint32_t stride_f, const uint64_t *labels,
                                  uint32_t count, const float *queries, uint32_t qc, const uint64_t *allow, uint64_t allow_words,
                                  uint64_t allow_nbits, uint64_t ld, uint64_t dist_words, uint32_t *out) {
  if (probe::g_leak || count == 0 || qc == 0 || ld < count || dist_words < (uint64_t)qc * ld || stride_f % 16 != 0 ||
      (allow && allow_words < (allow_nbits + 63) / 64))
    return probe::kRefused;
  probe::Stream st;
  PB_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
  const size_t rows_b = (size_t)count * stride_f * (bf16 ? 2 : 4), q_b = (size_t)qc * stride_f * 4;
  probe::DevBuf d_rows, d_labels, d_q, d_allow, d_dist;
  PB_TRY(d_rows.alloc(rows_b));
  PB_TRY(d_labels.alloc((size_t)count * 8));
  PB_TRY(d_q.alloc(q_b));
  PB_TRY(d_allow.alloc((size_t)allow_words * 8));
  PB_TRY(d_dist.alloc((size_t)dist_words * 4));
  PB_TRY(probe::up(d_rows.p, rows, rows_b, st.s));
  PB_TRY(probe::up(d_labels.p, labels, (size_t)count * 8, st.s));
  PB_TRY(probe::up(d_q.p, queries, q_b, st.s));
  if (allow) PB_TRY(probe::up(d_allow.p, allow, (size_t)allow_words * 8, st.s));
  PB_TRY(probe::fill(d_dist, fill, st.s));
  vk::FlatLargeKArgs a{};
  a.rows = d_rows.p;
  a.labels = d_labels.as<uint64_t>();
  a.queries = d_q.as<float>();
  a.allow_bits = allow ? d_allow.as<uint64_t>() : nullptr;
  a.allow_nbits = allow_nbits;
  a.row_stride_f = a.q_stride_f = stride_f;
  a.chunks = stride_f / 16;
  a.count = count;
  a.qc = qc;
  a.k = a.cap = 1;
  a.ld = ld;
  a.dist = d_dist.as<float>();
  a.state = reinterpret_cast<uint32_t *>(d_dist.p);   // (not used by these launches; the launchers want it non-null)
  PB_TRY(mfma ? vk::launch_flat_large_k_distance_mfma(a, bf16 != 0, st.s) : vk::launch_flat_large_k_distance(a, false, bf16 != 0, qb, st.s));
  PB_WAIT(st.s);
  PB_TRY(probe::down(out, d_dist.p, (size_t)dist_words * 4));
  return 0;
}
