// flat_large_k_probe.hip -- TEST INFRASTRUCTURE (tests/test_flat_large_k_kernels_gpu.py), not part of libvkindex.so.
//
// The kernels of the one-pass FLAT search for k > 1024 (valkey-search_amd/csrc/flat_large_k.hip) are reachable through the C
// ABI only behind FlatIndex::search_large_k, which sizes every buffer itself and sorts what comes back.  This probe includes
// that translation unit itself (compile with -I valkey-search_amd/csrc and the library's flags), so the product's kernels and
// launchers are what runs, on buffers the test owns.  Before the launches every output and scratch buffer is filled with a word
// of the caller's choice; only the words the product zeroes (the histogram bins) are zeroed; and every buffer comes back WHOLE,
// so a write outside the contract shows.  The probe never blocks on a launch: it polls the stream with a time limit and
// reports a timeout (return code 2) as a failure, leaving its buffers where they are.
#include "flat_large_k.hip"

#include "probe_common.hpp"

namespace vk {
hipError_t ensure_max_lds(const void *fn) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
}  // namespace vk

using probe::DevBuf;

extern "C" uint32_t lk_probe_slice() { return vk::flat_large_k_slice(); }
extern "C" uint32_t lk_probe_dist_blocks() { return vk::flat_large_k_dist_blocks(); }
extern "C" uint32_t lk_probe_bins() { return vk::kLargeKBins; }
extern "C" uint32_t lk_probe_state_words() { return vk::kLargeKStateWords; }
extern "C" uint64_t lk_probe_cap(uint64_t k) { return vk::large_k_cap(k); }

// The dense distance pass.  rows: count rows of row_stride_f elements (f32, or bf16 with bf16 != 0); queries [qc][row_stride_f]
// f32; allow: allow_words words or NULL; out_dist: dist_words words = the whole buffer, [qc][ld] and whatever the test adds
// behind it.  Returns 0, 1 = refused, 2 = the launch did not finish within the time limit, else the source line of a HIP error.
extern "C" int lk_probe_distance(uint32_t fill, int l2, int bf16, int qb, const void *rows, uint32_t row_stride_f, const uint64_t *labels,
                                 uint32_t count, const float *queries, uint32_t qc, const uint64_t *allow, uint64_t allow_words,
                                 uint64_t allow_nbits, uint64_t ld, uint64_t dist_words, uint32_t *out_dist) {
  if (probe::g_leak || count == 0 || qc == 0 || ld < count || dist_words < (uint64_t)qc * ld || row_stride_f % 16 != 0 ||
      (allow && allow_words < (allow_nbits + 63) / 64))
    return probe::kRefused;
  probe::Stream st;
  PB_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
  const size_t row_bytes = (size_t)row_stride_f * (bf16 ? 2 : 4);
  DevBuf d_rows, d_labels, d_q, d_allow, d_dist;
  PB_TRY(d_rows.alloc((size_t)count * row_bytes));
  PB_TRY(d_labels.alloc((size_t)count * 8));
  PB_TRY(d_q.alloc((size_t)qc * row_stride_f * 4));
  PB_TRY(d_allow.alloc((size_t)allow_words * 8));
  PB_TRY(d_dist.alloc((size_t)dist_words * 4));
  PB_TRY(probe::up(d_rows.p, rows, (size_t)count * row_bytes, st.s));
  PB_TRY(probe::up(d_labels.p, labels, (size_t)count * 8, st.s));
  PB_TRY(probe::up(d_q.p, queries, (size_t)qc * row_stride_f * 4, st.s));
  if (allow) PB_TRY(probe::up(d_allow.p, allow, (size_t)allow_words * 8, st.s));
  PB_TRY(probe::fill(d_dist, fill, st.s));
  vk::FlatLargeKArgs a{};
  a.rows = d_rows.p;
  a.labels = d_labels.as<uint64_t>();
  a.queries = d_q.as<float>();
  a.allow_bits = allow ? d_allow.as<uint64_t>() : nullptr;
  a.allow_nbits = allow_nbits;
  a.row_stride_f = a.q_stride_f = row_stride_f;
  a.chunks = row_stride_f / 16;
  a.count = count;
  a.qc = qc;
  a.k = 1;
  a.cap = 1;
  a.ld = ld;
  a.dist = d_dist.as<float>();
  a.state = reinterpret_cast<uint32_t *>(d_dist.p);   // (not used by this launch; the launcher wants it non-null)
  PB_TRY(vk::launch_flat_large_k_distance(a, l2 != 0, bf16 != 0, qb, st.s));
  PB_WAIT(st.s);
  PB_TRY(probe::down(out_dist, d_dist.p, (size_t)dist_words * 4));
  return 0;
}

// Select + emit over distances the test wrote: dist [qc][ld] as bits, labels [count].  Out, each buffer whole: state
// [qc][state words], hist [qc][bins] (left zeroed by the select), bits and label [out_entries >= qc * cap].
extern "C" int lk_probe_select_emit(uint32_t fill, const uint32_t *dist, const uint64_t *labels, uint32_t count, uint32_t qc, uint64_t ld,
                                    uint32_t k, uint32_t cap, uint64_t out_entries, uint32_t *out_state, uint32_t *out_hist, uint32_t *out_bits,
                                    uint64_t *out_label) {
  if (probe::g_leak || count == 0 || qc == 0 || k == 0 || cap == 0 || ld < count || out_entries < (uint64_t)qc * cap) return probe::kRefused;
  probe::Stream st;
  PB_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
  DevBuf d_dist, d_labels, d_state, d_hist, d_bits, d_label;
  PB_TRY(d_dist.alloc((size_t)qc * ld * 4));
  PB_TRY(d_labels.alloc((size_t)count * 8));
  PB_TRY(d_state.alloc((size_t)qc * vk::kLargeKStateWords * 4));
  PB_TRY(d_hist.alloc((size_t)qc * vk::kLargeKBins * 4));
  PB_TRY(d_bits.alloc((size_t)out_entries * 4));
  PB_TRY(d_label.alloc((size_t)out_entries * 8));
  PB_TRY(probe::up(d_dist.p, dist, (size_t)qc * ld * 4, st.s));
  PB_TRY(probe::up(d_labels.p, labels, (size_t)count * 8, st.s));
  for (const DevBuf *b : {&d_state, &d_hist, &d_bits, &d_label}) PB_TRY(probe::fill(*b, fill, st.s));
  PB_TRY(hipMemsetAsync(d_hist.p, 0, (size_t)qc * vk::kLargeKBins * 4, st.s));   // what FlatIndex::search_large_k zeroes, and nothing else
  vk::FlatLargeKArgs a{};
  a.labels = d_labels.as<uint64_t>();
  a.count = count;
  a.qc = qc;
  a.k = k;
  a.cap = cap;
  a.ld = ld;
  a.dist = d_dist.as<float>();
  a.hist = d_hist.as<uint32_t>();
  a.state = d_state.as<uint32_t>();
  a.out_bits = d_bits.as<uint32_t>();
  a.out_label = d_label.as<uint64_t>();
  PB_TRY(vk::launch_flat_large_k_select(a, st.s));
  PB_TRY(vk::launch_flat_large_k_emit(a, st.s));
  PB_WAIT(st.s);
  PB_TRY(probe::down(out_state, d_state.p, (size_t)qc * vk::kLargeKStateWords * 4));
  PB_TRY(probe::down(out_hist, d_hist.p, (size_t)qc * vk::kLargeKBins * 4));
  PB_TRY(probe::down(out_bits, d_bits.p, (size_t)out_entries * 4));
  PB_TRY(probe::down(out_label, d_label.p, (size_t)out_entries * 8));
  return 0;
}
