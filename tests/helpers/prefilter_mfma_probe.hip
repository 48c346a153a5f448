// prefilter_mfma_probe.hip -- TEST INFRASTRUCTURE (tests/test_prefilter_mfma_kernels_gpu.py), not part of libvkindex.so.
//
// The distance launcher of the batched pre-filter search (valkey-search_amd/csrc/prefilter_select.hip) over a shared list, with
// K8m (prefilter_mfma_kernel) wished for or not.  This probe includes that translation unit itself (compile with -I
// valkey-search_amd/csrc), so the product's kernels and launcher are what runs.  One call launches launch_prefilter_distance
// once and hands back every word of the output plus the guard words behind it; any HIP error is the return code (the source
// line that saw it), nothing is retried.
#include "prefilter_select.hip"

namespace vk {
// kernels.hpp: the library's version (filter_set.cc) remembers what it has raised; one call per probe call is enough here
hipError_t ensure_max_lds(const void *fn) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
}  // namespace vk

namespace {
struct DevBuf {   // freed on every way out
  void *p = nullptr;
  ~DevBuf() { (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
};
#define PM_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)
constexpr size_t kGuardWords = 64;
}  // namespace

// rows [n_rows][stride_f] f32, or bf16 (2 bytes an element) with bf16 != 0, and NOT ONE byte behind the last row; queries
// [nq][stride_f] f32; idx [shared_len] row slots.  out [nq * shared_len + 64]: every word 0xEEEEEEEE where nothing was written.
extern "C" int pm_probe_distance(const void *rows, uint32_t n_rows, uint32_t stride_f, const float *queries, uint32_t nq, const uint32_t *idx,
                                 uint32_t shared_len, int bf16, uint32_t mfma, uint32_t *out) {
  if (nq == 0 || n_rows == 0 || shared_len == 0 || stride_f == 0 || stride_f % 16 != 0) return 1;
  for (uint32_t i = 0; i < shared_len; ++i)
    if (idx[i] >= n_rows) return 1;   // the kernels read rows[idx]: nothing out of the table
  DevBuf d_rows, d_q, d_idx, d_out;
  const size_t rows_b = (size_t)n_rows * stride_f * (bf16 ? 2 : 4), q_b = (size_t)nq * stride_f * 4;
  const size_t out_b = ((size_t)nq * shared_len + kGuardWords) * 4;
  PM_TRY(d_rows.alloc(rows_b));
  PM_TRY(d_q.alloc(q_b));
  PM_TRY(d_idx.alloc((size_t)shared_len * 4));
  PM_TRY(d_out.alloc(out_b));
  PM_TRY(hipMemcpy(d_rows.p, rows, rows_b, hipMemcpyHostToDevice));
  PM_TRY(hipMemcpy(d_q.p, queries, q_b, hipMemcpyHostToDevice));
  PM_TRY(hipMemcpy(d_idx.p, idx, (size_t)shared_len * 4, hipMemcpyHostToDevice));
  PM_TRY(hipMemset(d_out.p, 0xEE, out_b));
  vk::PrefilterDistArgs da{};
  da.rows = d_rows.p;
  da.queries = static_cast<const float *>(d_q.p);
  da.idx = static_cast<const uint32_t *>(d_idx.p);
  da.out = static_cast<float *>(d_out.p);
  da.row_stride_f = stride_f;
  da.q_stride_f = stride_f;
  da.chunks = stride_f / 16;
  da.nq = nq;
  da.shared_len = shared_len;
  da.mfma = mfma;
  PM_TRY(vk::launch_prefilter_distance(da, false, bf16 != 0, nullptr));
  PM_TRY(hipDeviceSynchronize());
  PM_TRY(hipMemcpy(out, d_out.p, out_b, hipMemcpyDeviceToHost));
  return 0;
}

// prefilter_host.hpp's decision for a launch of this probe, and the query tile K8m would take (0 = a stride it cannot hold)
extern "C" int pm_probe_takes(uint32_t stride_f, uint32_t nq) { return vk::prefilter_takes_mfma(true, true, false, stride_f, nq) ? 1 : 0; }
extern "C" uint32_t pm_probe_tile_q(uint32_t stride_f) { return vk::prefilter_mfma_tile_q(stride_f); }
