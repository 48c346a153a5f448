// prefilter_probe.hip -- TEST INFRASTRUCTURE (tests/test_prefilter_kernels_gpu.py), not part of libvkindex.so.
//
// The batched pre-filter search's two kernels (valkey-search_amd/csrc/prefilter_select.hip: K8b distances over a CSR of
// row-slot lists, K8c threshold + ordered compaction) are reachable through the C ABI only behind the host's heap rule,
// which gives the right answer for ANY superset of {distance <= T}: most kernel errors are invisible there.  This probe
// includes that translation unit itself (compile with -I valkey-search_amd/csrc), so the product's kernels and launchers
// are what runs, on inputs the test chooses, and hands back exactly what the kernels wrote: every distance, every count
// word, every (index, distance bits) pair.  Each call launches each kernel once; any HIP error is the return code (the
// source line that saw it), nothing is retried.
#include "prefilter_select.hip"

#include <vector>

namespace vk {
// kernels.hpp: the library's version (filter_set.cc) remembers what it has raised; one call per probe call is enough here
hipError_t ensure_max_lds(const void *fn) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
}  // namespace vk

namespace {

struct DevBuf {   // freed on every way out
  void *p = nullptr;
  ~DevBuf() { (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

#define PF_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)

// offsets [nq + 1]: from 0, ascending
bool ascending(const uint32_t *b, uint32_t nq) {
  if (b[0] != 0) return false;
  for (uint32_t q = 0; q < nq; ++q)
    if (b[q + 1] < b[q]) return false;
  return true;
}

int run_select(const float *d_dist, const uint32_t *d_seg, uint32_t nq, uint32_t shared_len, uint32_t k, uint32_t cap, uint32_t *out_count,
               uint32_t *out_cand) {
  DevBuf count, cand;
  const size_t count_b = (size_t)nq * 4, cand_b = (size_t)nq * cap * 8;
  PF_TRY(count.alloc(count_b));
  PF_TRY(cand.alloc(cand_b));
  PF_TRY(hipMemset(count.p, 0xEE, count_b));   // a word the kernel never writes: an unwritten count / pair shows
  PF_TRY(hipMemset(cand.p, 0xEE, cand_b));
  vk::PrefilterSelectArgs sa{};
  sa.dist = d_dist;
  sa.seg_begin = d_seg;
  sa.shared_len = shared_len;
  sa.nq = nq;
  sa.k = k;
  sa.cap = cap;
  sa.count = count.as<uint32_t>();
  sa.cand = cand.as<uint2>();
  PF_TRY(vk::launch_prefilter_select(sa, nullptr));
  PF_TRY(hipDeviceSynchronize());
  PF_TRY(hipMemcpy(out_count, count.p, count_b, hipMemcpyDeviceToHost));
  PF_TRY(hipMemcpy(out_cand, cand.p, cand_b, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

// K8c alone.  dist: the segments' distances, [seg_begin[nq]] (CSR) or [nq][shared_len] (seg_begin == nullptr).
// out_count [nq], out_cand [nq][cap][2] = (index in the segment, distance bits); 0xEEEEEEEE where the kernel wrote nothing.
extern "C" int pf_probe_select(const float *dist, const uint32_t *seg_begin, uint32_t nq, uint32_t shared_len, uint32_t k, uint32_t cap,
                               uint32_t *out_count, uint32_t *out_cand) {
  if (nq == 0 || k == 0 || cap < k) return 1;
  if (seg_begin && !ascending(seg_begin, nq)) return 1;
  const size_t entries = seg_begin ? seg_begin[nq] : (size_t)nq * shared_len;
  DevBuf d, seg;
  PF_TRY(d.alloc(entries * 4));
  if (entries) PF_TRY(hipMemcpy(d.p, dist, entries * 4, hipMemcpyHostToDevice));
  if (seg_begin) {
    PF_TRY(seg.alloc((size_t)(nq + 1) * 4));
    PF_TRY(hipMemcpy(seg.p, seg_begin, (size_t)(nq + 1) * 4, hipMemcpyHostToDevice));
  }
  return run_select(d.as<float>(), seg_begin ? seg.as<uint32_t>() : nullptr, nq, shared_len, k, cap, out_count, out_cand);
}

// K8b then K8c.  rows [n_rows][stride_f] f32, zero padded (stride_f a multiple of 16); queries [nq][stride_f] padded
// alike; idx = row slots, [seg_begin[nq]] or [shared_len]; tile_begin [nq + 1] as prefilter_tiles gives it (with seg_begin).
// out_dist: every distance K8b wrote, laid out like K8c's input (bits 0xEEEEEEEE where it wrote nothing).
extern "C" int pf_probe_distance_select(const float *rows, uint32_t n_rows, uint32_t stride_f, const float *queries, uint32_t nq,
                                        const uint32_t *idx, const uint32_t *seg_begin, const uint32_t *tile_begin, uint32_t shared_len, int l2,
                                        uint32_t k, uint32_t cap, float *out_dist, uint32_t *out_count, uint32_t *out_cand) {
  if (nq == 0 || k == 0 || cap < k || n_rows == 0 || stride_f == 0 || stride_f % 16 != 0) return 1;
  if ((seg_begin == nullptr) != (tile_begin == nullptr)) return 1;
  const size_t n_idx = seg_begin ? 0 : shared_len;
  size_t slots = n_idx, entries = (size_t)nq * shared_len;
  if (seg_begin) {
    if (!ascending(seg_begin, nq) || !ascending(tile_begin, nq)) return 1;
    for (uint32_t q = 0; q < nq; ++q)   // the tile table the kernel trusts: one tile per 64 entries of each segment
      if (tile_begin[q + 1] - tile_begin[q] != vk::prefilter_tiles(seg_begin[q + 1] - seg_begin[q])) return 1;
    slots = entries = seg_begin[nq];
  }
  for (size_t i = 0; i < slots; ++i)
    if (idx[i] >= n_rows) return 1;   // K8b reads rows[idx]: nothing out of the table
  DevBuf d_rows, d_q, d_idx, d_seg, d_tile, d_out;
  const size_t rows_b = (size_t)n_rows * stride_f * 4, q_b = (size_t)nq * stride_f * 4;
  PF_TRY(d_rows.alloc(rows_b));
  PF_TRY(d_q.alloc(q_b));
  PF_TRY(d_idx.alloc(slots * 4));
  PF_TRY(d_out.alloc(entries * 4));
  PF_TRY(hipMemcpy(d_rows.p, rows, rows_b, hipMemcpyHostToDevice));
  PF_TRY(hipMemcpy(d_q.p, queries, q_b, hipMemcpyHostToDevice));
  if (slots) PF_TRY(hipMemcpy(d_idx.p, idx, slots * 4, hipMemcpyHostToDevice));
  PF_TRY(hipMemset(d_out.p, 0xEE, entries * 4));
  if (seg_begin) {
    PF_TRY(d_seg.alloc((size_t)(nq + 1) * 4));
    PF_TRY(d_tile.alloc((size_t)(nq + 1) * 4));
    PF_TRY(hipMemcpy(d_seg.p, seg_begin, (size_t)(nq + 1) * 4, hipMemcpyHostToDevice));
    PF_TRY(hipMemcpy(d_tile.p, tile_begin, (size_t)(nq + 1) * 4, hipMemcpyHostToDevice));
  }
  vk::PrefilterDistArgs da{};
  da.rows = d_rows.p;
  da.queries = d_q.as<float>();
  da.idx = d_idx.as<uint32_t>();
  da.seg_begin = seg_begin ? d_seg.as<uint32_t>() : nullptr;
  da.tile_begin = seg_begin ? d_tile.as<uint32_t>() : nullptr;
  da.out = d_out.as<float>();
  da.row_stride_f = stride_f;
  da.q_stride_f = stride_f;
  da.chunks = stride_f / 16;
  da.nq = nq;
  da.shared_len = seg_begin ? 0 : shared_len;
  da.n_tiles = seg_begin ? tile_begin[nq] : 0;
  PF_TRY(vk::launch_prefilter_distance(da, l2 != 0, false, nullptr));
  PF_TRY(hipDeviceSynchronize());
  if (entries) PF_TRY(hipMemcpy(out_dist, d_out.p, entries * 4, hipMemcpyDeviceToHost));
  return run_select(d_out.as<float>(), da.seg_begin, nq, da.shared_len, k, cap, out_count, out_cand);
}

// host only: prefilter_select_model (prefilter_host.hpp) on one segment; out_idx [cap]; returns the model's count word
extern "C" uint32_t pf_probe_model(const float *dist, uint64_t n, uint64_t k, uint64_t cap, uint32_t *out_idx, uint32_t *out_stored) {
  std::vector<uint32_t> idx;
  const uint32_t count = vk::prefilter_select_model(dist, n, k, cap, &idx);
  for (size_t i = 0; i < idx.size(); ++i) out_idx[i] = idx[i];
  *out_stored = (uint32_t)idx.size();
  return count;
}

extern "C" uint32_t pf_probe_tiles(uint64_t entries) { return vk::prefilter_tiles(entries); }
