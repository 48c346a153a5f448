// flat_select_probe.hip -- TEST INFRASTRUCTURE (tests/test_flat_select_kernels_gpu.py), not part of libvkindex.so.
//
// The back half of valkey-search_amd/csrc/flat_scan.hip -- the fused re-rank (flat_rerank_kernel), the list-mode scan
// (flat_scan_kernel<.., kIdx = true>), the two merges (merge_select_kernel, merge_topk_kernel<1|4|16>), K8
// (gather_distance_kernel), kth_bound_kernel and fill_empty_kernel -- is reachable through the C ABI only as "the answer of a
// search": which merge path a query takes, whether its list is re-ranked by one block or by eight, what a kernel leaves
// behind the count, none of that can be chosen or seen there.  This probe includes that translation unit itself (compile
// with -I valkey-search_amd/csrc), so the product's kernels and launchers are what runs, on buffers the probe owns: every
// OUTPUT and WORKSPACE buffer is filled with a 32-bit pattern the caller passes before the first launch -- except the words
// the product itself zeroes first (flat_qprep_kernel: done_cnt, reranked; scan_filter: redo_cnt) -- and handed back whole,
// so that a test can hold every word against a model and see every word a kernel did not write.  Each call launches each
// kernel once.  Return codes: 0 ok, 1 refused arguments, else the source line that saw a HIP error; nothing is retried.
#include "flat_scan.hip"

#include <algorithm>
#include <cstring>
#include <vector>

namespace vk {
// kernels.hpp: the library's version (filter_set.cc) remembers what it has raised; one call per launch is enough here
hipError_t ensure_max_lds(const void *fn) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
}  // namespace vk

namespace {

struct DevBuf {   // freed on every way out
  void *p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { (void)hipFree(p); }
  hipError_t alloc(size_t b) { bytes = b ? b : 4; return hipMalloc(&p, bytes); }
  template <class T> T *as() const { return static_cast<T *>(p); }
};

#define FS_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)

// every 32-bit word of the buffer = pattern (all sizes here are multiples of 4)
hipError_t fill32(const DevBuf &b, uint32_t pattern) { return hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b.p), (int)pattern, b.bytes / 4); }
hipError_t upload(const DevBuf &b, const void *src, size_t bytes) { return bytes ? hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) : hipSuccess; }
hipError_t download(void *dst, const DevBuf &b, size_t bytes) { return bytes ? hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }

}  // namespace

extern "C" {

// ---- the merges ------------------------------------------------------------------------------------------------------------------
struct FsMergeIO {
  const float *in_dist;        // [in_entries]: entry (part, q, i) at part * part_stride + q * q_stride + i
  const uint64_t *in_label;    // [in_entries]
  uint64_t in_entries;
  uint64_t part_stride, q_stride;
  uint32_t parts, per_part, nq, k, e, out_ld;
  const uint32_t *ovf_q;       // optional [nq]
  const uint32_t *q_index;     // optional [nq]: redo mode, with nq_dev (the device word holds it)
  uint32_t nq_dev;
  uint32_t use_flag, flag_value, run_if, run_hi;   // use_flag: run_flag points at a device word holding flag_value
  uint32_t direct_topk1;       // 1: merge_topk_kernel<1> itself, with the LDS size launch_merge_topk computes (not the selection)
  uint32_t fill;
  float *out_dist;             // [nq][max(out_ld, k)]
  uint64_t *out_label;         // [nq][max(out_ld, k)]
  uint32_t *out_n;             // [nq]
  uint32_t *redo_cnt;          // [1]
  uint32_t *redo_list;         // [nq]
};

int fs_probe_merge(const FsMergeIO *io) {
  const uint64_t total = (uint64_t)io->parts * io->per_part;
  if (total == 0) return 1;
  if (io->k == 0 || (io->e != 1 && io->e != 4 && io->e != 16) || io->k > 64u * io->e) return 1;
  if (io->direct_topk1 && io->e != 1) return 1;
  if ((io->q_index != nullptr) && io->nq_dev > io->nq) return 1;
  const uint32_t nq = io->nq, ld = std::max(io->out_ld, io->k);
  // nothing is read outside the input: the last entry of the last part of the last list
  if (nq != 0 && (uint64_t)(io->parts - 1) * io->part_stride + (uint64_t)(nq - 1) * io->q_stride + io->per_part > io->in_entries) return 1;
  if (io->q_index)
    for (uint32_t i = 0; i < nq; ++i)
      if (io->q_index[i] >= nq) return 1;
  DevBuf d_in_d, d_in_l, d_ovf, d_qi, d_words, d_out_d, d_out_l, d_out_n, d_redo;
  FS_TRY(d_in_d.alloc(io->in_entries * 4));
  FS_TRY(d_in_l.alloc(io->in_entries * 8));
  FS_TRY(d_ovf.alloc((size_t)nq * 4));
  FS_TRY(d_qi.alloc((size_t)nq * 4));
  FS_TRY(d_words.alloc(16));                         // nq_dev | run flag | redo_cnt | -
  FS_TRY(d_out_d.alloc((size_t)nq * ld * 4));
  FS_TRY(d_out_l.alloc((size_t)nq * ld * 8));
  FS_TRY(d_out_n.alloc((size_t)nq * 4));
  FS_TRY(d_redo.alloc((size_t)nq * 4));
  FS_TRY(upload(d_in_d, io->in_dist, io->in_entries * 4));
  FS_TRY(upload(d_in_l, io->in_label, io->in_entries * 8));
  if (io->ovf_q) FS_TRY(upload(d_ovf, io->ovf_q, (size_t)nq * 4));
  if (io->q_index) FS_TRY(upload(d_qi, io->q_index, (size_t)nq * 4));
  const uint32_t words[4] = {io->nq_dev, io->flag_value, 0u, 0u};   // redo_cnt: zero, as scan_filter leaves it before the passes
  FS_TRY(upload(d_words, words, 16));
  for (const DevBuf *b : {&d_out_d, &d_out_l, &d_out_n, &d_redo}) FS_TRY(fill32(*b, io->fill));

  vk::MergeArgs m{};
  m.in_dist = d_in_d.as<float>();
  m.in_label = d_in_l.as<uint64_t>();
  m.part_stride = io->part_stride;
  m.q_stride = io->q_stride;
  m.parts = io->parts;
  m.per_part = io->per_part;
  m.k = io->k;
  m.out_ld = io->out_ld;
  m.out_dist = d_out_d.as<float>();
  m.out_label = d_out_l.as<uint64_t>();
  m.out_n = d_out_n.as<uint32_t>();
  if (io->use_flag) {
    m.run_flag = d_words.as<uint32_t>() + 1;
    m.run_if = io->run_if;
    m.run_hi = io->run_hi;
  }
  if (io->ovf_q) {
    m.ovf_q = d_ovf.as<uint32_t>();
    m.redo_cnt = d_words.as<uint32_t>() + 2;
    m.redo_list = d_redo.as<uint32_t>();
  }
  if (io->q_index) {
    m.q_index = d_qi.as<uint32_t>();
    m.nq_dev = d_words.as<uint32_t>();
  }
  if (io->direct_topk1) {
    if (nq != 0) {
      // launch_merge_topk, behind the selection's branch: "MergeArgs a = a_in; if (a.out_ld < a.k) ..." and "const size_t lds = ..."
      vk::MergeArgs a = m;
      if (a.out_ld < a.k) a.out_ld = a.k;
      const int e = 1;
      const size_t lds = (size_t)(3 * e * 64 + 2) * 4 + (size_t)3 * e * 64 * 8;
      hipLaunchKernelGGL((vk::merge_topk_kernel<1>), dim3(nq), dim3(256), lds, nullptr, a);
      FS_TRY(hipGetLastError());
    }
  } else {
    FS_TRY(vk::launch_merge_topk(m, (int)io->e, nq, nullptr));
  }
  FS_TRY(hipDeviceSynchronize());
  FS_TRY(download(io->out_dist, d_out_d, (size_t)nq * ld * 4));
  FS_TRY(download(io->out_label, d_out_l, (size_t)nq * ld * 8));
  FS_TRY(download(io->out_n, d_out_n, (size_t)nq * 4));
  FS_TRY(download(io->redo_list, d_redo, (size_t)nq * 4));
  FS_TRY(hipMemcpy(io->redo_cnt, d_words.as<uint32_t>() + 2, 4, hipMemcpyDeviceToHost));
  return 0;
}

// ---- the re-rank -----------------------------------------------------------------------------------------------------------------
struct FsRerankIO {
  const void *rows;            // [n_rows][stride] f32, or bf16 as uint16
  const uint64_t *labels;      // [n_rows]
  const float *queries;        // [nq][stride] padded
  const uint32_t *list_begin;  // [nq + 1]: the survivors of query q are list_row / list_val [list_begin[q], list_begin[q + 1])
  const uint32_t *list_row;    // row slots
  const float *list_val;       // their approximate scores
  const float *qcoef;          // [nq][4]
  const uint32_t *tile_norm;   // [n_tiles] f32 bits, n_tiles >= ceil(n_rows / 128)
  const uint64_t *allow_bits;  // optional [(allow_nbits + 63) / 64]
  uint64_t allow_nbits;
  const uint32_t *ovf_q;       // optional [nq]
  uint32_t n_rows, stride, bf16, l2, nq, k, out_ld, cand_cap, n_tiles;
  uint32_t prune, fused, fill;
  float *out_dist;             // [nq][max(out_ld, k)]
  uint64_t *out_label;
  uint32_t *out_n;             // [nq]
  uint32_t *reranked;          // [nq]
  uint32_t *done_cnt;          // [nq]
  uint32_t *redo_cnt;          // [1]
  uint32_t *redo_list;         // [nq]
  float *part_dist;            // [nq][8 * (e == 1 ? 1 : 4) * k], e = flat_scan_slots_per_lane(k)
  uint64_t *part_label;
  uint32_t *qchunk;            // [nq][kSpillPerQuery]: the chunk table the probe made (slot = chunk + 2, 0 = none)
};

// entries of one query's partial lists (scan_filter: "const uint64_t per_q = ...")
uint32_t fs_probe_per_q(uint32_t k) {
  const int e = vk::flat_scan_slots_per_lane(k);
  return e == 0 ? 0 : 8u * (e == 1 ? 1u : 4u) * k;
}

int fs_probe_rerank(const FsRerankIO *io) {
  const uint32_t nq = io->nq, dp = io->stride, cap = io->cand_cap, k = io->k;
  const int e = vk::flat_scan_slots_per_lane(k);
  if (nq == 0 || io->n_rows == 0 || dp == 0 || dp % 64 != 0 || dp > 4096 || k == 0 || e == 0 || cap == 0) return 1;
  if (io->fused && k > 64) return 1;
  if (io->prune && !io->fused) return 1;             // the second bound is the fused kernel's
  if (io->n_tiles < (io->n_rows + 127) / 128) return 1;
  if ((io->allow_bits != nullptr) != (io->allow_nbits != 0)) return 1;
  if (io->list_begin[0] != 0) return 1;
  // chunk numbers: dealt round robin over the queries that spill and two apart -- a query's chunks are not contiguous, different
  // queries' chunks interleave
  std::vector<uint32_t> need(nq), qchunk((size_t)nq * vk::kSpillPerQuery, 0u);
  uint32_t dealt = 0, most_need = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    if (io->list_begin[q + 1] < io->list_begin[q]) return 1;
    const uint32_t cnt = io->list_begin[q + 1] - io->list_begin[q];
    need[q] = cnt > cap ? (cnt - cap + vk::kSpillChunk - 1) / vk::kSpillChunk : 0;
    if (need[q] > vk::kSpillPerQuery) return 1;      // survivors lost: out of scope here
    most_need = std::max(most_need, need[q]);
  }
  for (uint32_t i = 0; i < io->list_begin[nq]; ++i)
    if (io->list_row[i] >= io->n_rows) return 1;     // the kernels read rows[slot], labels[slot], tile_norm[slot >> 7]
  for (uint32_t j = 0; j < most_need; ++j)
    for (uint32_t q = 0; q < nq; ++q)
      if (need[q] > j) qchunk[(size_t)q * vk::kSpillPerQuery + j] = 2u + (2u * dealt++ + 1u);
  const uint32_t n_chunks = 2 * dealt + 1;
  if (n_chunks > 512) return 1;
  const uint32_t per_q = fs_probe_per_q(k), ld = std::max(io->out_ld, k);
  // What lies behind a list -- the rest of a private list, the rest of its last chunk, the chunks nobody took -- is what an
  // earlier batch left there: some row slot of the index and some score.  The slot is the pattern reduced to the table (a
  // kernel that reads it ranks a row the list does not hold, without reading outside the table); the score is the pattern.
  const uint32_t stale_row = io->fill % io->n_rows;
  std::vector<uint32_t> h_cand((size_t)nq * cap, stale_row), h_val((size_t)nq * cap, io->fill), h_cnt(nq);
  std::vector<uint32_t> h_spill((size_t)n_chunks * vk::kSpillChunk, stale_row), h_spill_val((size_t)n_chunks * vk::kSpillChunk, io->fill);
  for (uint32_t q = 0; q < nq; ++q) {
    const uint32_t b = io->list_begin[q], cnt = io->list_begin[q + 1] - b;
    h_cnt[q] = cnt;
    for (uint32_t i = 0; i < cnt; ++i) {
      uint32_t v;
      memcpy(&v, io->list_val + b + i, 4);
      if (i < cap) {
        h_cand[(size_t)q * cap + i] = io->list_row[b + i];
        h_val[(size_t)q * cap + i] = v;
      } else {
        const uint32_t jj = i - cap;
        const size_t at = (size_t)(qchunk[(size_t)q * vk::kSpillPerQuery + jj / vk::kSpillChunk] - 2u) * vk::kSpillChunk + jj % vk::kSpillChunk;
        h_spill[at] = io->list_row[b + i];
        h_spill_val[at] = v;
      }
    }
  }
  const size_t esz = io->bf16 ? 2 : 4;
  const size_t allow_b = ((size_t)io->allow_nbits + 63) / 64 * 8;
  DevBuf d_rows, d_lab, d_q, d_allow, d_tn, d_coef, d_cnt, d_cand, d_val, d_spill, d_spill_val, d_chunk, d_ovf, d_zero, d_redo, d_part_d, d_part_l,
      d_out_d, d_out_l, d_out_n;
  FS_TRY(d_rows.alloc((size_t)io->n_rows * dp * esz));
  FS_TRY(d_lab.alloc((size_t)io->n_rows * 8));
  FS_TRY(d_q.alloc((size_t)nq * dp * 4));
  FS_TRY(d_allow.alloc(allow_b));
  FS_TRY(d_tn.alloc((size_t)io->n_tiles * 4));
  FS_TRY(d_coef.alloc((size_t)nq * 16));
  FS_TRY(d_cnt.alloc((size_t)nq * 4));
  FS_TRY(d_cand.alloc(h_cand.size() * 4));
  FS_TRY(d_val.alloc(h_val.size() * 4));
  FS_TRY(d_spill.alloc(h_spill.size() * 4));
  FS_TRY(d_spill_val.alloc(h_spill_val.size() * 4));
  FS_TRY(d_chunk.alloc(qchunk.size() * 4));
  FS_TRY(d_ovf.alloc((size_t)nq * 4));
  FS_TRY(d_zero.alloc(((size_t)2 * nq + 1) * 4));     // done_cnt [nq] | reranked [nq] | redo_cnt
  FS_TRY(d_redo.alloc((size_t)nq * 4));
  FS_TRY(d_part_d.alloc((size_t)nq * per_q * 4));
  FS_TRY(d_part_l.alloc((size_t)nq * per_q * 8));
  FS_TRY(d_out_d.alloc((size_t)nq * ld * 4));
  FS_TRY(d_out_l.alloc((size_t)nq * ld * 8));
  FS_TRY(d_out_n.alloc((size_t)nq * 4));
  FS_TRY(upload(d_rows, io->rows, (size_t)io->n_rows * dp * esz));
  FS_TRY(upload(d_lab, io->labels, (size_t)io->n_rows * 8));
  FS_TRY(upload(d_q, io->queries, (size_t)nq * dp * 4));
  if (io->allow_bits) FS_TRY(upload(d_allow, io->allow_bits, allow_b));
  FS_TRY(upload(d_tn, io->tile_norm, (size_t)io->n_tiles * 4));
  FS_TRY(upload(d_coef, io->qcoef, (size_t)nq * 16));
  FS_TRY(upload(d_cnt, h_cnt.data(), (size_t)nq * 4));
  FS_TRY(upload(d_cand, h_cand.data(), h_cand.size() * 4));
  FS_TRY(upload(d_val, h_val.data(), h_val.size() * 4));
  FS_TRY(upload(d_spill, h_spill.data(), h_spill.size() * 4));
  FS_TRY(upload(d_spill_val, h_spill_val.data(), h_spill_val.size() * 4));
  FS_TRY(upload(d_chunk, qchunk.data(), qchunk.size() * 4));
  if (io->ovf_q) FS_TRY(upload(d_ovf, io->ovf_q, (size_t)nq * 4));
  else FS_TRY(hipMemset(d_ovf.p, 0, d_ovf.bytes));
  FS_TRY(hipMemset(d_zero.p, 0, d_zero.bytes));       // flat_qprep_kernel zeroes done_cnt and rerank_cnt, scan_filter redo_cnt
  for (const DevBuf *b : {&d_redo, &d_part_d, &d_part_l, &d_out_d, &d_out_l, &d_out_n}) FS_TRY(fill32(*b, io->fill));

  // flat_index.cc scan_filter, "3. exact re-rank of the survivors + selection": "FlatScanArgs r{};" to
  // "VK_HIP_TRY(launch_merge_topk(m, e, nq, s));" (nrp = 8 and per_q from "const uint32_t nrp = 8;" above it)
  const uint32_t nrp = 8;
  vk::FlatScanArgs r{};
  r.rows = d_rows.p;
  r.labels = d_lab.as<uint64_t>();
  r.queries = d_q.as<float>();
  r.allow_bits = io->allow_bits ? d_allow.as<uint64_t>() : nullptr;
  r.allow_nbits = io->allow_nbits;
  r.part_dist = d_part_d.as<float>();
  r.part_label = d_part_l.as<uint64_t>();
  r.row_stride_f = r.q_stride_f = dp;
  r.chunks = dp / 16;
  r.row_begin = 0;
  r.row_end = io->n_rows;
  r.nq = nq;
  r.k = k;
  r.nrp = nrp;
  r.nqg = nq;
  r.cand_cnt = d_cnt.as<uint32_t>();
  r.cand_row = d_cand.as<uint32_t>();
  r.cand_cap = cap;
  r.cand_qchunk = d_chunk.as<uint32_t>();
  r.cand_spill = d_spill.as<uint32_t>();
  r.cand_ovf = d_ovf.as<uint32_t>();
  if (!io->fused) FS_TRY(vk::launch_flat_scan(r, io->l2 != 0, io->bf16 != 0, 1, e, nullptr));
  vk::MergeArgs m{};
  m.in_dist = r.part_dist;
  m.in_label = r.part_label;
  m.part_stride = (uint64_t)nq * per_q;
  m.q_stride = per_q;
  m.parts = 1;
  m.per_part = per_q;
  m.k = k;
  m.out_ld = io->out_ld;
  m.out_dist = d_out_d.as<float>();
  m.out_label = d_out_l.as<uint64_t>();
  m.out_n = d_out_n.as<uint32_t>();
  m.ovf_q = d_ovf.as<uint32_t>();
  m.redo_cnt = d_zero.as<uint32_t>() + 2 * (size_t)nq;
  m.redo_list = d_redo.as<uint32_t>();
  if (io->fused) {
    r.cancel = nullptr;
    r.done_cnt = d_zero.as<uint32_t>();
    r.reranked = d_zero.as<uint32_t>() + nq;
    if (io->prune) {   // the second bound: from the survivors' own approximate scores
      r.cand_val = d_val.as<float>();
      r.cand_spill_val = d_spill_val.as<float>();
      r.qcoef = d_coef.as<float4>();
      r.tile_norm = d_tn.as<uint32_t>();
    }
    FS_TRY(vk::launch_flat_rerank(r, m, io->l2 != 0, io->bf16 != 0, nullptr));
  } else {
    FS_TRY(vk::launch_merge_topk(m, e, nq, nullptr));
  }
  FS_TRY(hipDeviceSynchronize());
  FS_TRY(download(io->out_dist, d_out_d, (size_t)nq * ld * 4));
  FS_TRY(download(io->out_label, d_out_l, (size_t)nq * ld * 8));
  FS_TRY(download(io->out_n, d_out_n, (size_t)nq * 4));
  FS_TRY(download(io->done_cnt, d_zero, (size_t)nq * 4));
  FS_TRY(hipMemcpy(io->reranked, d_zero.as<uint32_t>() + nq, (size_t)nq * 4, hipMemcpyDeviceToHost));
  FS_TRY(hipMemcpy(io->redo_cnt, d_zero.as<uint32_t>() + 2 * (size_t)nq, 4, hipMemcpyDeviceToHost));
  FS_TRY(download(io->redo_list, d_redo, (size_t)nq * 4));
  FS_TRY(download(io->part_dist, d_part_d, (size_t)nq * per_q * 4));
  FS_TRY(download(io->part_label, d_part_l, (size_t)nq * per_q * 8));
  memcpy(io->qchunk, qchunk.data(), qchunk.size() * 4);
  return 0;
}

// ---- K8 and the small kernels ----------------------------------------------------------------------------------------------------
// out [out_len >= n]: the pattern, then what launch_gather_distance wrote
int fs_probe_gather(const void *rows, uint32_t n_rows, uint32_t stride, uint32_t bf16, uint32_t l2, const float *query, const uint32_t *idx,
                    uint32_t n, uint32_t out_len, uint32_t fill, float *out) {
  if (n_rows == 0 || stride == 0 || stride % 64 != 0 || stride > 4096 || out_len < n) return 1;
  for (uint32_t i = 0; i < n; ++i)
    if (idx[i] >= n_rows) return 1;
  const size_t esz = bf16 ? 2 : 4;
  DevBuf d_rows, d_q, d_idx, d_out;
  FS_TRY(d_rows.alloc((size_t)n_rows * stride * esz));
  FS_TRY(d_q.alloc((size_t)stride * 4));
  FS_TRY(d_idx.alloc((size_t)n * 4));
  FS_TRY(d_out.alloc((size_t)out_len * 4));
  FS_TRY(upload(d_rows, rows, (size_t)n_rows * stride * esz));
  FS_TRY(upload(d_q, query, (size_t)stride * 4));
  FS_TRY(upload(d_idx, idx, (size_t)n * 4));
  FS_TRY(fill32(d_out, fill));
  vk::GatherArgs g{};
  g.rows = d_rows.p;
  g.query = d_q.as<float>();
  g.idx = d_idx.as<uint32_t>();
  g.out = d_out.as<float>();
  g.row_stride_f = stride;
  g.chunks = stride / 16;
  g.n = n;
  FS_TRY(vk::launch_gather_distance(g, l2 != 0, bf16 != 0, nullptr));
  FS_TRY(hipDeviceSynchronize());
  FS_TRY(download(out, d_out, (size_t)out_len * 4));
  return 0;
}

// out_dist [nq][k], out_n [nq] -> bound [2 * nq + 8]: the floats, the key words, and eight words the kernel does not own
int fs_probe_kth_bound(const float *out_dist, const uint32_t *out_n, uint32_t k, uint32_t nq, uint32_t fill, uint32_t *bound) {
  if (k == 0) return 1;
  DevBuf d_d, d_n, d_b;
  FS_TRY(d_d.alloc((size_t)nq * k * 4));
  FS_TRY(d_n.alloc((size_t)nq * 4));
  FS_TRY(d_b.alloc(((size_t)2 * nq + 8) * 4));
  FS_TRY(upload(d_d, out_dist, (size_t)nq * k * 4));
  FS_TRY(upload(d_n, out_n, (size_t)nq * 4));
  FS_TRY(fill32(d_b, fill));
  FS_TRY(vk::launch_kth_bound(d_d.as<float>(), d_n.as<uint32_t>(), k, nq, d_b.as<float>(), nullptr));
  FS_TRY(hipDeviceSynchronize());
  FS_TRY(download(bound, d_b, ((size_t)2 * nq + 8) * 4));
  return 0;
}

// out_dist / out_label [nq * k + 8], out_n [nq + 8] (with_n == 0: a null out_n is passed and the buffer keeps the pattern)
int fs_probe_fill_empty(uint32_t nq, uint32_t k, uint32_t with_n, uint32_t fill, float *out_dist, uint64_t *out_label, uint32_t *out_n) {
  const size_t total = (size_t)nq * k;
  DevBuf d_d, d_l, d_n;
  FS_TRY(d_d.alloc((total + 8) * 4));
  FS_TRY(d_l.alloc((total + 8) * 8));
  FS_TRY(d_n.alloc(((size_t)nq + 8) * 4));
  for (const DevBuf *b : {&d_d, &d_l, &d_n}) FS_TRY(fill32(*b, fill));
  FS_TRY(vk::launch_fill_empty(d_d.as<float>(), d_l.as<uint64_t>(), with_n ? d_n.as<uint32_t>() : nullptr, nq, k, nullptr));
  FS_TRY(hipDeviceSynchronize());
  FS_TRY(download(out_dist, d_d, (total + 8) * 4));
  FS_TRY(download(out_label, d_l, (total + 8) * 8));
  FS_TRY(download(out_n, d_n, ((size_t)nq + 8) * 4));
  return 0;
}

}  // extern "C"
