// flat_scan_probe.hip -- TEST INFRASTRUCTURE (tests/test_flat_scan_kernels_gpu.py), not part of libvkindex.so.
//
// The two kernels that produce every exact FLAT answer -- flat_scan_kernel in its plain (non-list) mode (K3) and
// flat_gemm_kernel / flat_gemm_prepass_kernel (K4) -- are reachable through the C ABI only as "the answer of a search": the
// partition count, the query block, the tile walk, the lockstep window, the pre-pass bound, the redo mode and the paged scan are
// all derived from the index there, and what a kernel leaves in its partial lists is invisible behind the merge.  This probe
// includes both translation units themselves (compile with -I valkey-search_amd/csrc), so the product's kernels and launchers
// are what runs, on buffers the probe owns.  The rows are allocated as RowStore does (n_alloc + RowStore::kRowSlack rows) and
// the CALLER says what every one of them holds, the rows past n_rows included.  Every OUTPUT and WORKSPACE buffer (part_dist,
// part_label, K4's sync and qbound) is filled with a 32-bit pattern the caller passes before the launch -- except the words the
// product itself prepares first (flat_index.cc, FlatIndex::scan_gemm, "if (!handover) {" to the closing brace in front of
// "VK_HIP_TRY(launch_flat_gemm(g, s));": sync zeroed; qbound copied from init_bound + nq, or set to the key of +inf; a
// hand-over launch, run_flag != nullptr, prepares neither) -- and handed back whole, so that a test can hold every word
// against a model and see every word a kernel did not write.  cancel is one word of host-pinned memory holding the value the
// caller gives, set before the launch and not changed during it; run_flag is a device word with a caller-given value.  Each
// call launches each kernel once.  Return codes: 0 ok, 1 refused arguments, else the source line that saw a HIP error; nothing
// is retried.
#include "flat_scan.hip"
#include "flat_gemm.hip"
#include "row_store.hpp"

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
struct PinnedWord {   // host-pinned, mapped into the device's address space (as SearchCtx::arm_cancel's word)
  uint32_t *p = nullptr;
  ~PinnedWord() { (void)hipHostFree(p); }
  hipError_t alloc() { return hipHostMalloc(reinterpret_cast<void **>(&p), 64, hipHostMallocDefault); }
};

#define FS_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)

// every 32-bit word of the buffer = pattern (all sizes here are multiples of 4)
hipError_t fill32(const DevBuf &b, uint32_t pattern) { return hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b.p), (int)pattern, b.bytes / 4); }
hipError_t upload(const DevBuf &b, const void *src, size_t bytes) { return bytes ? hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) : hipSuccess; }
hipError_t download(void *dst, const DevBuf &b, size_t bytes) { return bytes ? hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }

}  // namespace

extern "C" {

// ---- what the host side of the product computes: taken from it, not restated ----------------------------------------------------
uint32_t fsc_row_slack() { return (uint32_t)vk::RowStore::kRowSlack; }
uint32_t fsc_gemm_tile_q(uint32_t row_stride_f) { return vk::flat_gemm_tile_q(row_stride_f); }
uint64_t fsc_gemm_lds_bytes(uint32_t row_stride_f, uint32_t tile_q) { return vk::flat_gemm_lds_bytes(row_stride_f, tile_q); }
uint32_t fsc_gemm_supported(uint32_t row_stride_f, uint64_t k) { return vk::flat_gemm_supported(row_stride_f, k) ? 1u : 0u; }
int fsc_scan_pick_qb(uint64_t nq, uint32_t chunks, int e, uint32_t l2) { return vk::flat_scan_pick_qb(nq, chunks, e, l2 != 0); }
int fsc_scan_slots_per_lane(uint64_t k) { return vk::flat_scan_slots_per_lane(k); }

// ---- K4 ------------------------------------------------------------------------------------------------------------------------
struct FscGemmIO {               // mirrors FlatGemmArgs
  const void *rows;              // [n_alloc + fsc_row_slack()][stride] f32, or bf16 as uint16: ALL of them, the caller's choice
  const uint64_t *labels;        // [n_alloc + fsc_row_slack()]
  const float *queries;          // [nq][stride] padded
  const uint64_t *allow_bits;    // optional [(allow_nbits + 63) / 64]
  uint64_t allow_nbits;
  const uint32_t *init_bound;    // optional [2 * nq]: the floats, then their keys (what kth_bound_kernel writes)
  uint32_t n_rows, n_alloc, stride, bf16, nq, k, nrp, tile_q, lockstep, contig, prepass;
  uint32_t cancel;               // the value of the host-pinned word
  uint32_t use_flag, flag_value, run_if, run_hi;   // use_flag: run_flag points at a device word holding flag_value (a hand-over launch)
  uint32_t fill;
  uint32_t *part_dist;           // [nq][nrp][8][k] f32 bits
  uint64_t *part_label;          // [nq][nrp][8][k]
  uint32_t *sync;                // [nrp][4][32]
  uint32_t *qbound;              // [nq]
};

int fsc_probe_gemm(const FscGemmIO *io) {
  const uint32_t nq = io->nq, dp = io->stride, k = io->k, nrp = io->nrp, tq = io->tile_q;
  if (nq == 0 || io->n_rows == 0 || io->n_alloc < io->n_rows || dp == 0 || !vk::flat_gemm_supported(dp, k)) return 1;
  if (nrp == 0 || (nrp & 7u) || (tq != 16 && tq != 24 && tq != 32) || vk::flat_gemm_lds_bytes(dp, tq) > 160 * 1024) return 1;
  const uint32_t nqt = (nq + tq - 1) / tq;
  if (io->lockstep && nqt > 32) return 1;             // a wave's progress words: 32 per (partition, wave)
  if ((io->allow_bits != nullptr) != (io->allow_nbits != 0)) return 1;
  // the hand-over launch of the product: k <= 10, no lockstep window, no pre-pass bound (scan_gemm: "const bool handover")
  if (io->use_flag && (k > 10 || io->lockstep || io->init_bound)) return 1;
  // the rows a block reads: whole tiles of 128 from its first tile on, never past the last tile of the index
  const uint64_t n_total = (uint64_t)io->n_alloc + vk::RowStore::kRowSlack;
  if (((uint64_t)io->n_rows + 127) / 128 * 128 > n_total) return 1;
  const size_t esz = io->bf16 ? 2 : 4;
  const size_t allow_b = ((size_t)io->allow_nbits + 63) / 64 * 8;
  const size_t lists = (size_t)nq * nrp * 8 * k, sync_words = (size_t)nrp * 4 * 32;
  DevBuf d_rows, d_lab, d_q, d_allow, d_bound, d_flag, d_part_d, d_part_l, d_sync;
  PinnedWord cancel;
  FS_TRY(d_rows.alloc(n_total * dp * esz));
  FS_TRY(d_lab.alloc(n_total * 8));
  FS_TRY(d_q.alloc((size_t)nq * dp * 4));
  FS_TRY(d_allow.alloc(allow_b));
  FS_TRY(d_bound.alloc((size_t)2 * nq * 4));
  FS_TRY(d_flag.alloc(4));
  FS_TRY(d_part_d.alloc(lists * 4));
  FS_TRY(d_part_l.alloc(lists * 8));
  FS_TRY(d_sync.alloc((sync_words + nq) * 4));        // [ progress words | per-query bounds ], as scan_gemm lays them out
  FS_TRY(cancel.alloc());
  FS_TRY(upload(d_rows, io->rows, n_total * dp * esz));
  FS_TRY(upload(d_lab, io->labels, n_total * 8));
  FS_TRY(upload(d_q, io->queries, (size_t)nq * dp * 4));
  if (io->allow_bits) FS_TRY(upload(d_allow, io->allow_bits, allow_b));
  if (io->init_bound) FS_TRY(upload(d_bound, io->init_bound, (size_t)2 * nq * 4));
  FS_TRY(upload(d_flag, &io->flag_value, 4));
  for (const DevBuf *b : {&d_part_d, &d_part_l, &d_sync}) FS_TRY(fill32(*b, io->fill));
  *cancel.p = io->cancel;

  vk::FlatGemmArgs g{};
  g.init_bound = io->init_bound ? d_bound.as<float>() : nullptr;
  g.prepass = io->prepass ? 1 : 0;
  g.rows = d_rows.p;
  g.bf16 = io->bf16 ? 1 : 0;
  g.labels = d_lab.as<uint64_t>();
  g.queries = d_q.as<float>();
  g.allow_bits = io->allow_bits ? d_allow.as<uint64_t>() : nullptr;
  g.allow_nbits = io->allow_nbits;
  g.row_stride_f = g.q_stride_f = dp;
  g.chunks = dp / 16;
  g.n_rows = io->n_rows;
  g.nq = nq;
  g.k = k;
  g.tile_q = tq;
  g.nqt = nqt;
  g.nrp = nrp;
  g.part_dist = d_part_d.as<float>();
  g.part_label = d_part_l.as<uint64_t>();
  g.lockstep = io->lockstep;
  g.contig = io->contig ? 1 : 0;
  g.cancel = cancel.p;
  if (io->use_flag) {
    g.run_flag = d_flag.as<uint32_t>();
    g.run_if = io->run_if;
    g.run_hi = io->run_hi;
  }
  g.sync = d_sync.as<uint32_t>();
  g.qbound = g.sync + sync_words;
  // flat_index.cc, FlatIndex::scan_gemm: "if (!handover) {   // (the hand-over launch neither waits on the progress words nor
  // reads the shared bound)" -- hipMemsetAsync(g.sync, 0, ..), then hipMemcpyAsync(g.qbound, init_bound + nq, ..) or
  // hipMemsetD32Async(g.qbound, 0xFF800000, ..)
  if (!io->use_flag) {
    FS_TRY(hipMemset(g.sync, 0, sync_words * 4));
    if (io->init_bound) FS_TRY(hipMemcpy(g.qbound, d_bound.as<uint32_t>() + nq, (size_t)nq * 4, hipMemcpyDeviceToDevice));
    else FS_TRY(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(g.qbound), (int)0xFF800000u, nq));
  }
  FS_TRY(vk::launch_flat_gemm(g, nullptr));
  FS_TRY(hipDeviceSynchronize());
  FS_TRY(download(io->part_dist, d_part_d, lists * 4));
  FS_TRY(download(io->part_label, d_part_l, lists * 8));
  FS_TRY(hipMemcpy(io->sync, g.sync, sync_words * 4, hipMemcpyDeviceToHost));
  FS_TRY(hipMemcpy(io->qbound, g.qbound, (size_t)nq * 4, hipMemcpyDeviceToHost));
  return 0;
}

// ---- K3, plain mode ------------------------------------------------------------------------------------------------------------
struct FscScanIO {               // mirrors FlatScanArgs without the survivor lists (cand_row stays null)
  const void *rows;              // [n_alloc + fsc_row_slack()][stride]
  const uint64_t *labels;        // [n_alloc + fsc_row_slack()]
  const float *queries;          // [nq][stride] padded
  const uint64_t *allow_bits;
  uint64_t allow_nbits;
  const float *lb_dist;          // optional [nq], with lb_label: the paged scan
  const uint64_t *lb_label;
  const uint32_t *q_index;       // optional [nq]: redo mode, with nq_dev
  uint32_t n_alloc, stride, bf16, l2, qb, e, row_begin, row_end, nq, k, nrp;
  uint32_t nq_dev;               // redo mode: the device word holds it
  uint32_t use_cancel, cancel;   // use_cancel: the kernel gets the host-pinned word, holding `cancel`
  // use_flag 1: run_flag points at a device word holding flag_value; 2: at the nq_dev word itself, as scan_k3 passes it
  uint32_t use_flag, flag_value, run_if, run_hi;
  uint32_t fill;
  uint32_t *part_dist;           // [nq][nrp * (e == 1 ? 1 : 4)][k] f32 bits
  uint64_t *part_label;
};

int fsc_probe_scan(const FscScanIO *io) {
  const uint32_t nq = io->nq, dp = io->stride, k = io->k, nrp = io->nrp;
  const int qb = (int)io->qb, e = (int)io->e;
  if (nq == 0 || dp == 0 || dp % 64 != 0 || dp > 4096 || k == 0) return 1;
  if ((qb != 1 && qb != 2 && qb != 4 && qb != 8) || (e != 1 && e != 4 && e != 16) || k > 64u * (uint32_t)e) return 1;
  if ((e == 4 && qb > 2) || (e == 16 && qb > 1)) return 1;     // flat_scan_pick_qb never asks for these
  if (nrp == 0 || (nrp & 7u)) return 1;
  if (io->row_begin >= io->row_end || io->row_end > io->n_alloc) return 1;
  if ((io->allow_bits != nullptr) != (io->allow_nbits != 0)) return 1;
  if ((io->lb_dist != nullptr) != (io->lb_label != nullptr)) return 1;
  if (io->lb_dist && (e != 16 || qb != 1 || io->q_index)) return 1;
  if (io->q_index) {
    if (io->nq_dev > nq) return 1;
    for (uint32_t i = 0; i < nq; ++i)
      if (io->q_index[i] >= nq) return 1;
  }
  if (io->use_flag == 2 && !io->q_index) return 1;
  const uint64_t n_total = (uint64_t)io->n_alloc + vk::RowStore::kRowSlack;
  const size_t esz = io->bf16 ? 2 : 4;
  const size_t allow_b = ((size_t)io->allow_nbits + 63) / 64 * 8;
  const size_t lists = (size_t)nq * nrp * (e == 1 ? 1 : 4) * k;
  DevBuf d_rows, d_lab, d_q, d_allow, d_lbd, d_lbl, d_qi, d_words, d_part_d, d_part_l;
  PinnedWord cancel;
  FS_TRY(d_rows.alloc(n_total * dp * esz));
  FS_TRY(d_lab.alloc(n_total * 8));
  FS_TRY(d_q.alloc((size_t)nq * dp * 4));
  FS_TRY(d_allow.alloc(allow_b));
  FS_TRY(d_lbd.alloc((size_t)nq * 4));
  FS_TRY(d_lbl.alloc((size_t)nq * 8));
  FS_TRY(d_qi.alloc((size_t)nq * 4));
  FS_TRY(d_words.alloc(8));                           // nq_dev | run flag
  FS_TRY(d_part_d.alloc(lists * 4));
  FS_TRY(d_part_l.alloc(lists * 8));
  FS_TRY(cancel.alloc());
  FS_TRY(upload(d_rows, io->rows, n_total * dp * esz));
  FS_TRY(upload(d_lab, io->labels, n_total * 8));
  FS_TRY(upload(d_q, io->queries, (size_t)nq * dp * 4));
  if (io->allow_bits) FS_TRY(upload(d_allow, io->allow_bits, allow_b));
  if (io->lb_dist) {
    FS_TRY(upload(d_lbd, io->lb_dist, (size_t)nq * 4));
    FS_TRY(upload(d_lbl, io->lb_label, (size_t)nq * 8));
  }
  if (io->q_index) FS_TRY(upload(d_qi, io->q_index, (size_t)nq * 4));
  const uint32_t words[2] = {io->nq_dev, io->flag_value};
  FS_TRY(upload(d_words, words, 8));
  for (const DevBuf *b : {&d_part_d, &d_part_l}) FS_TRY(fill32(*b, io->fill));
  *cancel.p = io->cancel;

  // flat_index.cc, FlatIndex::scan_k3: "FlatScanArgs a{};" to "VK_HIP_TRY(launch_flat_scan(a, l2(), store_.bf16(), qb, e, s));"
  vk::FlatScanArgs a{};
  a.rows = d_rows.p;
  a.labels = d_lab.as<uint64_t>();
  a.queries = d_q.as<float>();
  a.allow_bits = io->allow_bits ? d_allow.as<uint64_t>() : nullptr;
  a.allow_nbits = io->allow_nbits;
  a.lb_dist = io->lb_dist ? d_lbd.as<float>() : nullptr;
  a.lb_label = io->lb_dist ? d_lbl.as<uint64_t>() : nullptr;
  a.part_dist = d_part_d.as<float>();
  a.part_label = d_part_l.as<uint64_t>();
  a.row_stride_f = a.q_stride_f = dp;
  a.chunks = dp / 16;
  a.row_begin = io->row_begin;
  a.row_end = io->row_end;
  a.nq = nq;
  a.k = k;
  a.nrp = nrp;
  a.nqg = (nq + (uint32_t)qb - 1) / (uint32_t)qb;
  a.cancel = io->use_cancel ? cancel.p : nullptr;
  if (io->use_flag) {
    a.run_flag = io->use_flag == 2 ? d_words.as<uint32_t>() : d_words.as<uint32_t>() + 1;
    a.run_if = io->run_if;
    a.run_hi = io->run_hi;
  }
  if (io->q_index) {
    a.q_index = d_qi.as<uint32_t>();
    a.nq_dev = d_words.as<uint32_t>();
  }
  FS_TRY(vk::launch_flat_scan(a, io->l2 != 0, io->bf16 != 0, qb, e, nullptr));
  FS_TRY(hipDeviceSynchronize());
  FS_TRY(download(io->part_dist, d_part_d, lists * 4));
  FS_TRY(download(io->part_label, d_part_l, lists * 8));
  return 0;
}

}  // extern "C"
