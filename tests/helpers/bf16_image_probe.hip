// bf16_image_probe.hip -- TEST INFRASTRUCTURE (tests/test_flat_bf16_image_gpu.py), not part of libvkindex.so.
//
// The 16-bit image of an f32 index's rows in either number format (option flat-image-format) and the filter passes over it,
// on buffers the probe owns.  This file includes valkey-search_amd/csrc/flat_filter.hip itself (compile with -I
// valkey-search_amd/csrc and the library's flags), so the product's kernels and launchers are what runs:
//   bi_probe_image   row_stats_kernel over rows [lo, hi) with the image written as f16 or bf16, the image buffer pre-filled with
//                    a pattern the caller chooses and handed back whole
//   bi_probe_chain   row stats + image, qprep, sample, bound selection, early pass, tighten, main pass -- the launches of
//                    FlatIndex::scan_filter (csrc/flat_index.cc) with the arguments it builds for an f32 index behind an image
//                    of that format -- every buffer handed back, so that a test can hold each stage against float64
// Each call launches each kernel once.  Nothing blocks on a launch: the host polls the stream, and gives up after kWaitMs
// (return code 3).  Return codes: 0 ok, 1 refused arguments, 3 time limit, else the source line that saw a HIP error.
#include "flat_filter.hip"

#include <algorithm>
#include <chrono>
#include <thread>

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

#define BI_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)
#define BI_WAIT() do { const int w_ = wait_stream(); if (w_ != 0) return w_ == 3 ? 3 : __LINE__; } while (0)

hipError_t fill32(const DevBuf &b, uint32_t pattern) { return hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b.p), (int)pattern, b.bytes / 4); }

constexpr uint32_t kSlackRows = 256;   // RowStore::kRowSlack: readable rows past the capacity
constexpr int kWaitMs = 20000;

// 0 = the null stream is idle, 3 = still busy after kWaitMs, 1 = a HIP error
int wait_stream() {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipStreamQuery(nullptr);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotReady) return 1;
    if (std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count() > kWaitMs) return 3;
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

}  // namespace

extern "C" {

// out_tile_norm [n_tiles + 2], out_stats [16], out_img [alloc = n_tiles * 128 + 256][stride] 16-bit words.  tile_norm and stats
// start from zero (their atomicMax contract, FlatIndex::ensure_row_stats); the image starts from `fill`.
int bi_probe_image(const float *rows, uint32_t stride, uint32_t n_rows, uint32_t lo, uint32_t hi, uint32_t format, uint32_t fill,
                   uint32_t *out_tile_norm, uint32_t *out_stats, uint16_t *out_img) {
  if (n_rows == 0 || stride == 0 || stride % 64 != 0 || stride > 65536 || lo > hi || hi > n_rows || format > 1) return 1;
  const uint32_t n_tiles = (n_rows + 127) / 128, alloc = n_tiles * 128 + kSlackRows;
  DevBuf d_rows, d_tn, d_st, d_img;
  BI_TRY(d_rows.alloc((size_t)alloc * stride * 4));
  BI_TRY(d_tn.alloc((size_t)(n_tiles + 2) * 4));
  BI_TRY(d_st.alloc(64));
  BI_TRY(d_img.alloc((size_t)alloc * stride * 2));
  BI_TRY(fill32(d_rows, fill));
  BI_TRY(hipMemcpy(d_rows.p, rows, (size_t)n_rows * stride * 4, hipMemcpyHostToDevice));
  BI_TRY(hipMemset(d_tn.p, 0, d_tn.bytes));
  BI_TRY(hipMemset(d_st.p, 0, 64));
  BI_TRY(fill32(d_img, fill));
  BI_TRY(vk::launch_row_stats(d_rows.p, false, false, stride, lo, hi, n_tiles, d_st.as<uint32_t>(), d_tn.as<uint32_t>(), nullptr, d_img.p, nullptr,
                              format));
  BI_WAIT();
  BI_TRY(hipMemcpy(out_tile_norm, d_tn.p, d_tn.bytes, hipMemcpyDeviceToHost));
  BI_TRY(hipMemcpy(out_stats, d_st.p, 64, hipMemcpyDeviceToHost));
  BI_TRY(hipMemcpy(out_img, d_img.p, d_img.bytes, hipMemcpyDeviceToHost));
  return 0;
}

struct BiCfg {
  uint32_t n_rows, stride, nq, k;   // stride = row_stride_f = q_stride_f: the padded dimension, a multiple of 64
  uint32_t format;                  // 0 = f16 image, 1 = bf16 image
  uint32_t mfma16;                  // FlatFilterArgs::mfma16
  uint32_t cap;                     // private list entries per query (>= n_rows: nothing spills)
  uint32_t sample_rows;             // what filter_prepass_rows(k) stands for in scan_filter
  uint32_t blocks;                  // grid of the passes of mode 0 (<= tiles)
  uint32_t early_tiles;             // tiles per block of the early pass (0 = one pass, no tighten)
  uint32_t fill;                    // the pattern every workspace word holds before the first launch
};

struct BiIO {
  const float *rows;        // [n_rows][stride]
  const float *queries;     // [nq][stride]
  uint32_t *tile_norm;      // [n_tiles + 2]
  uint32_t *stats;          // [16]
  float *thr;               // [nqt * 32][4] qcoef | [nqt * 32] qbound (final) | [nqt * 32] qwit
  float *qbound_select;     // [nqt * 32] behind the bound selection
  float *smax;              // [nq][smax_ld]
  uint32_t *cnt;            // [nq] cand_cnt | [nq] ovf_q | [2] spill_next, redo_cnt
  uint32_t *cand;           // [nq][cap] rows | [nq][cap] scores
  uint32_t *layout;         // [6] n_s, gap, fine, groups, smax_ld, nqt
};

int bi_probe_chain(const BiCfg *c, const BiIO *io) {
  const uint32_t dp = c->stride, nq = c->nq, cap = c->cap;
  if (c->n_rows < 128 || nq == 0 || nq > 256 || dp == 0 || dp % 64 != 0 || dp > 4096 || c->k == 0 || c->k > 64 || c->format > 1) return 1;
  if (cap < c->n_rows || cap > (1u << 16) || c->blocks == 0 || c->sample_rows == 0) return 1;
  // flat_index.cc scan_filter, "uint64_t n_s = ..." to "const uint32_t smax_ld = ..."
  const uint64_t count = c->n_rows;
  uint64_t n_s = std::min<uint64_t>(std::max<uint64_t>(1, (uint64_t)c->sample_rows / 128), (uint64_t)vk::kFilterMaxGroups / 2);
  n_s = std::min<uint64_t>(n_s, count / 128);
  const uint32_t gap = (uint32_t)std::max<uint64_t>(1, count / (128 * n_s));
  const bool fine = n_s * 8 <= 4096;
  const uint32_t groups = (uint32_t)n_s * (fine ? 8 : 2), smax_ld = (groups + 63) & ~63u;
  const uint32_t nqt = (nq + 31) / 32, n_tiles = (uint32_t)((count + 127) / 128), alloc = n_tiles * 128 + kSlackRows;
  if (c->blocks > n_tiles || (uint64_t)128 * n_s * gap > count) return 1;
  if (c->early_tiles != 0 && c->early_tiles >= n_tiles / c->blocks) return 1;
  const uint32_t lay[6] = {(uint32_t)n_s, gap, fine ? 1u : 0u, groups, smax_ld, nqt};
  for (int i = 0; i < 6; ++i) io->layout[i] = lay[i];
  const size_t w_ovf = nq, w_misc = 2 * (size_t)nq, w_chunk = 3 * (size_t)nq + 4, w_done = w_chunk + (size_t)nq * vk::kSpillPerQuery;
  const size_t n_words = w_done + 2 * (size_t)nq;

  DevBuf d_rows, d_q, d_lab, d_tn, d_st, d_img, d_q16, d_thr, d_cnt, d_cand, d_spill, d_smax;
  BI_TRY(d_rows.alloc((size_t)alloc * dp * 4));
  BI_TRY(d_q.alloc((size_t)nq * dp * 4));
  BI_TRY(d_lab.alloc((size_t)alloc * 8));
  BI_TRY(d_tn.alloc((size_t)(n_tiles + 2) * 4));
  BI_TRY(d_st.alloc(64));
  BI_TRY(d_img.alloc((size_t)alloc * dp * 2));
  BI_TRY(d_q16.alloc((size_t)nqt * 32 * dp * 2));
  BI_TRY(d_thr.alloc((size_t)nqt * 32 * (16 + 4 + 4)));
  BI_TRY(d_cnt.alloc(n_words * 4));
  BI_TRY(d_cand.alloc((size_t)nq * cap * 8));
  BI_TRY(d_spill.alloc(8));
  BI_TRY(d_smax.alloc((size_t)nq * smax_ld * 4));
  BI_TRY(fill32(d_rows, c->fill));
  BI_TRY(hipMemcpy(d_rows.p, io->rows, (size_t)c->n_rows * dp * 4, hipMemcpyHostToDevice));
  BI_TRY(hipMemcpy(d_q.p, io->queries, (size_t)nq * dp * 4, hipMemcpyHostToDevice));
  BI_TRY(hipMemset(d_lab.p, 0, d_lab.bytes));
  BI_TRY(hipMemset(d_tn.p, 0, d_tn.bytes));
  BI_TRY(hipMemset(d_st.p, 0, 64));
  for (const DevBuf *b : {&d_img, &d_q16, &d_thr, &d_cnt, &d_cand, &d_smax}) BI_TRY(fill32(*b, c->fill));
  BI_TRY(vk::launch_row_stats(d_rows.p, false, false, dp, 0, c->n_rows, n_tiles, d_st.as<uint32_t>(), d_tn.as<uint32_t>(), nullptr, d_img.p, nullptr,
                              c->format));
  BI_WAIT();

  // flat_index.cc scan_filter, "FlatFilterArgs f{};" to "f.redo_cnt = redo_cnt;" for f32 rows behind a current image
  uint32_t *words = d_cnt.as<uint32_t>();
  vk::FlatFilterArgs f{};
  f.rows = d_rows.p;
  f.rows16 = d_img.p;
  f.bdma = 1;
  f.mfma16 = c->mfma16 ? 1u : 0u;
  if (c->format == vk::kImageBf16) {   // "a bf16 image ..."
    f.rows = f.rows16;
    f.rows16 = nullptr;
    f.bf16 = f.qbf16 = f.dma = f.img_bf16 = 1;
  }
  f.labels = d_lab.as<uint64_t>();
  f.queries = d_q.as<float>();
  f.q_stride_f = dp;
  f.q16 = d_q16.p;
  f.qcoef = d_thr.as<float4>();
  f.qbound = reinterpret_cast<float *>(d_thr.as<char>() + (size_t)nqt * 32 * 16);
  f.qwit = f.qbound + (size_t)nqt * 32;
  f.norm_cap = d_st.as<uint32_t>() + 3;
  f.sample_gap = gap;
  f.tile_norm = d_tn.as<uint32_t>();
  f.cand_cnt = words;
  f.cand_row = d_cand.as<uint32_t>();
  f.cand_val = reinterpret_cast<float *>(f.cand_row + nq * (size_t)cap);
  f.cap = cap;
  f.qchunk = words + w_chunk;
  f.spill = d_spill.as<uint32_t>();
  f.spill_val = reinterpret_cast<float *>(f.spill) + 1;
  f.spill_next = words + w_misc;
  f.n_chunks = 0;
  f.ovf_q = words + w_ovf;
  f.done_cnt = words + w_done;
  f.rerank_cnt = words + w_done + nq;
  f.smax = d_smax.as<float>();
  f.smax_ld = smax_ld;
  f.smax_fine = fine ? 1 : 0;
  f.row_stride_f = dp;
  f.n_rows = c->n_rows;
  f.nq = nq;
  f.nqt = nqt;
  f.redo_cnt = words + w_misc + 1;
  BI_TRY(vk::launch_flat_qprep(f, nullptr));
  BI_WAIT();
  {
    vk::FlatFilterArgs fs = f;
    fs.mode = 1;
    fs.n_tiles = (uint32_t)n_s;
    BI_TRY(vk::launch_flat_filter(fs, (uint32_t)std::min<uint64_t>(c->blocks, n_s), nullptr));
    BI_WAIT();
    vk::FlatBoundArgs b{};
    b.smax = f.smax;
    b.smax_ld = smax_ld;
    b.groups = groups;
    b.k = c->k;
    b.nq = nq;
    b.qbound = f.qbound;
    BI_TRY(vk::launch_flat_bound_select(b, nullptr));
    BI_WAIT();
    BI_TRY(hipMemcpy(io->qbound_select, f.qbound, (size_t)nqt * 32 * 4, hipMemcpyDeviceToHost));
  }
  vk::FlatFilterArgs fm = f;
  fm.mode = 0;
  fm.n_tiles = n_tiles;
  if (c->early_tiles != 0) {
    vk::FlatFilterArgs fe = fm;
    fe.part_first = 0;
    fe.part_tiles = c->early_tiles;
    fe.early = 1;
    BI_TRY(vk::launch_flat_filter(fe, c->blocks, nullptr));
    BI_WAIT();
    vk::FlatTightenArgs t{};
    t.cand_cnt = f.cand_cnt;
    t.cand_row = f.cand_row;
    t.cand_val = f.cand_val;
    t.cap = cap;
    t.k = c->k;
    t.nq = nq;
    t.l2 = 0;
    t.qcoef = f.qcoef;
    t.tile_norm = f.tile_norm;
    t.qbound = f.qbound;
    BI_TRY(vk::launch_flat_bound_tighten(t, nullptr));
    BI_WAIT();
    fm.part_first = c->early_tiles;
    fm.part_tiles = 0xFFFFFFFFu;
  }
  BI_TRY(vk::launch_flat_filter(fm, c->blocks, nullptr));
  BI_WAIT();
  BI_TRY(hipMemcpy(io->tile_norm, d_tn.p, d_tn.bytes, hipMemcpyDeviceToHost));
  BI_TRY(hipMemcpy(io->stats, d_st.p, 64, hipMemcpyDeviceToHost));
  BI_TRY(hipMemcpy(io->thr, d_thr.p, d_thr.bytes, hipMemcpyDeviceToHost));
  BI_TRY(hipMemcpy(io->smax, d_smax.p, d_smax.bytes, hipMemcpyDeviceToHost));
  BI_TRY(hipMemcpy(io->cnt, d_cnt.p, (2 * (size_t)nq + 2) * 4, hipMemcpyDeviceToHost));
  BI_TRY(hipMemcpy(io->cand, d_cand.p, d_cand.bytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
