// filter_probe.hip -- TEST INFRASTRUCTURE (tests/test_flat_filter_stages_gpu.py), not part of libvkindex.so.
//
// The candidate filter (K4h, valkey-search_amd/csrc/flat_filter.hip) is reachable through the C ABI only end to end: six
// kernels between query and answer, and a lost neighbour says "the answer differs", not which of them lost it.  This probe
// includes that translation unit itself (compile with -I valkey-search_amd/csrc), so the product's kernels and launchers are
// what runs -- row_stats + tile cap, qprep, the sample pass, the bound selection, the early pass, the tighten step and the
// main pass -- on buffers the probe owns, each FILLED WITH A PATTERN THE CALLER CHOOSES before the first launch and handed
// back whole, so that a test can hold every stage against exact arithmetic and see every word a kernel did not write.
// Between the launches the host does what FlatIndex::scan_filter (csrc/flat_index.cc) does; the lines mirrored are named
// where they are repeated.  Each call launches each kernel once; a HIP error is the return code (the source line that saw
// it), nothing is retried.  Return codes: 0 ok, 1 refused arguments, 2 qprep left a counter unwritten (the passes, which would
// index memory with it, are not run), else the line of a HIP error.
#include "flat_filter.hip"

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

#define FP_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)

// every 32-bit word of the buffer = pattern (hipMemsetD32: whole words; all sizes here are multiples of 4)
hipError_t fill32(const DevBuf &b, uint32_t pattern) { return hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b.p), (int)pattern, b.bytes / 4); }

constexpr uint32_t kSlackRows = 256;   // RowStore::kRowSlack: readable rows past the capacity

}  // namespace

extern "C" {

// stage bits of FilterProbeCfg::stages
enum { kStQprep = 1, kStSample = 2, kStSelect = 4, kStEarly = 8, kStTighten = 16, kStMain = 32 };

struct FilterProbeCfg {
  uint32_t n_rows, stride, nq, k;            // stride = row_stride_f = q_stride_f: the padded dimension, a multiple of 64
  uint32_t bf16, l2, qbf16, dma, bdma, image;   // FlatFilterArgs' variant switches; image: rows16 is made and passed
  uint32_t fill;                             // the pattern every workspace word holds before the first launch
  uint32_t cap, n_chunks;                    // private list entries per query, spill chunks of the pool
  uint32_t sample_rows;                      // what filter_prepass_rows(k) stands for in scan_filter
  uint32_t blocks;                           // grid of the passes of mode 0 (scan_filter launches min(CUs, tiles): the caller keeps it <= tiles); the sample takes min(blocks, n_s)
  uint32_t early_tiles;                      // tiles per block of the early pass (kStEarly)
  uint32_t stages;                           // which launches run (kStQprep is required)
  uint32_t allow_nbits;                      // with allow_bits
};

// what scan_filter derives from (count, sample_rows): out = {n_s, gap, fine, groups, smax_ld, nqt, n_tiles, alloc_rows}
// (flat_index.cc, scan_filter: "uint64_t n_s = ..." to "const uint32_t smax_ld = ...")
int filter_probe_layout(const FilterProbeCfg *c, uint32_t *out) {
  if (c->n_rows < 128 || c->nq == 0 || c->sample_rows == 0) return 1;
  const uint64_t count = c->n_rows;
  uint64_t n_s = std::min<uint64_t>(std::max<uint64_t>(1, (uint64_t)c->sample_rows / 128), (uint64_t)vk::kFilterMaxGroups / 2);
  n_s = std::min<uint64_t>(n_s, count / 128);
  const uint32_t gap = (uint32_t)std::max<uint64_t>(1, count / (128 * n_s));
  const bool fine = n_s * 8 <= 4096;
  const uint32_t groups = (uint32_t)n_s * (fine ? 8 : 2);
  const uint32_t n_tiles = (uint32_t)((count + 127) / 128);
  out[0] = (uint32_t)n_s;
  out[1] = gap;
  out[2] = fine ? 1 : 0;
  out[3] = groups;
  out[4] = (groups + 63) & ~63u;
  out[5] = (c->nq + 31) / 32;
  out[6] = n_tiles;
  out[7] = n_tiles * 128 + kSlackRows;
  return 0;
}

// the index row behind local row i of sample tile `tile`: sample_row() of flat_filter.hip (a __device__ function) repeated
// for the host -- ((i / kR) * n_tiles + tile) * kR + i % kR) * gap, kR = 16 for bf16 rows, 8 for f32
uint64_t filter_probe_sample_row(uint32_t bf16, uint32_t n_s, uint32_t gap, uint32_t tile, uint32_t i) {
  const uint32_t kR = bf16 ? 16 : 8;
  return ((uint64_t)((i / kR) * n_s + tile) * kR + i % kR) * gap;
}

// the kernel symbol launch_flat_filter's `fn` ends at for these switches (its branches, in its order; product build)
const char *filter_probe_symbol(uint32_t bf16, uint32_t l2, uint32_t qbf16, uint32_t dma, uint32_t bdma, uint32_t image, uint32_t mode, uint32_t early) {
  const char *fn = bf16 ? (l2 ? "flat_filter_kernel<bf16,l2>" : "flat_filter_kernel<bf16,ip>") : (l2 ? "flat_filter_kernel<f32,l2>" : "flat_filter_kernel<f32,ip>");
  if (mode == 1) fn = bf16 ? (l2 ? "flat_filter_sample_kernel<bf16,l2>" : "flat_filter_sample_kernel<bf16,ip>")
                           : (l2 ? "flat_filter_sample_kernel<f32,l2>" : "flat_filter_sample_kernel<f32,ip>");
  if (qbf16) {
    if (!bf16 || l2) return "refused";
    fn = mode == 1 ? "flat_filter_bfmma_sample_kernel" : "flat_filter_bfmma_kernel";
    if (mode == 0 && dma) fn = early ? "flat_filter_early_bfmma_dma_kernel" : "flat_filter_bfmma_dma_kernel";
  }
  if (bdma && mode == 0 && !(qbf16 && dma)) {
    fn = qbf16 ? "flat_filter_bdma_kernel<bf16,ip,bfmma>"
         : bf16 ? (l2 ? "flat_filter_bdma_kernel<bf16,l2>" : "flat_filter_bdma_kernel<bf16,ip>")
                : (l2 ? "flat_filter_bdma_kernel<f32,l2>" : "flat_filter_bdma_kernel<f32,ip>");
    if (early)
      fn = qbf16 ? "flat_filter_early_kernel<bf16,ip,bfmma>"
           : bf16 ? (l2 ? "flat_filter_early_kernel<bf16,l2>" : "flat_filter_early_kernel<bf16,ip>")
                  : (l2 ? "flat_filter_early_kernel<f32,l2>" : "flat_filter_early_kernel<f32,ip>");
  }
  if (image && mode == 0) {
    if (bf16 || l2 || qbf16) return "refused";
    fn = early ? "flat_filter_early_kernel<f32,ip,image>" : "flat_filter_bdma_kernel<f32,ip,image>";
  }
  return fn;
}

// row_stats_kernel + tile_cap_kernel over rows [lo, hi) of a table of n_rows rows (alloc rows allocated, the rows behind
// n_rows holding the pattern).  tile_norm and stats start from ZERO, as ensure_row_stats (flat_index.cc) leaves them before
// a full pass -- they are accumulated with atomicMax, so zero is their contract; hn16 and rows16 start from the pattern and
// keep it wherever the kernel wrote nothing.  out_tile_norm [n_tiles + 2], out_stats [16], out_hn16 [alloc] (l2),
// out_rows16 [alloc][stride] (want_image).
int filter_probe_row_stats(const void *rows, uint32_t bf16, uint32_t l2, uint32_t stride, uint32_t n_rows, uint32_t lo, uint32_t hi,
                           uint32_t want_image, uint32_t fill, uint32_t *out_tile_norm, uint32_t *out_stats, uint32_t *out_hn16,
                           uint16_t *out_rows16) {
  if (n_rows == 0 || stride == 0 || stride % 64 != 0 || stride > 65536 || lo > hi || hi > n_rows) return 1;
  if (want_image && (bf16 || l2)) return 1;
  const uint32_t n_tiles = (n_rows + 127) / 128, alloc = n_tiles * 128 + kSlackRows;
  const size_t esz = bf16 ? 2 : 4, row_b = (size_t)stride * esz;
  DevBuf d_rows, d_tn, d_st, d_hn, d_img;
  FP_TRY(d_rows.alloc((size_t)alloc * row_b));
  FP_TRY(d_tn.alloc((size_t)(n_tiles + 2) * 4));
  FP_TRY(d_st.alloc(64));
  FP_TRY(d_hn.alloc((size_t)alloc * 4));
  FP_TRY(d_img.alloc(want_image ? (size_t)alloc * stride * 2 : 4));
  FP_TRY(fill32(d_rows, fill));
  FP_TRY(hipMemcpy(d_rows.p, rows, (size_t)n_rows * row_b, hipMemcpyHostToDevice));
  FP_TRY(hipMemset(d_tn.p, 0, d_tn.bytes));
  FP_TRY(hipMemset(d_st.p, 0, 64));
  FP_TRY(fill32(d_hn, fill));
  FP_TRY(fill32(d_img, fill));
  FP_TRY(vk::launch_row_stats(d_rows.p, bf16 != 0, l2 != 0, stride, lo, hi, n_tiles, d_st.as<uint32_t>(), d_tn.as<uint32_t>(),
                              l2 ? d_hn.as<uint32_t>() : nullptr, want_image ? d_img.p : nullptr, nullptr));
  FP_TRY(hipDeviceSynchronize());
  FP_TRY(hipMemcpy(out_tile_norm, d_tn.p, d_tn.bytes, hipMemcpyDeviceToHost));
  FP_TRY(hipMemcpy(out_stats, d_st.p, 64, hipMemcpyDeviceToHost));
  if (l2) FP_TRY(hipMemcpy(out_hn16, d_hn.p, d_hn.bytes, hipMemcpyDeviceToHost));
  if (want_image) FP_TRY(hipMemcpy(out_rows16, d_img.p, d_img.bytes, hipMemcpyDeviceToHost));
  return 0;
}

// host buffers of one chain run; every output is the device buffer copied back whole
struct FilterProbeIO {
  const void *rows;            // [n_rows][stride] f32, or bf16 as uint16
  const float *queries;        // [nq][stride]
  const uint64_t *labels;      // [n_rows]
  const uint64_t *allow_bits;  // [(allow_nbits + 63) / 64] or nullptr
  uint32_t *tile_norm;         // [n_tiles + 2]
  uint32_t *stats;             // [16]
  uint16_t *q16;               // [nqt * 32][stride] in fragment order
  float *thr;                  // scan_filter's d_fthr: [nqt * 32][4] qcoef | [nqt * 32] qbound | [nqt * 32] qwit
  uint32_t *words;             // scan_filter's d_fcnt: [nq] cand_cnt | [nq] ovf_q | [4] spill_next, redo_cnt | [nq] redo list | [nq][32] qchunk | [nq] done_cnt | [nq] rerank_cnt
  float *smax;                 // [nq][smax_ld]
  uint32_t *cand;              // scan_filter's d_fcand: [nq][cap] rows | [nq][cap] scores
  uint32_t *spill;             // scan_filter's d_fspill: [n_chunks][4096] rows | [n_chunks][4096] scores
  float *qbound_select;        // [nqt * 32] snapshot behind the bound selection (optional)
  uint32_t *cnt_early;         // [nq] cand_cnt behind the early pass (optional)
};

int filter_probe_chain(const FilterProbeCfg *c, const FilterProbeIO *io) {
  uint32_t lay[8];
  if (filter_probe_layout(c, lay) != 0) return 1;
  const uint32_t n_s = lay[0], gap = lay[1], fine = lay[2], groups = lay[3], smax_ld = lay[4], nqt = lay[5], n_tiles = lay[6], alloc = lay[7];
  const uint32_t dp = c->stride, nq = c->nq, cap = c->cap, n_chunks = c->n_chunks;
  if (dp == 0 || dp % 64 != 0 || dp > 4096 || nq > 2048 || c->k == 0 || c->k > 1024 || cap < 64 || cap > (1u << 20) || n_chunks > 256) return 1;
  if (c->blocks == 0 || c->blocks > 1024 || !(c->stages & kStQprep)) return 1;
  if (c->qbf16 && (!c->bf16 || c->l2)) return 1;
  if (c->dma && !c->qbf16) return 1;
  if (c->image && (c->bf16 || c->l2 || c->qbf16)) return 1;
  if ((c->stages & kStEarly) && c->early_tiles == 0) return 1;
  if ((io->allow_bits != nullptr) != (c->allow_nbits != 0)) return 1;
  if (!vk::flat_filter_supported(dp, c->k, c->bf16 != 0, c->l2 != 0)) return 1;
  // the sample's last row lies inside the index (sample_row: (127 n_s + n_s - 1) gap + ... < 128 n_s gap <= count)
  if ((uint64_t)128 * n_s * gap > c->n_rows) return 1;
  const size_t esz = c->bf16 ? 2 : 4, row_b = (size_t)dp * esz;
  // per-batch words, flat_index.cc scan_filter ("const size_t w_cnt = 0, w_ovf = nq, ...")
  const size_t w_cnt = 0, w_ovf = nq, w_misc = 2 * (size_t)nq, w_chunk = 3 * (size_t)nq + 4, w_done = w_chunk + (size_t)nq * vk::kSpillPerQuery;
  const size_t n_words = w_done + 2 * (size_t)nq;

  DevBuf d_rows, d_q, d_lab, d_allow, d_tn, d_st, d_hn, d_img, d_q16, d_thr, d_cnt, d_cand, d_spill, d_smax;
  FP_TRY(d_rows.alloc((size_t)alloc * row_b));
  FP_TRY(d_q.alloc((size_t)nq * dp * 4));
  FP_TRY(d_lab.alloc((size_t)alloc * 8));
  FP_TRY(d_allow.alloc(((size_t)c->allow_nbits + 63) / 64 * 8 + 8));
  FP_TRY(d_tn.alloc((size_t)(n_tiles + 2) * 4));
  FP_TRY(d_st.alloc(64));
  FP_TRY(d_hn.alloc((size_t)alloc * 4));
  FP_TRY(d_img.alloc(c->image ? (size_t)alloc * dp * 2 : 4));
  FP_TRY(d_q16.alloc((size_t)nqt * 32 * dp * 2));
  FP_TRY(d_thr.alloc((size_t)nqt * 32 * (16 + 4 + 4)));
  FP_TRY(d_cnt.alloc(n_words * 4));
  FP_TRY(d_cand.alloc((size_t)nq * cap * 8));
  FP_TRY(d_spill.alloc((size_t)n_chunks * vk::kSpillChunk * 8));
  FP_TRY(d_smax.alloc((size_t)nq * smax_ld * 4));
  // rows: the table, and behind it what an allocation may hold; labels behind the table as RowStore leaves them
  FP_TRY(fill32(d_rows, c->fill));
  FP_TRY(hipMemcpy(d_rows.p, io->rows, (size_t)c->n_rows * row_b, hipMemcpyHostToDevice));
  FP_TRY(hipMemcpy(d_q.p, io->queries, (size_t)nq * dp * 4, hipMemcpyHostToDevice));
  FP_TRY(hipMemset(d_lab.p, 0xFF, d_lab.bytes));
  FP_TRY(hipMemcpy(d_lab.p, io->labels, (size_t)c->n_rows * 8, hipMemcpyHostToDevice));
  FP_TRY(hipMemset(d_allow.p, 0, d_allow.bytes));
  if (io->allow_bits) FP_TRY(hipMemcpy(d_allow.p, io->allow_bits, ((size_t)c->allow_nbits + 63) / 64 * 8, hipMemcpyHostToDevice));
  // ensure_row_stats: tile norms and statistics from zero (their atomicMax contract); everything else holds the pattern
  FP_TRY(hipMemset(d_tn.p, 0, d_tn.bytes));
  FP_TRY(hipMemset(d_st.p, 0, 64));
  for (const DevBuf *b : {&d_hn, &d_img, &d_q16, &d_thr, &d_cnt, &d_cand, &d_spill, &d_smax}) FP_TRY(fill32(*b, c->fill));
  FP_TRY(vk::launch_row_stats(d_rows.p, c->bf16 != 0, c->l2 != 0, dp, 0, c->n_rows, n_tiles, d_st.as<uint32_t>(), d_tn.as<uint32_t>(),
                              c->l2 ? d_hn.as<uint32_t>() : nullptr, c->image ? d_img.p : nullptr, nullptr));
  FP_TRY(hipDeviceSynchronize());

  // flat_index.cc scan_filter, "FlatFilterArgs f{};" to "f.redo_cnt = redo_cnt;"
  uint32_t *words = d_cnt.as<uint32_t>();
  vk::FlatFilterArgs f{};
  f.rows = d_rows.p;
  f.bf16 = c->bf16 ? 1 : 0;
  f.l2 = c->l2 ? 1 : 0;
  f.qbf16 = c->qbf16 ? 1 : 0;
  f.dma = c->dma ? 1 : 0;
  f.bdma = c->bdma ? 1 : 0;
  f.hn16 = c->l2 ? d_hn.as<uint32_t>() : nullptr;
  f.rows16 = c->image ? d_img.p : nullptr;
  f.labels = d_lab.as<uint64_t>();
  f.allow_bits = io->allow_bits ? d_allow.as<uint64_t>() : nullptr;
  f.allow_nbits = c->allow_nbits;
  f.queries = d_q.as<float>();
  f.q_stride_f = dp;
  f.q16 = d_q16.p;
  f.qcoef = d_thr.as<float4>();
  f.qbound = reinterpret_cast<float *>(d_thr.as<char>() + (size_t)nqt * 32 * 16);
  f.qwit = f.qbound + (size_t)nqt * 32;
  f.norm_cap = d_st.as<uint32_t>() + 3;
  f.sample_gap = gap;
  f.tile_norm = d_tn.as<uint32_t>();
  f.cand_cnt = words + w_cnt;
  f.cand_row = d_cand.as<uint32_t>();
  f.cand_val = reinterpret_cast<float *>(f.cand_row + nq * (size_t)cap);
  f.cap = cap;
  f.qchunk = words + w_chunk;
  f.spill = d_spill.as<uint32_t>();
  f.spill_val = reinterpret_cast<float *>(f.spill + (size_t)n_chunks * vk::kSpillChunk);
  f.spill_next = words + w_misc;
  f.n_chunks = n_chunks;
  f.ovf_q = words + w_ovf;
  f.done_cnt = words + w_done;
  f.rerank_cnt = words + w_done + nq;
  f.smax = d_smax.as<float>();
  f.smax_ld = smax_ld;
  f.smax_fine = fine;
  f.row_stride_f = dp;
  f.n_rows = c->n_rows;
  f.nq = nq;
  f.nqt = nqt;
  f.cancel = nullptr;
  f.redo_cnt = words + w_misc + 1;
  FP_TRY(vk::launch_flat_qprep(f, nullptr));
  FP_TRY(hipDeviceSynchronize());
  const uint32_t later = c->stages & (kStSample | kStSelect | kStEarly | kStTighten | kStMain);
  bool counters_ok = true;
  if (later) {
    // the passes index memory with the counters qprep resets (list slots, chunk ids): over a pattern they must be zero first
    std::vector<uint32_t> h(n_words);
    FP_TRY(hipMemcpy(h.data(), words, n_words * 4, hipMemcpyDeviceToHost));
    bool ok = h[w_misc] == 0;
    for (size_t q = 0; q < nq && ok; ++q) ok = h[w_cnt + q] == 0;
    for (size_t i = 0; i < (size_t)nq * vk::kSpillPerQuery && ok; ++i) ok = h[w_chunk + i] == 0;
    counters_ok = ok;
  }
  if (later && counters_ok) {
    // scan_filter's filter_launches: one launch per 256 queries, every launch one pass over its tiles
    auto filter_launches = [&](const vk::FlatFilterArgs &base, uint32_t blocks) -> int {
      for (uint32_t g0 = 0; g0 < nqt; g0 += 8) {
        vk::FlatFilterArgs fg = base;
        const size_t c0 = (size_t)g0 * 32;
        fg.nqt = std::min<uint32_t>(8, nqt - g0);
        fg.nq = (uint32_t)std::min<uint64_t>(256, nq - c0);
        fg.q16 = static_cast<char *>(base.q16) + c0 * dp * 2;
        fg.qcoef = base.qcoef + c0;
        fg.qbound = base.qbound + c0;
        fg.qwit = base.qwit + c0;
        fg.cand_cnt = base.cand_cnt + c0;
        fg.cand_row = base.cand_row + c0 * cap;
        fg.cand_val = base.cand_val + c0 * cap;
        fg.qchunk = base.qchunk + c0 * vk::kSpillPerQuery;
        fg.ovf_q = base.ovf_q + c0;
        fg.done_cnt = base.done_cnt + c0;
        fg.rerank_cnt = base.rerank_cnt + c0;
        fg.smax = base.smax + c0 * smax_ld;
        FP_TRY(vk::launch_flat_filter(fg, blocks, nullptr));
      }
      return 0;
    };
    int rc;
    // scan_filter "1. the bound"
    if (c->stages & kStSample) {
      vk::FlatFilterArgs fs = f;
      fs.mode = 1;
      fs.n_tiles = n_s;
      fs.cancel = nullptr;
      if ((rc = filter_launches(fs, std::min<uint32_t>(c->blocks, n_s))) != 0) return rc;
      FP_TRY(hipDeviceSynchronize());
    }
    if (c->stages & kStSelect) {
      vk::FlatBoundArgs b{};
      b.smax = f.smax;
      b.smax_ld = smax_ld;
      b.groups = groups;
      b.k = c->k;
      b.nq = nq;
      b.qbound = f.qbound;
      FP_TRY(vk::launch_flat_bound_select(b, nullptr));
      FP_TRY(hipDeviceSynchronize());
      if (io->qbound_select) FP_TRY(hipMemcpy(io->qbound_select, f.qbound, (size_t)nqt * 32 * 4, hipMemcpyDeviceToHost));
    }
    // scan_filter "2. the filter over all rows"
    vk::FlatFilterArgs fm = f;
    fm.mode = 0;
    fm.n_tiles = n_tiles;
    if (c->stages & kStEarly) {
      vk::FlatFilterArgs fe = fm;
      fe.part_first = 0;
      fe.part_tiles = c->early_tiles;
      fe.early = 1;
      if ((rc = filter_launches(fe, c->blocks)) != 0) return rc;
      FP_TRY(hipDeviceSynchronize());
      if (io->cnt_early) FP_TRY(hipMemcpy(io->cnt_early, f.cand_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost));
    }
    if (c->stages & kStTighten) {
      vk::FlatTightenArgs t{};
      t.cand_cnt = f.cand_cnt;
      t.cand_row = f.cand_row;
      t.cand_val = f.cand_val;
      t.cap = cap;
      t.k = c->k;
      t.nq = nq;
      t.l2 = c->l2 ? 1u : 0u;
      t.qcoef = f.qcoef;
      t.tile_norm = f.tile_norm;
      t.qbound = f.qbound;
      FP_TRY(vk::launch_flat_bound_tighten(t, nullptr));
      FP_TRY(hipDeviceSynchronize());
    }
    if (c->stages & kStMain) {
      if (c->stages & kStEarly) {
        fm.part_first = c->early_tiles;
        fm.part_tiles = 0xFFFFFFFFu;
      }
      if ((rc = filter_launches(fm, c->blocks)) != 0) return rc;
      FP_TRY(hipDeviceSynchronize());
    }
  }
  {
    FP_TRY(hipMemcpy(io->tile_norm, d_tn.p, d_tn.bytes, hipMemcpyDeviceToHost));
    FP_TRY(hipMemcpy(io->stats, d_st.p, 64, hipMemcpyDeviceToHost));
    FP_TRY(hipMemcpy(io->q16, d_q16.p, d_q16.bytes, hipMemcpyDeviceToHost));
    FP_TRY(hipMemcpy(io->thr, d_thr.p, d_thr.bytes, hipMemcpyDeviceToHost));
    FP_TRY(hipMemcpy(io->words, d_cnt.p, n_words * 4, hipMemcpyDeviceToHost));
    FP_TRY(hipMemcpy(io->smax, d_smax.p, d_smax.bytes, hipMemcpyDeviceToHost));
    FP_TRY(hipMemcpy(io->cand, d_cand.p, d_cand.bytes, hipMemcpyDeviceToHost));
    if (n_chunks) FP_TRY(hipMemcpy(io->spill, d_spill.p, d_spill.bytes, hipMemcpyDeviceToHost));
  }
  return counters_ok ? 0 : 2;
}

}  // extern "C"
