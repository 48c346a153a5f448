// filter_shape_probe.hip -- TEST INFRASTRUCTURE (tests/test_flat_filter_mfma_shape_gpu.py), not part of libvkindex.so.
//
// The final pass of the candidate filter (K4h, valkey-search_amd/csrc/flat_filter.hip) with either matrix-core shape
// (FlatFilterArgs::mfma16), alone: flat_qprep_kernel and then one launch of mode 0 -- or two, the early and the main part of a
// split walk -- on buffers the CALLER fills (rows, the f16 image, tile norms, bounds, labels, allow bits) and gets back whole
// (counts, survivor lists, scores, coefficients), so that a test can hold every (query, row) pair a kernel stored against exact
// arithmetic.  Like filter_probe.hip this includes the product's translation unit (compile with -I valkey-search_amd/csrc):
// the product's kernels and launcher are what runs.  Return codes: 0 ok, 1 refused arguments, else the line of a HIP error.
#include "flat_filter.hip"

#include <vector>

namespace vk {
hipError_t ensure_max_lds(const void *fn) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
}  // namespace vk

namespace {
struct DevBuf {   // freed on every way out
  void *p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { (void)hipFree(p); }
  hipError_t alloc(size_t b) { bytes = b ? (b + 3) / 4 * 4 : 4; return hipMalloc(&p, bytes); }
  template <class T> T *as() const { return static_cast<T *>(p); }
};
#define SP_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)
hipError_t fill32(const DevBuf &b, uint32_t pattern) { return hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(b.p), (int)pattern, b.bytes / 4); }
constexpr uint32_t kSlackRows = 256;   // RowStore::kRowSlack: readable rows past the capacity
}  // namespace

extern "C" {

enum { kVarF32Image = 0, kVarF32Reg = 1, kVarBf16Dma = 2 };

struct ShapeProbeCfg {
  uint32_t n_rows, stride, nq;       // stride = row_stride_f = q_stride_f: the padded dimension, a multiple of 64
  uint32_t variant;                  // kVarF32Image: f32 rows + their f16 image; kVarF32Reg: f32 rows through registers, B by DMA; kVarBf16Dma: bf16 rows by DMA
  uint32_t mfma16;                   // FlatFilterArgs::mfma16
  uint32_t blocks;                   // grid of the launch(es)
  uint32_t early_tiles;              // != 0: two launches -- the first early_tiles tiles of every block's range, then what is behind them
  uint32_t cap;                      // private list entries per query
  uint32_t allow_nbits;              // with allow_bits
  uint32_t fill;                     // the pattern of every word the caller does not supply (rows behind n_rows among them)
};

struct ShapeProbeIO {
  const void *rows;            // [n_rows][stride] f32, or (kVarBf16Dma) bf16 as uint16
  const uint16_t *rows16;      // [n_rows][stride] f16 bits (kVarF32Image)
  const float *queries;        // [nq][stride]
  const uint64_t *labels;      // [n_rows]
  const uint64_t *allow_bits;  // [(allow_nbits + 63) / 64] or nullptr
  const uint32_t *tile_norm;   // [n_tiles] f32 bits
  const float *qbound;         // [nq]
  uint32_t *cand_cnt;          // out [nq]
  uint32_t *ovf_q;             // out [nq]
  uint32_t *cand_row;          // out [nq][cap]
  float *cand_val;             // out [nq][cap]
  float *qcoef;                // out [nqt * 32][4]
  uint32_t *cnt_early;         // out [nq]: cand_cnt behind the early launch (early_tiles != 0; optional)
};

int filter_shape_probe_run(const ShapeProbeCfg *c, const ShapeProbeIO *io) {
  const uint32_t dp = c->stride, nq = c->nq, cap = c->cap;
  if (c->n_rows == 0 || dp == 0 || dp % 64 != 0 || dp > 4096 || nq == 0 || nq > 256 || c->variant > kVarBf16Dma) return 1;
  if (cap < 64 || cap > (1u << 20) || c->blocks == 0 || c->blocks > 1024) return 1;
  if ((io->allow_bits != nullptr) != (c->allow_nbits != 0)) return 1;
  if ((c->variant == kVarF32Image) != (io->rows16 != nullptr)) return 1;
  const bool bf16 = c->variant == kVarBf16Dma;
  const uint32_t nqt = (nq + 31) / 32, n_tiles = (c->n_rows + 127) / 128, alloc = n_tiles * 128 + kSlackRows;
  const size_t row_b = (size_t)dp * (bf16 ? 2 : 4);
  const size_t n_words = 2 * (size_t)nq + 4 + (size_t)nq * vk::kSpillPerQuery;   // cand_cnt | ovf_q | spill_next, redo_cnt | qchunk

  DevBuf d_rows, d_img, d_q, d_lab, d_allow, d_tn, d_st, d_q16, d_thr, d_cnt, d_cand, d_spill;
  SP_TRY(d_rows.alloc((size_t)alloc * row_b));
  SP_TRY(d_img.alloc(io->rows16 ? (size_t)alloc * dp * 2 : 4));
  SP_TRY(d_q.alloc((size_t)nq * dp * 4));
  SP_TRY(d_lab.alloc((size_t)alloc * 8));
  SP_TRY(d_allow.alloc(((size_t)c->allow_nbits + 63) / 64 * 8 + 8));
  SP_TRY(d_tn.alloc((size_t)(n_tiles + 2) * 4));
  SP_TRY(d_st.alloc(64));
  SP_TRY(d_q16.alloc((size_t)nqt * 32 * dp * 2));
  SP_TRY(d_thr.alloc((size_t)nqt * 32 * (16 + 4 + 4)));
  SP_TRY(d_cnt.alloc(n_words * 4));
  SP_TRY(d_cand.alloc((size_t)nq * cap * 8));
  SP_TRY(d_spill.alloc(64));
  for (const DevBuf *b : {&d_rows, &d_img, &d_q16, &d_thr, &d_cnt, &d_cand, &d_spill}) SP_TRY(fill32(*b, c->fill));
  SP_TRY(hipMemcpy(d_rows.p, io->rows, (size_t)c->n_rows * row_b, hipMemcpyHostToDevice));
  if (io->rows16) SP_TRY(hipMemcpy(d_img.p, io->rows16, (size_t)c->n_rows * dp * 2, hipMemcpyHostToDevice));
  SP_TRY(hipMemcpy(d_q.p, io->queries, (size_t)nq * dp * 4, hipMemcpyHostToDevice));
  SP_TRY(hipMemset(d_lab.p, 0xFF, d_lab.bytes));
  SP_TRY(hipMemcpy(d_lab.p, io->labels, (size_t)c->n_rows * 8, hipMemcpyHostToDevice));
  SP_TRY(hipMemset(d_allow.p, 0, d_allow.bytes));
  if (io->allow_bits) SP_TRY(hipMemcpy(d_allow.p, io->allow_bits, ((size_t)c->allow_nbits + 63) / 64 * 8, hipMemcpyHostToDevice));
  SP_TRY(hipMemset(d_tn.p, 0, d_tn.bytes));
  SP_TRY(hipMemcpy(d_tn.p, io->tile_norm, (size_t)n_tiles * 4, hipMemcpyHostToDevice));
  SP_TRY(hipMemset(d_st.p, 0, 64));

  uint32_t *words = d_cnt.as<uint32_t>();
  vk::FlatFilterArgs f{};
  f.rows = d_rows.p;
  f.rows16 = io->rows16 ? d_img.p : nullptr;
  f.bf16 = bf16 ? 1 : 0;
  f.qbf16 = bf16 ? 1 : 0;
  f.dma = bf16 ? 1 : 0;
  f.bdma = 1;
  f.mfma16 = c->mfma16 ? 1 : 0;
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
  f.tile_norm = d_tn.as<uint32_t>();
  f.cand_cnt = words;
  f.cand_row = d_cand.as<uint32_t>();
  f.cand_val = reinterpret_cast<float *>(f.cand_row + nq * (size_t)cap);
  f.cap = cap;
  f.qchunk = words + 2 * (size_t)nq + 4;
  f.spill = d_spill.as<uint32_t>();
  f.spill_val = reinterpret_cast<float *>(d_spill.as<uint32_t>() + 8);
  f.spill_next = words + 2 * (size_t)nq;
  f.n_chunks = 0;                      // (a full list marks its query in ovf_q; nothing is written beyond the lists)
  f.redo_cnt = words + 2 * (size_t)nq + 1;
  f.ovf_q = words + nq;
  f.row_stride_f = dp;
  f.n_rows = c->n_rows;
  f.nq = nq;
  f.nqt = nqt;
  f.mode = 0;
  f.n_tiles = n_tiles;
  SP_TRY(vk::launch_flat_qprep(f, nullptr));
  SP_TRY(hipDeviceSynchronize());
  {   // the pass indexes memory with the counters qprep resets
    std::vector<uint32_t> h(nq);
    SP_TRY(hipMemcpy(h.data(), words, (size_t)nq * 4, hipMemcpyDeviceToHost));
    for (uint32_t q = 0; q < nq; ++q)
      if (h[q] != 0) return 2;
  }
  {   // the bounds: the caller's for the queries, +inf (closed, as a padding column is anyway) behind them
    std::vector<float> b((size_t)nqt * 32, __builtin_inff());
    for (uint32_t q = 0; q < nq; ++q) b[q] = io->qbound[q];
    SP_TRY(hipMemcpy(f.qbound, b.data(), b.size() * 4, hipMemcpyHostToDevice));
  }
  if (c->early_tiles != 0) {
    vk::FlatFilterArgs fe = f;
    fe.part_first = 0;
    fe.part_tiles = c->early_tiles;
    fe.early = 1;
    SP_TRY(vk::launch_flat_filter(fe, c->blocks, nullptr));
    SP_TRY(hipDeviceSynchronize());
    if (io->cnt_early) SP_TRY(hipMemcpy(io->cnt_early, f.cand_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost));
    f.part_first = c->early_tiles;
    f.part_tiles = 0xFFFFFFFFu;
  }
  SP_TRY(vk::launch_flat_filter(f, c->blocks, nullptr));
  SP_TRY(hipDeviceSynchronize());
  SP_TRY(hipMemcpy(io->cand_cnt, f.cand_cnt, (size_t)nq * 4, hipMemcpyDeviceToHost));
  SP_TRY(hipMemcpy(io->ovf_q, f.ovf_q, (size_t)nq * 4, hipMemcpyDeviceToHost));
  SP_TRY(hipMemcpy(io->cand_row, f.cand_row, (size_t)nq * cap * 4, hipMemcpyDeviceToHost));
  SP_TRY(hipMemcpy(io->cand_val, f.cand_val, (size_t)nq * cap * 4, hipMemcpyDeviceToHost));
  SP_TRY(hipMemcpy(io->qcoef, f.qcoef, (size_t)nqt * 32 * 16, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
