// filter_l2_image_probe.hip -- TEST INFRASTRUCTURE (tests/test_flat_l2_image_kernels_gpu.py), not part of libvkindex.so.
//
// The early and the main pass of the candidate filter over an f32 L2 index, through registers (rows16 = nullptr) or over the f16
// image of the rows (option flat-l2-image), on buffers the probe owns.  This file includes valkey-search_amd/csrc/flat_filter.hip
// itself (compile with -I valkey-search_amd/csrc and the library's flags), so the product's kernels and launchers are what runs:
// launch_row_stats (tile norms, half norms, the image), launch_flat_qprep, then launch_flat_filter twice -- the early pass over
// the first early_tiles tiles of every block's range and the main pass behind them -- against bounds the CALLER sets, so that
// both row paths gate against the same numbers.  Every workspace word holds `fill` before the first launch.
// Return codes: 0 ok, 1 refused arguments, 2 time limit (probe_common.hpp), else the source line that saw a HIP error.
#include "flat_filter.hip"

#include "probe_common.hpp"

namespace vk {
// kernels.hpp: the library's version (filter_set.cc) remembers what it has raised; one call per launch is enough here
hipError_t ensure_max_lds(const void *fn) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
}  // namespace vk

extern "C" {

struct L2iCfg {
  uint32_t n_rows, stride, nq;   // stride = row_stride_f = q_stride_f: the padded dimension, a multiple of 64
  uint32_t image;                // 0 = the register path, 1 = the passes read the image
  uint32_t cap;                  // private list entries per query (>= n_rows: nothing spills)
  uint32_t blocks;               // grid of both passes (may exceed the tiles: blocks that own none)
  uint32_t early_tiles;          // tiles per block of the early pass
  uint32_t fill;
};

struct L2iIO {
  const float *rows;       // [n_rows][stride]
  const float *queries;    // [nq][stride]
  const float *qbound;     // [nqt * 32] the gate's bounds, accumulator space (dot - |x|^2 / 2)
  uint32_t *tile_norm;     // [n_tiles + 2]
  float *qcoef;            // [nqt * 32][4]
  uint32_t *cnt;           // [nq] survivors per query
  uint32_t *cand;          // [nq][cap] rows | [nq][cap] score bits
};

int l2i_probe_passes(const L2iCfg *c, const L2iIO *io) {
  if (probe::g_leak) return probe::kRefused;
  const uint32_t dp = c->stride, nq = c->nq, cap = c->cap;
  if (c->n_rows == 0 || nq == 0 || nq > 256 || dp == 0 || dp % 64 != 0 || dp > 4096 || c->image > 1) return probe::kRefused;
  if (cap < c->n_rows || cap > (1u << 16) || c->blocks == 0 || c->blocks > 1024 || c->early_tiles == 0) return probe::kRefused;
  const uint32_t nqt = (nq + 31) / 32, n_tiles = (c->n_rows + 127) / 128, alloc = n_tiles * 128 + 256;   // (RowStore::kRowSlack)
  const size_t w_ovf = nq, w_misc = 2 * (size_t)nq, w_chunk = 3 * (size_t)nq + 4, w_done = w_chunk + (size_t)nq * vk::kSpillPerQuery;
  const size_t n_words = w_done + 2 * (size_t)nq;
  if (vk::flat_filter_dma_lds_bytes() > 160 * 1024) return probe::kRefused;

  probe::DevBuf d_rows, d_q, d_lab, d_tn, d_st, d_hn, d_img, d_q16, d_thr, d_cnt, d_cand, d_spill;
  PB_TRY(d_rows.alloc((size_t)alloc * dp * 4));
  PB_TRY(d_q.alloc((size_t)nq * dp * 4));
  PB_TRY(d_lab.alloc((size_t)alloc * 8));
  PB_TRY(d_tn.alloc((size_t)(n_tiles + 2) * 4));
  PB_TRY(d_st.alloc(64));
  PB_TRY(d_hn.alloc((size_t)alloc * 4));
  PB_TRY(d_img.alloc((size_t)alloc * dp * 2));
  PB_TRY(d_q16.alloc((size_t)nqt * 32 * dp * 2));
  PB_TRY(d_thr.alloc((size_t)nqt * 32 * (16 + 4 + 4)));
  PB_TRY(d_cnt.alloc(n_words * 4));
  PB_TRY(d_cand.alloc((size_t)nq * cap * 8));
  PB_TRY(d_spill.alloc(8));
  for (const probe::DevBuf *b : {&d_rows, &d_hn, &d_img, &d_q16, &d_thr, &d_cnt, &d_cand}) PB_TRY(probe::fill(*b, c->fill, nullptr));
  for (const probe::DevBuf *b : {&d_lab, &d_tn, &d_st}) PB_TRY(probe::fill(*b, 0u, nullptr));   // (atomicMax tables start from zero)
  PB_TRY(probe::up(d_rows.p, io->rows, (size_t)c->n_rows * dp * 4, nullptr));
  PB_TRY(probe::up(d_q.p, io->queries, (size_t)nq * dp * 4, nullptr));
  PB_TRY(vk::launch_row_stats(d_rows.p, false, true, dp, 0, c->n_rows, n_tiles, d_st.as<uint32_t>(), d_tn.as<uint32_t>(), d_hn.as<uint32_t>(),
                              c->image ? d_img.p : nullptr, nullptr, vk::kImageF16));
  PB_WAIT(nullptr);

  // flat_index.cc scan_filter, "FlatFilterArgs f{};" to "f.redo_cnt = redo_cnt;" for an f32 L2 index
  uint32_t *words = d_cnt.as<uint32_t>();
  vk::FlatFilterArgs f{};
  f.rows = d_rows.p;
  f.rows16 = c->image ? d_img.p : nullptr;
  f.l2 = 1;
  f.bdma = 1;
  f.hn16 = d_hn.as<uint32_t>();
  f.labels = d_lab.as<uint64_t>();
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
  f.qchunk = words + w_chunk;
  f.spill = d_spill.as<uint32_t>();
  f.spill_val = reinterpret_cast<float *>(f.spill) + 1;
  f.spill_next = words + w_misc;
  f.n_chunks = 0;
  f.ovf_q = words + w_ovf;
  f.done_cnt = words + w_done;
  f.rerank_cnt = words + w_done + nq;
  f.row_stride_f = dp;
  f.n_rows = c->n_rows;
  f.nq = nq;
  f.nqt = nqt;
  f.n_tiles = n_tiles;
  f.redo_cnt = words + w_misc + 1;
  PB_TRY(vk::launch_flat_qprep(f, nullptr));
  PB_TRY(probe::up(f.qbound, io->qbound, (size_t)nqt * 32 * 4, nullptr));
  vk::FlatFilterArgs fe = f, fm = f;
  fe.part_first = 0;
  fe.part_tiles = c->early_tiles;
  fe.early = 1;
  fm.part_first = c->early_tiles;
  fm.part_tiles = 0xFFFFFFFFu;
  PB_TRY(vk::launch_flat_filter(fe, c->blocks, nullptr));
  PB_WAIT(nullptr);
  PB_TRY(vk::launch_flat_filter(fm, c->blocks, nullptr));
  PB_WAIT(nullptr);
  PB_TRY(probe::down(io->tile_norm, d_tn.p, (size_t)(n_tiles + 2) * 4));
  PB_TRY(probe::down(io->qcoef, d_thr.p, (size_t)nqt * 32 * 16));
  PB_TRY(probe::down(io->cnt, d_cnt.p, (size_t)nq * 4));
  PB_TRY(probe::down(io->cand, d_cand.p, (size_t)nq * cap * 8));
  return 0;
}

}  // extern "C"
