// hnsw_build_probe.hip -- TEST INFRASTRUCTURE (tests/test_hnsw_build_kernels_gpu.py), not part of libvkindex.so.
//
// The device HNSW build (valkey-search_amd/csrc/hnsw_build.hip, K9: eleven kernels behind five launchers) is reachable
// through the C ABI only behind the beam search and the host's threads, where recall is all that can be pinned.  This probe
// includes that translation unit itself (compile with -I valkey-search_amd/csrc), so the product's kernels and launchers are
// what runs, on inputs the test chooses, and hands back everything they wrote plus the whole links0 table.  Each call
// launches each launcher once; every output and scratch buffer is filled with 0xEE bytes first, so a word a kernel never
// wrote shows as 0xEEEEEEEE and no result can lean on a zeroed allocation.  Return codes: 0 = done, 1 = the arguments were
// refused (the kernels trust their caller: ids index the row table, counts index the lists -- nothing refused is ever
// launched), anything else = the source line that saw a HIP error; nothing is retried.
#include "hnsw_build.hip"

#include <string.h>

#include <vector>

namespace vk {
// kernels.hpp: the library's version (filter_set.cc) remembers what it has raised; one call per launch is enough here
hipError_t ensure_max_lds(const void *fn) { return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
}  // namespace vk

namespace {

constexpr uint32_t kMaxKeep = 192;   // what the host guarantees the kernels (hnsw_index.cc: maxM0 <= 192)

struct DevBuf {   // freed on every way out
  void *p = nullptr;
  size_t bytes = 0;
  ~DevBuf() { (void)hipFree(p); }
  hipError_t alloc(size_t b) { bytes = b ? b : 4; return hipMalloc(&p, bytes); }
  hipError_t dirty() { return hipMemset(p, 0xEE, bytes); }   // a word no kernel wrote stays 0xEEEEEEEE
  template <class T> T *as() const { return static_cast<T *>(p); }
};

#define HB_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)
#define HB_UP(buf, src, b) do { HB_TRY((buf).alloc(b)); if (b) HB_TRY(hipMemcpy((buf).p, src, b, hipMemcpyHostToDevice)); } while (0)
#define HB_DIRTY(buf, b) do { HB_TRY((buf).alloc(b)); HB_TRY((buf).dirty()); } while (0)
#define HB_DOWN(dst, buf, b) do { if (b) HB_TRY(hipMemcpy(dst, (buf).p, b, hipMemcpyDeviceToHost)); } while (0)

bool rows_ok(uint32_t n_rows, uint32_t stride) { return n_rows != 0 && stride != 0 && stride % 16 == 0; }

// every list of the table: count within the row and within max_cnt, ids inside the row table
bool links_ok(const uint32_t *links0, uint32_t n_rows, uint32_t l0s, uint32_t max_cnt) {
  for (uint32_t r = 0; r < n_rows; ++r) {
    const uint32_t *ll = links0 + (size_t)r * l0s, cnt = ll[0] & 0xFFFFu;
    if (cnt > max_cnt || cnt + 1 > l0s) return false;
    for (uint32_t i = 0; i < cnt; ++i)
      if (ll[1 + i] >= n_rows) return false;
  }
  return true;
}

// candidate lists of the new points first .. first + n_new - 1: every id the select kernel can read is a row
bool cands_ok(const uint64_t *cand_id, const uint32_t *cand_n, uint32_t cand_ld, uint32_t n_new, uint32_t first, uint32_t n_rows,
              uint32_t m, uint32_t l0s) {
  if (n_new == 0 || m == 0 || m > kMaxKeep || m + 1 > l0s || (uint64_t)first + n_new > n_rows) return false;
  for (uint32_t p = 0; p < n_new; ++p) {
    const uint32_t n = cand_n[p] < cand_ld ? cand_n[p] : cand_ld;
    for (uint32_t i = 0; i < n; ++i)
      if (cand_id[(size_t)p * cand_ld + i] >= n_rows) return false;
  }
  return true;
}

// the CSR the relink kernel walks: distinct touched nodes inside the table, offsets from 0 ascending, additions inside the table
bool csr_ok(const uint32_t *node, const uint32_t *off, const uint32_t *add_p, uint32_t n_touched, uint32_t n_rows) {
  if (off[0] != 0) return false;
  std::vector<uint8_t> seen(n_rows, 0);
  for (uint32_t t = 0; t < n_touched; ++t) {
    if (off[t + 1] < off[t] || node[t] >= n_rows || seen[node[t]]) return false;   // (two waves on one list would race)
    seen[node[t]] = 1;
  }
  for (uint32_t i = 0; i < off[n_touched]; ++i)
    if (add_p[i] >= n_rows) return false;
  return true;
}

struct Graph {   // the row table and the level-0 lists on the device
  DevBuf rows, links;
  size_t links_b = 0;
  int up(const void *h_rows, uint32_t n_rows, uint32_t stride, int bf16, const uint32_t *h_links, uint32_t l0s) {
    const size_t rows_b = (size_t)n_rows * stride * (bf16 ? 2 : 4);
    links_b = (size_t)n_rows * l0s * 4;
    HB_UP(rows, h_rows, rows_b);
    HB_UP(links, h_links, links_b);
    return 0;
  }
  void args(vk::HnswBuildArgs *b, uint32_t stride, uint32_t l0s) const {
    b->rows = rows.p;
    b->row_stride_f = stride;
    b->chunks = stride / 16;
    b->links0 = links.as<uint32_t>();
    b->l0_stride = l0s;
  }
};

struct GroupBufs {   // launch_hnsw_group's outputs and scratch, all dirty
  DevBuf keys_a, keys_b, vals_a, flags, pos, tmp, node, off, add_p, add_d, counts;
  int make(uint32_t n, vk::HnswGroupArgs *g) {
    HB_DIRTY(keys_a, (size_t)n * 8);
    HB_DIRTY(keys_b, (size_t)n * 8);
    HB_DIRTY(vals_a, (size_t)n * 4);
    HB_DIRTY(flags, (size_t)n * 4);
    HB_DIRTY(pos, (size_t)n * 4);
    HB_DIRTY(tmp, vk::hnsw_group_tmp_bytes(n));
    HB_DIRTY(node, (size_t)n * 4);
    HB_DIRTY(off, ((size_t)n + 1) * 4);
    HB_DIRTY(add_p, (size_t)n * 4);
    HB_DIRTY(add_d, (size_t)n * 4);
    HB_DIRTY(counts, 8);
    g->keys_a = keys_a.as<uint64_t>();
    g->keys_b = keys_b.as<uint64_t>();
    g->vals_a = vals_a.as<uint32_t>();
    g->flags = flags.as<uint32_t>();
    g->pos = pos.as<uint32_t>();
    g->tmp = tmp.p;
    g->tmp_bytes = vk::hnsw_group_tmp_bytes(n);
    g->node = node.as<uint32_t>();
    g->off = off.as<uint32_t>();
    g->add_p = add_p.as<uint32_t>();
    g->add_d = add_d.as<float>();
    g->counts = counts.as<uint32_t>();
    return 0;
  }
};

}  // namespace

// launch_hnsw_select.  rows [n_rows][stride] f32 or bf16 (stride in elements, a multiple of 16, zero padded); links0
// [n_rows][l0s] in and out; cand_id / cand_dist [n_new][cand_ld], cand_n [n_new] (may exceed cand_ld: the kernel clamps).
// out: sel_id / sel_dist [n_new][m], sel_n [n_new].
extern "C" int hb_probe_select(const void *rows, uint32_t n_rows, uint32_t stride, int bf16, int l2, uint32_t *links0, uint32_t l0s, uint32_t m,
                               const uint64_t *cand_id, const float *cand_dist, const uint32_t *cand_n, uint32_t cand_ld, uint32_t n_new,
                               uint32_t first, uint32_t *sel_id, float *sel_dist, uint32_t *sel_n) {
  if (!rows_ok(n_rows, stride) || !cands_ok(cand_id, cand_n, cand_ld, n_new, first, n_rows, m, l0s)) return 1;
  Graph gr;
  if (int rc = gr.up(rows, n_rows, stride, bf16, links0, l0s)) return rc;
  DevBuf d_cid, d_cd, d_cn, d_sid, d_sd, d_sn;
  const size_t cand_e = (size_t)n_new * cand_ld, sel_e = (size_t)n_new * m;
  HB_UP(d_cid, cand_id, cand_e * 8);
  HB_UP(d_cd, cand_dist, cand_e * 4);
  HB_UP(d_cn, cand_n, (size_t)n_new * 4);
  HB_DIRTY(d_sid, sel_e * 4);
  HB_DIRTY(d_sd, sel_e * 4);
  HB_DIRTY(d_sn, (size_t)n_new * 4);
  vk::HnswBuildArgs b{};
  gr.args(&b, stride, l0s);
  b.max_keep = m;
  b.cand_id = d_cid.as<uint64_t>();
  b.cand_dist = d_cd.as<float>();
  b.cand_n = d_cn.as<uint32_t>();
  b.cand_ld = cand_ld;
  b.n_new = n_new;
  b.first_id = first;
  b.sel_id = d_sid.as<uint32_t>();
  b.sel_dist = d_sd.as<float>();
  b.sel_n = d_sn.as<uint32_t>();
  if (vk::hnsw_build_lds_bytes(b, false) > 160 * 1024) return 1;
  HB_TRY(vk::launch_hnsw_select(b, l2 != 0, bf16 != 0, nullptr));
  HB_TRY(hipDeviceSynchronize());
  HB_DOWN(sel_id, d_sid, sel_e * 4);
  HB_DOWN(sel_dist, d_sd, sel_e * 4);
  HB_DOWN(sel_n, d_sn, (size_t)n_new * 4);
  HB_DOWN(links0, gr.links, gr.links_b);
  return 0;
}

// launch_hnsw_group.  sel_id / sel_dist [n_new][m], sel_n [n_new] (<= m).  out: counts [2], node [n], off [n + 1], add_p [n],
// add_d [n] with n = n_new * m.  No rows here: ids are free 32-bit words.
extern "C" int hb_probe_group(const uint32_t *sel_id, const float *sel_dist, const uint32_t *sel_n, uint32_t n_new, uint32_t m, uint32_t first,
                              uint32_t *counts, uint32_t *node, uint32_t *off, uint32_t *add_p, float *add_d) {
  if (n_new == 0 || m == 0 || (uint64_t)n_new * m >= (1ull << 28) || (uint64_t)first + n_new > 0xFFFFFFFFull) return 1;
  for (uint32_t p = 0; p < n_new; ++p)
    if (sel_n[p] > m) return 1;
  const uint32_t n = n_new * m;
  DevBuf d_sid, d_sd, d_sn;
  HB_UP(d_sid, sel_id, (size_t)n * 4);
  HB_UP(d_sd, sel_dist, (size_t)n * 4);
  HB_UP(d_sn, sel_n, (size_t)n_new * 4);
  vk::HnswGroupArgs g{};
  GroupBufs gb;
  if (int rc = gb.make(n, &g)) return rc;
  g.sel_id = d_sid.as<uint32_t>();
  g.sel_dist = d_sd.as<float>();
  g.sel_n = d_sn.as<uint32_t>();
  g.n_new = n_new;
  g.m = m;
  g.first_id = first;
  HB_TRY(vk::launch_hnsw_group(g, nullptr));
  HB_TRY(hipDeviceSynchronize());
  HB_DOWN(counts, gb.counts, 8);
  HB_DOWN(node, gb.node, (size_t)n * 4);
  HB_DOWN(off, gb.off, ((size_t)n + 1) * 4);
  HB_DOWN(add_p, gb.add_p, (size_t)n * 4);
  HB_DOWN(add_d, gb.add_d, (size_t)n * 4);
  return 0;
}

// launch_hnsw_relink.  node [n_touched], off [n_touched + 1], add_p / add_d [off[n_touched]].  bound == 0: the host knows
// n_touched (counts == nullptr).  bound >= n_touched: the number comes from device-side counts, the grid covers `bound`.
extern "C" int hb_probe_relink(const void *rows, uint32_t n_rows, uint32_t stride, int bf16, int l2, uint32_t *links0, uint32_t l0s, uint32_t max_keep,
                               const uint32_t *node, const uint32_t *off, const uint32_t *add_p, const float *add_d, uint32_t n_touched,
                               uint32_t bound) {
  if (!rows_ok(n_rows, stride) || max_keep == 0 || max_keep > kMaxKeep || max_keep + 1 > l0s || n_touched == 0) return 1;
  if (bound != 0 && bound < n_touched) return 1;
  if (!links_ok(links0, n_rows, l0s, max_keep) || !csr_ok(node, off, add_p, n_touched, n_rows)) return 1;
  Graph gr;
  if (int rc = gr.up(rows, n_rows, stride, bf16, links0, l0s)) return rc;
  DevBuf d_node, d_off, d_ap, d_ad, d_counts;
  const size_t pairs = off[n_touched];
  HB_UP(d_node, node, (size_t)n_touched * 4);
  HB_UP(d_off, off, ((size_t)n_touched + 1) * 4);
  HB_UP(d_ap, add_p, pairs * 4);
  HB_UP(d_ad, add_d, pairs * 4);
  const uint32_t h_counts[2] = {n_touched, (uint32_t)pairs};
  HB_UP(d_counts, h_counts, 8);
  vk::HnswBuildArgs b{};
  gr.args(&b, stride, l0s);
  b.max_keep = max_keep;
  b.node = d_node.as<uint32_t>();
  b.off = d_off.as<uint32_t>();
  b.add_p = d_ap.as<uint32_t>();
  b.add_d = d_ad.as<float>();
  b.n_touched = bound ? bound : n_touched;
  b.counts = bound ? d_counts.as<uint32_t>() : nullptr;
  if (vk::hnsw_build_lds_bytes(b, true) > 160 * 1024) return 1;
  HB_TRY(vk::launch_hnsw_relink(b, l2 != 0, bf16 != 0, nullptr));
  HB_TRY(hipDeviceSynchronize());
  HB_DOWN(links0, gr.links, gr.links_b);
  return 0;
}

// launch_hnsw_gather_lists.  node [n_node] with counts[0] = touched <= n_node.  out: dst [(n_new + n_node)][l0s]: the rows
// beyond n_new + touched stay 0xEEEEEEEE.
extern "C" int hb_probe_gather(const uint32_t *links0, uint32_t n_rows, uint32_t l0s, uint32_t first, uint32_t n_new, const uint32_t *node,
                               uint32_t n_node, uint32_t touched, uint32_t *dst) {
  if (n_rows == 0 || l0s == 0 || (uint64_t)first + n_new > n_rows || touched > n_node) return 1;
  for (uint32_t t = 0; t < touched; ++t)
    if (node[t] >= n_rows) return 1;
  DevBuf d_links, d_node, d_counts, d_dst;
  const size_t dst_b = ((size_t)n_new + n_node) * l0s * 4;
  HB_UP(d_links, links0, (size_t)n_rows * l0s * 4);
  HB_UP(d_node, node, (size_t)n_node * 4);
  const uint32_t h_counts[2] = {touched, 0xEEEEEEEEu};
  HB_UP(d_counts, h_counts, 8);
  HB_DIRTY(d_dst, dst_b);
  HB_TRY(vk::launch_hnsw_gather_lists(d_dst.as<uint32_t>(), d_links.as<uint32_t>(), l0s, first, n_new, d_node.as<uint32_t>(),
                                      d_counts.as<uint32_t>(), nullptr));
  HB_TRY(hipDeviceSynchronize());
  HB_DOWN(dst, d_dst, dst_b);
  return 0;
}

// launch_hnsw_widen_rows.  rows [n_rows][stride_e] bf16.  out [n + pad_rows][stride_e] f32: the pad rows stay 0xEEEEEEEE.
extern "C" int hb_probe_widen(const uint16_t *rows, uint32_t n_rows, uint32_t stride_e, uint32_t first, uint32_t n, uint32_t pad_rows, float *out) {
  if (n_rows == 0 || stride_e == 0 || (uint64_t)first + n > n_rows) return 1;
  DevBuf d_rows, d_out;
  const size_t out_b = ((size_t)n + pad_rows) * stride_e * 4;
  HB_UP(d_rows, rows, (size_t)n_rows * stride_e * 2);
  HB_DIRTY(d_out, out_b);
  HB_TRY(vk::launch_hnsw_widen_rows(d_rows.p, stride_e, first, n, d_out.as<float>(), nullptr));
  HB_TRY(hipDeviceSynchronize());
  HB_DOWN(out, d_out, out_b);
  return 0;
}

// select (max_keep = m) -> group -> relink (max_keep = max_m0, device-side counts, bound n_new * m) -> gather, enqueued on one
// stream as HnswIndex::device_batch does.  out: counts [2], node [n_new * m], lists [(n_new + n_new * m)][l0s], links0.
extern "C" int hb_probe_chain(const void *rows, uint32_t n_rows, uint32_t stride, int bf16, int l2, uint32_t *links0, uint32_t l0s, uint32_t m,
                              uint32_t max_m0, const uint64_t *cand_id, const float *cand_dist, const uint32_t *cand_n, uint32_t cand_ld,
                              uint32_t n_new, uint32_t first, uint32_t *counts, uint32_t *node, uint32_t *lists) {
  if (!rows_ok(n_rows, stride) || !cands_ok(cand_id, cand_n, cand_ld, n_new, first, n_rows, m, l0s)) return 1;
  if (max_m0 < m || max_m0 > kMaxKeep || max_m0 + 1 > l0s || !links_ok(links0, n_rows, l0s, max_m0)) return 1;
  Graph gr;
  if (int rc = gr.up(rows, n_rows, stride, bf16, links0, l0s)) return rc;
  DevBuf d_cid, d_cd, d_cn, d_sid, d_sd, d_sn, d_lists;
  const uint32_t np = n_new * m;
  const size_t cand_e = (size_t)n_new * cand_ld, lists_b = ((size_t)n_new + np) * l0s * 4;
  HB_UP(d_cid, cand_id, cand_e * 8);
  HB_UP(d_cd, cand_dist, cand_e * 4);
  HB_UP(d_cn, cand_n, (size_t)n_new * 4);
  HB_DIRTY(d_sid, (size_t)np * 4);
  HB_DIRTY(d_sd, (size_t)np * 4);
  HB_DIRTY(d_sn, (size_t)n_new * 4);
  HB_DIRTY(d_lists, lists_b);
  vk::HnswGroupArgs g{};
  GroupBufs gb;
  if (int rc = gb.make(np, &g)) return rc;
  vk::HnswBuildArgs b{};
  gr.args(&b, stride, l0s);
  b.max_keep = m;
  b.cand_id = d_cid.as<uint64_t>();
  b.cand_dist = d_cd.as<float>();
  b.cand_n = d_cn.as<uint32_t>();
  b.cand_ld = cand_ld;
  b.n_new = n_new;
  b.first_id = first;
  b.sel_id = d_sid.as<uint32_t>();
  b.sel_dist = d_sd.as<float>();
  b.sel_n = d_sn.as<uint32_t>();
  g.sel_id = b.sel_id;
  g.sel_dist = b.sel_dist;
  g.sel_n = b.sel_n;
  g.n_new = n_new;
  g.m = m;
  g.first_id = first;
  vk::HnswBuildArgs widest = b;
  widest.max_keep = max_m0;
  if (vk::hnsw_build_lds_bytes(b, false) > 160 * 1024 || vk::hnsw_build_lds_bytes(widest, true) > 160 * 1024) return 1;
  hipStream_t s = nullptr;
  HB_TRY(vk::launch_hnsw_select(b, l2 != 0, bf16 != 0, s));
  HB_TRY(vk::launch_hnsw_group(g, s));
  b.node = g.node;
  b.off = g.off;
  b.add_p = g.add_p;
  b.add_d = g.add_d;
  b.counts = g.counts;
  b.n_touched = np;
  b.max_keep = max_m0;
  HB_TRY(vk::launch_hnsw_relink(b, l2 != 0, bf16 != 0, s));
  HB_TRY(vk::launch_hnsw_gather_lists(d_lists.as<uint32_t>(), gr.links.as<uint32_t>(), l0s, first, n_new, g.node, g.counts, s));
  HB_TRY(hipDeviceSynchronize());
  HB_DOWN(counts, gb.counts, 8);
  HB_DOWN(node, gb.node, (size_t)np * 4);
  HB_DOWN(lists, d_lists, lists_b);
  HB_DOWN(links0, gr.links, gr.links_b);
  return 0;
}
