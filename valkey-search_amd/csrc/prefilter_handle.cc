// prefilter_handle.cc -- vk_index_search_filter_exact_batch on any index: exact kNN among the rows a device filter admits,
// for a caller that holds the handle and no key array.  The driver of the device stage of one run on one device stands
// beside prefilter_resolve.cc's: the expansion of the bitmap (filter_expand.hip) takes the place of the upload of the keys,
// and a gather of the candidates' labels the place of the download of the kept positions; the resolve launches
// (label_map.hip), K8b and K8c (prefilter_select.hip) are launched as prefilter_device_stage_keys launches them.  The
// HIP-free pieces are in prefilter_handle_host.hpp.
#include <string.h>

#include <algorithm>

#include "filter_lane.hpp"
#include "index.hpp"

namespace vk {

namespace {
// Most distances of one chunk of queries (x 4 B = 256 MiB of d_tmp).  The list path's shared case has no such bound (its
// scratch is nq x list entries whatever they come to); here a run is cut into chunks of queries instead, at least one query
// each, so a single query over kPrefilterChunkEntries labels still takes 64 MiB.
constexpr uint64_t kHandleDistEntries = 1ull << 26;
}

Status prefilter_handle_stage(SearchCtx *ctx, const LabelMapTable *map, const uint64_t *d_bits, uint64_t nbits, uint64_t allowed,
                              const void *d_rows, uint32_t dim, uint32_t stride_f, bool l2, bool bf16, const float *queries, uint64_t nq,
                              uint64_t k, HandleCands *out, uint64_t *expanded, uint64_t *known) {
  const uint64_t cap = prefilter_cap(k);
  *expanded = 0;
  *known = 0;
  out->reset(nq, true);
  if (map == nullptr || k == 0 || cap == 0 || (uint64_t)stride_f * 4 > 160 * 1024 || allowed > kPrefilterChunkEntries) return Status::Ok();
  // ---- the expansion: [list_begin | ktile_begin] (4 words) | total | - | keys [n] | tile_off [tiles], n as the filter counted it
  const uint64_t n = allowed, tiles = filter_expand_tiles(nbits), off_keys = 32;
  const uint32_t kt = label_map_key_tiles(n);
  VK_TRY(ctx->d_pool.ensure(off_keys + n * 8 + tiles * 8 + 8));
  VK_TRY(ctx->h_idx.ensure(64));
  char *din = ctx->d_pool.as<char>();
  uint64_t *d_keys = reinterpret_cast<uint64_t *>(din + off_keys);
  unsigned long long *d_total = reinterpret_cast<unsigned long long *>(din + 16);
  uint32_t *h_csr = ctx->h_idx.as<uint32_t>();
  volatile uint64_t *h_total = ctx->h_idx.as<uint64_t>() + 2;
  uint32_t *h_back = h_csr + 8;
  h_csr[0] = 0;
  h_csr[1] = (uint32_t)n;
  h_csr[2] = 0;
  h_csr[3] = kt;
  VK_HIP_TRY(hipMemcpyAsync(din, h_csr, 16, hipMemcpyHostToDevice, ctx->stream));
  VK_HIP_TRY(launch_filter_expand(d_bits, nbits, n, d_keys, d_total, reinterpret_cast<unsigned long long *>(d_keys + n), ctx->stream));
  VK_HIP_TRY(hipMemcpyAsync(const_cast<uint64_t *>(h_total), d_total, 8, hipMemcpyDeviceToHost, ctx->stream));
  VK_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const uint64_t total = *h_total;
  *expanded = std::min(total, n);
  if (total != n) return Status::Ok();   // the device's count is the truth: the list path, over a list read with the right size
  out->reset(nq, false);
  if (n == 0) return Status::Ok();       // nothing admitted: empty answers
  // ---- label -> slot: the list is one shared segment; [seg_begin | tile_begin | pos | slot | raw | tile_off] out
  const uint64_t out_words = 4 + 3 * n + kt + 1;
  VK_TRY(ctx->d_idx.ensure(out_words * 4));
  uint32_t *dout = ctx->d_idx.as<uint32_t>();
  LabelMapResolveArgs a{};
  a.t = *map;
  a.keys = d_keys;
  a.list_begin = reinterpret_cast<const uint32_t *>(din);
  a.ktile_begin = a.list_begin + 2;
  a.n_seg = 1;
  a.n_keys = (uint32_t)n;
  a.n_ktiles = kt;
  a.seg_begin = dout;
  a.tile_begin = dout + 2;
  a.pos = dout + 4;
  a.slot = a.pos + n;
  a.raw = a.slot + n;
  a.tile_off = a.raw + n;
  VK_HIP_TRY(launch_label_map_resolve(a, ctx->stream));
  VK_HIP_TRY(hipMemcpyAsync(h_back, dout, 16, hipMemcpyDeviceToHost, ctx->stream));   // the offsets only: pos[] stays on the device
  VK_HIP_TRY(hipStreamSynchronize(ctx->stream));
  const uint64_t entries = h_back[1];
  if (entries > n) return Status::Err(VK_ERR_INTERNAL, "prefilter: more resolved entries than keys");
  *known = entries;
  if (entries == 0) return Status::Ok();   // no admitted label is a row of this index: empty answers
  // ---- K8b, K8c and the labels of the hand-back, a chunk of queries at a time
  const uint64_t q_bytes = (uint64_t)stride_f * 4;
  const uint64_t per_q = std::max<uint64_t>(q_bytes, cap * 8);
  const uint64_t max_q = std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(kPrefilterChunkBytes / per_q, kHandleDistEntries / entries), 65535));
  for (uint64_t q0 = 0; q0 < nq; q0 += max_q) {
    const uint64_t cq = std::min(max_q, nq - q0);
    VK_TRY(ctx->h_q.ensure(cq * q_bytes));
    VK_TRY(ctx->d_q.ensure(cq * q_bytes));
    char *h = ctx->h_q.as<char>();
    for (uint64_t q = 0; q < cq; ++q) {
      float *dst = reinterpret_cast<float *>(h + q * q_bytes);
      memcpy(dst, queries + (q0 + q) * dim, (size_t)dim * 4);
      memset(dst + dim, 0, (size_t)(stride_f - dim) * 4);
    }
    VK_HIP_TRY(hipMemcpyAsync(ctx->d_q.p, h, cq * q_bytes, hipMemcpyHostToDevice, ctx->stream));
    VK_TRY(ctx->d_tmp.ensure(cq * entries * 4));
    const uint64_t off_cand = (cq * 4 + 7) & ~7ull, back_bytes = off_cand + cq * cap * 8;
    VK_TRY(ctx->d_out_d.ensure(back_bytes));
    VK_TRY(ctx->d_out_l.ensure(cq * cap * 8));
    VK_TRY(ctx->h_tmp.ensure(back_bytes));
    VK_TRY(ctx->h_out_l.ensure(cq * cap * 8));
    PrefilterDistArgs da{};
    da.rows = d_rows;
    da.queries = ctx->d_q.as<float>();
    da.idx = a.slot;
    da.out = ctx->d_tmp.as<float>();
    da.row_stride_f = stride_f;
    da.q_stride_f = stride_f;
    da.chunks = stride_f / 16;
    da.nq = (uint32_t)cq;
    da.shared_len = (uint32_t)entries;
    VK_HIP_TRY(launch_prefilter_distance(da, l2, bf16, ctx->stream));
    PrefilterSelectArgs sa{};
    sa.dist = da.out;
    sa.shared_len = da.shared_len;
    sa.nq = (uint32_t)cq;
    sa.k = (uint32_t)k;
    sa.cap = (uint32_t)cap;
    sa.count = ctx->d_out_d.as<uint32_t>();
    sa.cand = reinterpret_cast<uint2 *>(ctx->d_out_d.as<char>() + off_cand);
    VK_HIP_TRY(launch_prefilter_select(sa, ctx->stream));
    VK_HIP_TRY(launch_filter_gather_labels(sa.count, sa.cand, a.pos, d_keys, (uint32_t)entries, (uint32_t)cq, (uint32_t)cap,
                                           ctx->d_out_l.as<uint64_t>(), ctx->stream));
    VK_HIP_TRY(hipMemcpyAsync(ctx->h_tmp.p, ctx->d_out_d.p, back_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP_TRY(hipMemcpyAsync(ctx->h_out_l.p, ctx->d_out_l.p, cq * cap * 8, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t *cnt = ctx->h_tmp.as<uint32_t>();
    const uint32_t *cand = reinterpret_cast<const uint32_t *>(ctx->h_tmp.as<char>() + off_cand);
    const uint64_t *lab = ctx->h_out_l.as<uint64_t>();
    for (uint64_t q = 0; q < cq; ++q) {
      const uint64_t gq = q0 + q;
      if (prefilter_is_fallback(cnt[q], cap)) {
        out->fallback[gq] = 1;
      } else {
        const uint32_t *c = cand + q * cap * 2;
        for (uint32_t i = 0; i < cnt[q]; ++i) {
          if (c[2 * i] >= entries) return Status::Err(VK_ERR_INTERNAL, "prefilter: a candidate outside its list");
          HandleCand hc;
          hc.label = lab[q * cap + i];
          memcpy(&hc.dist, &c[2 * i + 1], 4);
          out->items.push_back(hc);
        }
      }
      out->begin[gq + 1] = out->items.size();
    }
  }
  return Status::Ok();
}

Status filter_read_labels(const FilterSet &f, uint64_t *out_labels, uint64_t cap, uint64_t *out_n) {
  const int device = f.first_device();
  if (device < 0) return Status::Err(VK_ERR_INTERNAL, "filter: no device copy");
  VK_HIP_TRY(hipSetDevice(device));
  filter_lane::BuildLane *lane = filter_lane::lane_of(device);
  std::lock_guard<std::mutex> lk(lane->mu);
  VK_TRY(filter_lane::lane_ready(lane));
  filter_lane::LaneDrain drain{lane->stream};
  // the scratch holds what the filter counted, and no more than the caller takes: keys [n] | tile_off [tiles]
  const uint64_t n = std::min(cap, f.allowed()), tiles = filter_expand_tiles(f.nbits());
  VK_TRY(filter_lane::stage_ensure(lane, (size_t)(n * 8 + tiles * 8 + 8)));
  uint64_t *d_keys = static_cast<uint64_t *>(lane->d_stage);
  VK_HIP_TRY(launch_filter_expand(f.bits_on(device), f.nbits(), n, d_keys, lane->d_count, reinterpret_cast<unsigned long long *>(d_keys + n),
                                  lane->stream));
  unsigned long long total = 0;
  VK_HIP_TRY(hipMemcpyAsync(&total, lane->d_count, 8, hipMemcpyDeviceToHost, lane->stream));
  VK_HIP_TRY(hipStreamSynchronize(lane->stream));
  *out_n = total;
  uint64_t have = std::min<uint64_t>(total, n);
  if (have) VK_HIP_TRY(hipMemcpy(out_labels, d_keys, (size_t)have * 8, hipMemcpyDeviceToHost));
  if (have < std::min<uint64_t>(total, cap)) {
    // the device found more labels than the filter had counted: once more with the caller's room
    const uint64_t m = std::min<uint64_t>(total, cap);
    VK_TRY(filter_lane::stage_ensure(lane, (size_t)(m * 8 + tiles * 8 + 8)));
    d_keys = static_cast<uint64_t *>(lane->d_stage);
    VK_HIP_TRY(launch_filter_expand(f.bits_on(device), f.nbits(), m, d_keys, lane->d_count, reinterpret_cast<unsigned long long *>(d_keys + m),
                                    lane->stream));
    VK_HIP_TRY(hipStreamSynchronize(lane->stream));
    VK_HIP_TRY(hipMemcpy(out_labels, d_keys, (size_t)m * 8, hipMemcpyDeviceToHost));
  }
  return Status::Ok();
}

Status Index::search_filter_exact_batch(const float *queries, uint64_t nq, uint64_t k, const FilterSet *const *tab, float *out_dist,
                                        uint64_t *out_label, uint64_t *out_n) {
  for (uint64_t q = 0; q < nq; ++q) out_n[q] = 0;
  if (nq == 0 || k == 0) return Status::Ok();
  for (uint64_t i = 0; i < nq * k; ++i) { out_dist[i] = __builtin_inff(); out_label[i] = ~0ull; }
  std::vector<std::pair<uint64_t, uint64_t>> runs;
  handle_runs(reinterpret_cast<const void *const *>(tab), nq, &runs);
  const uint64_t dim = params_.dim;
  uint64_t fell = 0, downloaded = 0;
  HandleCands c;
  std::vector<uint64_t> which, list;
  for (const auto &run : runs) {
    const uint64_t q0 = run.first, q1 = run.second, rq = q1 - q0;
    const FilterSet &f = *tab[q0];
    VK_TRY(handle_candidates(queries + q0 * dim, rq, k, f, &c));
    if (c.fallback.size() != rq || c.begin.size() != rq + 1) return Status::Err(VK_ERR_INTERNAL, "prefilter: malformed handle candidates");
    for (uint64_t q = q0; q < q1; ++q) {
      if (c.fallback[q - q0]) continue;
      handle_finish(c.items.data() + c.begin[q - q0], c.begin[q - q0 + 1] - c.begin[q - q0], k, out_dist + q * k, out_label + q * k, out_n + q);
    }
    handle_fallback_queries(c, q0, q1, &which);
    if (which.empty()) continue;
    // what the device stage handed over: the run's list on the host, once, and the list path for those queries
    uint64_t total = 0;
    list.resize(f.allowed());
    VK_TRY(filter_read_labels(f, list.data(), list.size(), &total));
    if (total > list.size()) {
      list.resize(total);
      VK_TRY(filter_read_labels(f, list.data(), list.size(), &total));
    }
    list.resize(std::min<uint64_t>(total, list.size()));
    ++downloaded;
    fell += which.size();
    if (which.size() == rq) {   // the whole run: in place
      VK_TRY(search_labels_batch(queries + q0 * dim, rq, k, list.data(), nullptr, list.size(), out_dist + q0 * k, out_label + q0 * k, out_n + q0));
      continue;
    }
    std::vector<float> fq(which.size() * dim), fd(which.size() * k);
    std::vector<uint64_t> fl(which.size() * k), fn(which.size());
    for (size_t i = 0; i < which.size(); ++i) memcpy(fq.data() + i * dim, queries + which[i] * dim, (size_t)dim * 4);
    VK_TRY(search_labels_batch(fq.data(), which.size(), k, list.data(), nullptr, list.size(), fd.data(), fl.data(), fn.data()));
    for (size_t i = 0; i < which.size(); ++i) {
      memcpy(out_dist + which[i] * k, fd.data() + i * k, (size_t)k * 4);
      memcpy(out_label + which[i] * k, fl.data() + i * k, (size_t)k * 8);
      out_n[which[i]] = fn[i];
    }
  }
  hx_.batches.fetch_add(1, std::memory_order_relaxed);
  hx_.queries.fetch_add(nq, std::memory_order_relaxed);
  hx_.runs.fetch_add(runs.size(), std::memory_order_relaxed);
  hx_.fallback_queries.fetch_add(fell, std::memory_order_relaxed);
  hx_.downloaded_runs.fetch_add(downloaded, std::memory_order_relaxed);
  return Status::Ok();
}

}  // namespace vk
