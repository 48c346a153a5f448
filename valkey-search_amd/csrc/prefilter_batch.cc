// prefilter_batch.cc -- vk_index_search_labels_batch on any index: the device stage's driver (one device) and the host
// half that turns candidates into answers.  The kernels are in prefilter_select.hip, the HIP-free pieces (heap rule,
// candidate order, fallback decision, sharded union) in prefilter_host.hpp.
#include <string.h>

#include <algorithm>

#include "index.hpp"

namespace vk {

Status prefilter_device_stage(SearchCtx *ctx, const void *d_rows, uint32_t dim, uint32_t stride_f, bool l2, bool bf16, const float *queries,
                              uint64_t k, const PrefilterResolved &r, PrefilterCands *out) {
  const uint64_t nq = r.nq;
  const uint64_t cap = prefilter_cap(k);
  out->reset(nq, false);
  // what the stage does not cover at all: k beyond the hand-back's size, a vector too long for the query's place in LDS
  // (the per-query path refuses that one itself), a shared list beyond the scratch
  if (k == 0 || cap == 0 || (uint64_t)stride_f * 4 > 160 * 1024 || (r.shared && r.begin[1] > kPrefilterChunkEntries)) {
    out->reset(nq, true);
    return Status::Ok();
  }
  const uint64_t q_bytes = (uint64_t)stride_f * 4;
  const uint64_t per_q_bytes = std::max<uint64_t>(q_bytes, cap * 8);
  const uint64_t max_q = std::max<uint64_t>(1, std::min<uint64_t>(kPrefilterChunkBytes / per_q_bytes, 1u << 16));
  for (uint64_t q0 = 0; q0 < nq;) {
    // the chunk: queries [q0, q1) -- as many as the scratch bounds allow, at least one
    uint64_t q1 = q0, entries = 0;
    while (q1 < nq && q1 - q0 < max_q) {
      const uint64_t len = prefilter_seg_len(r, q1);
      if (!r.shared && len > kPrefilterChunkEntries) {   // a list beyond the scratch: the per-query path (an empty segment here)
        out->fallback[q1] = 1;
        ++q1;
        continue;
      }
      if (q1 > q0 && entries + len > kPrefilterChunkEntries) break;
      entries += len;
      ++q1;
    }
    const uint64_t cq = q1 - q0;
    if (entries == 0) {   // nothing known in any list of the chunk: empty answers
      for (uint64_t q = q0; q < q1; ++q) out->begin[q + 1] = out->items.size();
      q0 = q1;
      continue;
    }
    // one staging block: [cq] padded queries | [cq + 1] segment offsets | [cq + 1] tile offsets | slots
    const uint64_t n_slots = r.shared ? r.begin[1] : entries;
    const uint64_t off_seg = cq * q_bytes, off_tile = off_seg + (cq + 1) * 4, off_idx = off_tile + (cq + 1) * 4;
    const uint64_t up_bytes = off_idx + n_slots * 4;
    VK_TRY(ctx->h_q.ensure(up_bytes));
    VK_TRY(ctx->d_q.ensure(up_bytes));
    char *h = ctx->h_q.as<char>();
    for (uint64_t q = 0; q < cq; ++q) {
      float *dst = reinterpret_cast<float *>(h + q * q_bytes);
      memcpy(dst, queries + (q0 + q) * dim, (size_t)dim * 4);
      memset(dst + dim, 0, (size_t)(stride_f - dim) * 4);
    }
    uint32_t *seg = reinterpret_cast<uint32_t *>(h + off_seg), *tile = reinterpret_cast<uint32_t *>(h + off_tile);
    uint32_t *idx = reinterpret_cast<uint32_t *>(h + off_idx);
    if (r.shared) {
      memcpy(idx, r.slot.data(), n_slots * 4);
    } else {
      uint32_t e = 0, t = 0;
      for (uint64_t q = 0; q < cq; ++q) {
        seg[q] = e;
        tile[q] = t;
        if (out->fallback[q0 + q]) continue;
        const uint64_t len = prefilter_seg_len(r, q0 + q);
        memcpy(idx + e, r.slot.data() + prefilter_seg_lo(r, q0 + q), len * 4);
        e += (uint32_t)len;
        t += prefilter_tiles(len);
      }
      seg[cq] = e;
      tile[cq] = t;
    }
    VK_HIP_TRY(hipMemcpyAsync(ctx->d_q.p, h, up_bytes, hipMemcpyHostToDevice, ctx->stream));
    // distances ([cq][m] shared, CSR otherwise), then the hand-back: [cq] counts | [cq][cap] (index, distance bits)
    const uint64_t dist_entries = r.shared ? cq * n_slots : entries;
    VK_TRY(ctx->d_tmp.ensure(dist_entries * 4));
    const uint64_t off_cand = (cq * 4 + 7) & ~7ull, back_bytes = off_cand + cq * cap * 8;
    VK_TRY(ctx->d_out_d.ensure(back_bytes));
    VK_TRY(ctx->h_tmp.ensure(back_bytes));
    const char *dq = ctx->d_q.as<char>();
    PrefilterDistArgs da{};
    da.rows = d_rows;
    da.queries = reinterpret_cast<const float *>(dq);
    da.idx = reinterpret_cast<const uint32_t *>(dq + off_idx);
    da.seg_begin = r.shared ? nullptr : reinterpret_cast<const uint32_t *>(dq + off_seg);
    da.tile_begin = r.shared ? nullptr : reinterpret_cast<const uint32_t *>(dq + off_tile);
    da.out = ctx->d_tmp.as<float>();
    da.row_stride_f = stride_f;
    da.q_stride_f = stride_f;
    da.chunks = stride_f / 16;
    da.nq = (uint32_t)cq;
    da.shared_len = r.shared ? (uint32_t)n_slots : 0;
    da.n_tiles = r.shared ? 0 : tile[cq];
    VK_HIP_TRY(launch_prefilter_distance(da, l2, bf16, ctx->stream));
    PrefilterSelectArgs sa{};
    sa.dist = da.out;
    sa.seg_begin = da.seg_begin;
    sa.shared_len = da.shared_len;
    sa.nq = (uint32_t)cq;
    sa.k = (uint32_t)k;
    sa.cap = (uint32_t)cap;
    sa.count = ctx->d_out_d.as<uint32_t>();
    sa.cand = reinterpret_cast<uint2 *>(ctx->d_out_d.as<char>() + off_cand);
    VK_HIP_TRY(launch_prefilter_select(sa, ctx->stream));
    VK_HIP_TRY(hipMemcpyAsync(ctx->h_tmp.p, ctx->d_out_d.p, back_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VK_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t *cnt = ctx->h_tmp.as<uint32_t>();
    const uint32_t *cand = reinterpret_cast<const uint32_t *>(ctx->h_tmp.as<char>() + off_cand);
    for (uint64_t q = 0; q < cq; ++q) {
      const uint64_t gq = q0 + q;
      if (!out->fallback[gq]) {
        const uint64_t lo = prefilter_seg_lo(r, gq), len = prefilter_seg_len(r, gq);
        if (prefilter_is_fallback(cnt[q], cap)) {
          out->fallback[gq] = 1;
        } else {
          const uint32_t *c = cand + q * cap * 2;
          for (uint32_t i = 0; i < cnt[q]; ++i) {
            if (c[2 * i] >= len) return Status::Err(VK_ERR_INTERNAL, "prefilter: a candidate outside its list");
            PrefilterCand pc;
            pc.pos = r.pos[lo + c[2 * i]];
            memcpy(&pc.dist, &c[2 * i + 1], 4);
            out->items.push_back(pc);
          }
        }
      }
      out->begin[gq + 1] = out->items.size();
    }
    q0 = q1;
  }
  return Status::Ok();
}

Status Index::search_labels_batch(const float *queries, uint64_t nq, uint64_t k, const uint64_t *labels, const uint64_t *list_begin,
                                  uint64_t n_labels, float *out_dist, uint64_t *out_label, uint64_t *out_n) {
  for (uint64_t q = 0; q < nq; ++q) out_n[q] = 0;
  if (nq == 0 || k == 0) return Status::Ok();
  for (uint64_t i = 0; i < nq * k; ++i) { out_dist[i] = __builtin_inff(); out_label[i] = ~0ull; }
  PrefilterCands c;
  VK_TRY(prefilter_candidates(queries, nq, k, labels, list_begin, n_labels, &c));
  if (c.fallback.size() != nq || c.begin.size() != nq + 1) return Status::Err(VK_ERR_INTERNAL, "prefilter: malformed candidates");
  uint64_t fell = 0;
  for (uint64_t q = 0; q < nq; ++q) {
    if (c.fallback[q]) continue;
    prefilter_finish(c.items.data() + c.begin[q], c.begin[q + 1] - c.begin[q], labels, k, out_dist + q * k, out_label + q * k, out_n + q);
  }
  // what the device stage handed over: the per-query path, after the batch
  for (uint64_t q = 0; q < nq; ++q) {
    if (!c.fallback[q]) continue;
    ++fell;
    const uint64_t lo = list_begin ? list_begin[q] : 0, hi = list_begin ? list_begin[q + 1] : n_labels;
    VK_TRY(search_labels(queries + q * params_.dim, k, labels + lo, hi - lo, out_dist + q * k, out_label + q * k, out_n + q));
  }
  pf_.fallback_queries.fetch_add(fell, std::memory_order_relaxed);
  return Status::Ok();
}

}  // namespace vk
