// prefilter_resolve.cc -- the batched pre-filter search with the label -> slot step on the device (option
// prefilter-device-resolve): the owner of an index's device label map, and the driver that stands where prefilter_resolve +
// prefilter_device_stage (prefilter_host.hpp, prefilter_batch.cc) stand with the option off.  The kernels are in
// label_map.hip; K8b and K8c (prefilter_select.hip) are launched as the host-resolved path launches them.
#include <string.h>

#include <algorithm>
#include <vector>

#include "index.hpp"
#include "label_map_hash.hpp"

namespace vk {

// ---- the map of one index ---------------------------------------------------------------------------------------------
// the table built whole from the published labels on stream s, the stream synchronised; headroom = slots beyond `count` the
// sizing rule is asked for (upkeep: a table that is exactly twice the count would be due again after the first new label)
bool DeviceLabelMap::rebuild(uint64_t epoch, uint32_t count, const uint64_t *d_labels, const uint32_t *d_links0, uint32_t l0_stride,
                             uint64_t budget, hipStream_t s, uint64_t headroom) {
  tagged_ = true;
  epoch_ = epoch;
  count_ = count;
  usable_ = false;
  used_ = live_ = 0;
  const uint64_t capacity = label_map_capacity((uint64_t)count + headroom);
  const uint64_t bytes = capacity * 12 + 32;   // keys | values | the failure word, the four counters of an apply launch
  if (bytes > budget || capacity > kLabelMapMaxCapacity || !buf_.ensure(bytes).ok()) {
    buf_.release();
    bytes_.store(0, std::memory_order_relaxed);
    return false;
  }
  bytes_.store(buf_.cap, std::memory_order_relaxed);
  t_.keys = buf_.as<uint64_t>();
  t_.vals = reinterpret_cast<uint32_t *>(t_.keys + capacity);
  t_.fail = reinterpret_cast<unsigned int *>(t_.vals + capacity);
  t_.capacity = capacity;
  LabelMapBuildArgs a{};
  a.t = t_;
  a.labels = d_labels;
  a.links0 = d_links0;
  a.l0_stride = l0_stride;
  a.count = count;
  unsigned int failed = 1;
  if (launch_label_map_build(a, s) != hipSuccess || hipMemcpyAsync(&failed, t_.fail, 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  builds_.fetch_add(1, std::memory_order_relaxed);
  usable_ = failed == 0;
  return usable_;
}

bool DeviceLabelMap::ready(uint64_t epoch, uint32_t count, const uint64_t *d_labels, const uint32_t *d_links0, uint32_t l0_stride, uint64_t budget,
                           hipStream_t s, LabelMapTable *out, const LabelMapUpkeep *up) {
  std::lock_guard<std::mutex> g(mu_);
  const bool same = tagged_ && epoch_ == epoch && count_ == count;
  if (up == nullptr || !up->on) {
    if (!same) {   // another publication: rebuilt whole, on this batch's stream
      touched_.clear();   // (whatever the phase touched is in the labels the build reads)
      rebuild(epoch, count, d_labels, d_links0, l0_stride, budget, s, 0);
      used_ = live_ = up ? up->live : 0;
    }
  } else if (!same || !touched_.empty()) {
    // upkeep: the labels the write phase touched against the index's truth, applied to the table where it lies.  Everything
    // up to the synchronise happens under mu_: no other stream sees a half-applied table.
    std::vector<uint64_t> labels;
    bool everything = false;
    touched_.take(&labels, &everything);
    LabelMapDelta d;
    if (!everything && labels.size() > up->delta_max) everything = true;
    if (!everything && tagged_ && usable_) label_map_net_delta(&labels, up->truth, &d);
    LabelMapState st;
    st.usable = tagged_ && usable_;
    st.capacity = st.usable ? t_.capacity : 0;
    st.used = used_;
    st.live = live_;
    const LabelMapPlan plan = label_map_plan(st, everything, d.upserts, count);
    bool applied = false;
    if (plan == LabelMapPlan::kApply) {
      LabelMapApplied c;
      const uint64_t n = d.labels.size();
      bool ok = n <= 0xFFFFFFFFull && delta_.ensure(std::max<uint64_t>(n, 1) * 12).ok();
      if (ok && n) {
        LabelMapApplyArgs a{};
        a.t = t_;
        a.labels = delta_.as<uint64_t>();
        a.slots = reinterpret_cast<const uint32_t *>(delta_.as<uint64_t>() + n);
        a.n = (uint32_t)n;
        a.counters = t_.fail + 1;
        unsigned int back[1 + kLabelMapCounters] = {1, 0, 0, 0, 0};
        ok = hipMemcpyAsync(delta_.p, d.labels.data(), n * 8, hipMemcpyHostToDevice, s) == hipSuccess &&
             hipMemcpyAsync(delta_.as<uint64_t>() + n, d.slots.data(), n * 4, hipMemcpyHostToDevice, s) == hipSuccess &&
             launch_label_map_apply(a, s) == hipSuccess &&
             hipMemcpyAsync(back, t_.fail, sizeof(back), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        c.fail = back[0];
        c.claimed = back[1 + kLabelMapClaimed];
        c.revived = back[1 + kLabelMapRevived];
        c.killed = back[1 + kLabelMapKilled];
        c.moved = back[1 + kLabelMapMoved];
      }
      uint64_t live_after = 0;
      if (ok) {
        delta_batches_.fetch_add(1, std::memory_order_relaxed);
        delta_records_.fetch_add(n, std::memory_order_relaxed);
        claimed_.fetch_add(c.claimed, std::memory_order_relaxed);
        revived_.fetch_add(c.revived, std::memory_order_relaxed);
        killed_.fetch_add(c.killed, std::memory_order_relaxed);
        moved_.fetch_add(c.moved, std::memory_order_relaxed);
        used_ += c.claimed;
      }
      if (ok && label_map_check_applied(live_, c, up->live, &live_after)) {
        live_ = live_after;
        epoch_ = epoch;
        count_ = count;
        applied = true;
      } else {   // a touched label was missed somewhere, or a launch failed: never served from -- rebuilt at once, same stream
        delta_mismatches_.fetch_add(1, std::memory_order_relaxed);
      }
    } else if (plan != LabelMapPlan::kRebuildNoMap) {
      rebuilds_forced_.fetch_add(1, std::memory_order_relaxed);
    }
    if (!applied) {
      rebuild(epoch, count, d_labels, d_links0, l0_stride, budget, s, count / 4);
      used_ = live_ = up->live;
    }
  }
  if (!usable_) return false;
  *out = t_;
  return true;
}

void DeviceLabelMap::release() {
  std::lock_guard<std::mutex> g(mu_);
  buf_.release();
  delta_.release();
  bytes_.store(0, std::memory_order_relaxed);
  tagged_ = usable_ = false;
  used_ = live_ = 0;
  touched_.clear();
}

void DeviceLabelMap::stats(vk_label_map_stats *out) {
  std::lock_guard<std::mutex> g(mu_);
  const bool have = tagged_ && usable_;
  out->builds = builds_.load(std::memory_order_relaxed);
  out->delta_batches = delta_batches_.load(std::memory_order_relaxed);
  out->delta_records = delta_records_.load(std::memory_order_relaxed);
  out->claimed = claimed_.load(std::memory_order_relaxed);
  out->revived = revived_.load(std::memory_order_relaxed);
  out->killed = killed_.load(std::memory_order_relaxed);
  out->moved = moved_.load(std::memory_order_relaxed);
  out->dead_entries = have ? used_ - live_ : 0;
  out->used_entries = have ? used_ : 0;
  out->capacity = have ? t_.capacity : 0;
  out->delta_mismatches = delta_mismatches_.load(std::memory_order_relaxed);
  out->rebuilds_forced = rebuilds_forced_.load(std::memory_order_relaxed);
}

Status DeviceLabelMap::read(uint64_t *out_labels, uint32_t *out_slots, uint64_t cap, uint64_t *out_n) {
  std::lock_guard<std::mutex> g(mu_);
  *out_n = 0;
  if (!tagged_ || !usable_) return Status::Err(VK_ERR_INTERNAL, "the device has no room for the label map");
  std::vector<uint64_t> keys(t_.capacity);
  std::vector<uint32_t> vals(t_.capacity);
  VK_HIP_TRY(hipMemcpy(keys.data(), t_.keys, t_.capacity * 8, hipMemcpyDeviceToHost));
  VK_HIP_TRY(hipMemcpy(vals.data(), t_.vals, t_.capacity * 4, hipMemcpyDeviceToHost));
  uint64_t n = 0;
  for (uint64_t h = 0; h < t_.capacity; ++h) {
    if (keys[h] == kLabelMapEmpty || vals[h] == kLabelMapNone) continue;
    if (n < cap) {
      out_labels[n] = keys[h];
      out_slots[n] = vals[h];
    }
    ++n;
  }
  *out_n = n;
  return Status::Ok();
}

// ---- the driver ---------------------------------------------------------------------------------------------------------
namespace {

// the lists of one device pass, resolved: device arrays for K8b / K8c, host copies of the offsets and the kept positions
struct ResolvedLists {
  const uint32_t *d_seg = nullptr, *d_tile = nullptr, *d_slot = nullptr;
  const uint32_t *h_seg = nullptr, *h_tile = nullptr, *h_pos = nullptr;   // h_pos: indices into the uploaded keys
};

// keys[0 .. n) cut into ns lists by lb (ns + 1 ascending offsets, lb[ns] - lb[0] == n; nullptr = one list): upload, the
// three resolve launches, one download (offsets and positions), one synchronise
Status resolve_lists(SearchCtx *ctx, const LabelMapTable &map, const uint64_t *keys, uint64_t n, const uint64_t *lb, uint64_t ns,
                     ResolvedLists *out) {
  const uint64_t csr_words = 2 * (ns + 1), csr_bytes = (csr_words * 4 + 7) & ~7ull;
  VK_TRY(ctx->h_idx.ensure(csr_bytes));
  uint32_t *h_lb = ctx->h_idx.as<uint32_t>(), *h_kt = h_lb + ns + 1;
  uint32_t e = 0, t = 0;
  for (uint64_t s = 0; s < ns; ++s) {
    h_lb[s] = e;
    h_kt[s] = t;
    const uint64_t len = lb ? lb[s + 1] - lb[s] : n;
    e += (uint32_t)len;
    t += label_map_key_tiles(len);
  }
  h_lb[ns] = e;
  h_kt[ns] = t;
  // device: [list_begin | ktile_begin | keys] in, [seg_begin | tile_begin | pos | slot | raw | tile_off] out
  VK_TRY(ctx->d_pool.ensure(csr_bytes + n * 8));
  const uint64_t back_words = csr_words + n, out_words = csr_words + 3 * n + t + 1;
  VK_TRY(ctx->d_idx.ensure(out_words * 4));
  VK_TRY(ctx->h_out_l.ensure(back_words * 4));
  char *din = ctx->d_pool.as<char>();
  VK_HIP_TRY(hipMemcpyAsync(din, h_lb, csr_words * 4, hipMemcpyHostToDevice, ctx->stream));
  if (n) VK_HIP_TRY(hipMemcpyAsync(din + csr_bytes, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
  uint32_t *dout = ctx->d_idx.as<uint32_t>();
  LabelMapResolveArgs a{};
  a.t = map;
  a.keys = reinterpret_cast<const uint64_t *>(din + csr_bytes);
  a.list_begin = reinterpret_cast<const uint32_t *>(din);
  a.ktile_begin = a.list_begin + ns + 1;
  a.n_seg = (uint32_t)ns;
  a.n_keys = (uint32_t)n;
  a.n_ktiles = t;
  a.seg_begin = dout;
  a.tile_begin = dout + ns + 1;
  a.pos = dout + csr_words;
  a.slot = a.pos + n;
  a.raw = a.slot + n;
  a.tile_off = a.raw + n;
  VK_HIP_TRY(launch_label_map_resolve(a, ctx->stream));
  VK_HIP_TRY(hipMemcpyAsync(ctx->h_out_l.p, dout, back_words * 4, hipMemcpyDeviceToHost, ctx->stream));
  VK_HIP_TRY(hipStreamSynchronize(ctx->stream));
  out->d_seg = a.seg_begin;
  out->d_tile = a.tile_begin;
  out->d_slot = a.slot;
  out->h_seg = ctx->h_out_l.as<uint32_t>();
  out->h_tile = out->h_seg + ns + 1;
  out->h_pos = out->h_seg + csr_words;
  return Status::Ok();
}

}  // namespace

Status prefilter_device_stage_keys(SearchCtx *ctx, const LabelMapTable &map, const void *d_rows, uint32_t dim, uint32_t stride_f, bool l2,
                                   bool bf16, const float *queries, uint64_t nq, uint64_t k, const uint64_t *labels, const uint64_t *list_begin,
                                   uint64_t n_labels, PrefilterCands *out, bool *took, uint64_t *resolved_keys) {
  const bool shared = list_begin == nullptr;
  const uint64_t cap = prefilter_cap(k);
  *took = false;
  *resolved_keys = 0;
  // what prefilter_device_stage hands to the per-query path, and any list beyond the scratch (shorter once its unknown
  // labels are gone, perhaps): the host-resolved path decides, as it does with the option off
  if (k == 0 || cap == 0 || (uint64_t)stride_f * 4 > 160 * 1024) return Status::Ok();
  if (shared && n_labels > kPrefilterChunkEntries) return Status::Ok();
  for (uint64_t q = 0; !shared && q < nq; ++q)
    if (list_begin[q + 1] - list_begin[q] > kPrefilterChunkEntries) return Status::Ok();
  *took = true;
  out->reset(nq, false);
  const uint64_t q_bytes = (uint64_t)stride_f * 4;
  const uint64_t per_q = std::max<uint64_t>(q_bytes, cap * 8);
  const uint64_t max_q = std::max<uint64_t>(1, std::min<uint64_t>(kPrefilterChunkBytes / per_q, 1u << 16));   // (prefilter_batch.cc's)
  ResolvedLists r;
  if (shared) {   // one resolve for the batch, whatever nq is
    VK_TRY(resolve_lists(ctx, map, labels, n_labels, nullptr, 1, &r));
    *resolved_keys += n_labels;
  }
  for (uint64_t q0 = 0; q0 < nq;) {
    // the chunk: queries [q0, q1) -- as many as the scratch bounds allow (by the lists' lengths as sent), at least one
    uint64_t q1 = q0, keys = 0;
    while (q1 < nq && q1 - q0 < max_q) {
      const uint64_t len = shared ? 0 : list_begin[q1 + 1] - list_begin[q1];
      if (q1 > q0 && keys + len > kPrefilterChunkEntries) break;
      keys += len;
      ++q1;
    }
    const uint64_t cq = q1 - q0, base = shared ? 0 : list_begin[q0];
    if (!shared && keys) {
      VK_TRY(resolve_lists(ctx, map, labels + base, keys, list_begin + q0, cq, &r));
      *resolved_keys += keys;
    }
    const uint64_t entries = shared ? r.h_seg[1] : (keys ? r.h_seg[cq] : 0);
    if (entries == 0) {   // nothing known in any list of the chunk: empty answers
      for (uint64_t q = q0; q < q1; ++q) out->begin[q + 1] = out->items.size();
      q0 = q1;
      continue;
    }
    VK_TRY(ctx->h_q.ensure(cq * q_bytes));
    VK_TRY(ctx->d_q.ensure(cq * q_bytes));
    char *h = ctx->h_q.as<char>();
    for (uint64_t q = 0; q < cq; ++q) {
      float *dst = reinterpret_cast<float *>(h + q * q_bytes);
      memcpy(dst, queries + (q0 + q) * dim, (size_t)dim * 4);
      memset(dst + dim, 0, (size_t)(stride_f - dim) * 4);
    }
    VK_HIP_TRY(hipMemcpyAsync(ctx->d_q.p, h, cq * q_bytes, hipMemcpyHostToDevice, ctx->stream));
    // distances ([cq][m] shared, CSR otherwise), then the hand-back: [cq] counts | [cq][cap] (index, distance bits)
    const uint64_t dist_entries = shared ? cq * entries : entries;
    VK_TRY(ctx->d_tmp.ensure(dist_entries * 4));
    const uint64_t off_cand = (cq * 4 + 7) & ~7ull, back_bytes = off_cand + cq * cap * 8;
    VK_TRY(ctx->d_out_d.ensure(back_bytes));
    VK_TRY(ctx->h_tmp.ensure(back_bytes));
    PrefilterDistArgs da{};
    da.rows = d_rows;
    da.queries = ctx->d_q.as<float>();
    da.idx = r.d_slot;
    da.seg_begin = shared ? nullptr : r.d_seg;
    da.tile_begin = shared ? nullptr : r.d_tile;
    da.out = ctx->d_tmp.as<float>();
    da.row_stride_f = stride_f;
    da.q_stride_f = stride_f;
    da.chunks = stride_f / 16;
    da.nq = (uint32_t)cq;
    da.shared_len = shared ? (uint32_t)entries : 0;
    da.n_tiles = shared ? 0 : r.h_tile[cq];
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
      const uint64_t lo = shared ? 0 : r.h_seg[q], len = shared ? entries : r.h_seg[q + 1] - lo;
      if (prefilter_is_fallback(cnt[q], cap)) {
        out->fallback[gq] = 1;
      } else {
        const uint32_t *c = cand + q * cap * 2;
        for (uint32_t i = 0; i < cnt[q]; ++i) {
          if (c[2 * i] >= len) return Status::Err(VK_ERR_INTERNAL, "prefilter: a candidate outside its list");
          PrefilterCand pc;
          pc.pos = base + r.h_pos[lo + c[2 * i]];
          memcpy(&pc.dist, &c[2 * i + 1], 4);
          out->items.push_back(pc);
        }
      }
      out->begin[gq + 1] = out->items.size();
    }
    q0 = q1;
  }
  return Status::Ok();
}

}  // namespace vk
