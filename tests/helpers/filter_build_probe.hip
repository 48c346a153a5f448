// filter_build_probe.hip -- TEST INFRASTRUCTURE (tests/test_filter_kernels_gpu.py), not part of libvkindex.so.
//
// The device filter kernels (valkey-search_amd/csrc/filter_build.hip) are reachable through the C ABI only behind FilterSet,
// which hands back words() words and one added-up count: the slack word, the bits above nbits, the per-block partial sums and
// whatever a count is added ONTO stay out of sight, and every build there is small enough for one trip of every loop.  This
// probe includes that translation unit itself (compile with -I valkey-search_amd/csrc and the library's flags), so the
// product's kernels and launchers are what runs, on buffers the test owns.  Every buffer a kernel writes is filled with a word
// of the caller's choice first, except where the contract (kernels.hpp) says "zeroed by the caller" or "holds the set to
// extend": there the caller supplies the content.  Whole buffers come back, slack and padding included.
//
// Return codes: 0 = done, 1 = the arguments were refused (the kernels trust their caller; nothing refused is launched), 2 = a
// launch did not finish within the time limit (the buffers stay where they are and every later call is refused), -1 = the
// launcher itself answered hipErrorInvalidValue (the buffers still come back: nothing may have been written), anything else
// = the source line that saw a HIP error.
#include "filter_build.hip"

#include <vector>

#include "filter_lane.hpp"   // kPartials
#include "probe_common.hpp"

using probe::DevBuf;
using probe::Stream;

namespace {
constexpr uint64_t kPad = 2;                              // words behind every bitmap's slack word, and behind every count table
constexpr uint64_t kPartials = vk::filter_lane::kPartials;
constexpr int kInvalid = -1;

int open_stream(Stream &st) { return hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking) == hipSuccess ? 0 : __LINE__; }
}  // namespace

extern "C" uint32_t fb_probe_set_ids_blocks(uint64_t n) { return vk::filter_set_ids_blocks(n); }
extern "C" uint32_t fb_probe_set_runs_blocks(uint64_t n_runs) { return vk::filter_set_runs_blocks(n_runs); }
extern "C" uint32_t fb_probe_combine_blocks(uint64_t words) { return vk::filter_combine_blocks(words); }
extern "C" uint32_t fb_probe_partials() { return (uint32_t)kPartials; }
extern "C" uint32_t fb_probe_pad() { return (uint32_t)kPad; }

// launch_filter_set_ids (runs = 0: data [n] ids) or launch_filter_set_runs (runs = 1: data [n][2] = first, last) onto
// bits_io [alloc_words]: in = the set to extend (the caller's words, also those past (nbits + 63) / 64), out = the same words after
// the launch.  out_partial [kPartials]: what the launch did not write shows the fill.
extern "C" int fb_probe_set(uint32_t fill, int runs, uint64_t *bits_io, uint64_t alloc_words, uint64_t nbits, const uint64_t *data, uint64_t n,
                            uint64_t *out_partial) {
  if (probe::g_leak) return probe::kRefused;
  if (nbits > ((uint64_t)1 << 40) || alloc_words < (nbits + 63) / 64 + 1 || n > ((uint64_t)1 << 26)) return probe::kRefused;
  if ((runs ? vk::filter_set_runs_blocks(n) : vk::filter_set_ids_blocks(n)) > kPartials) return probe::kRefused;
  Stream st;
  if (int rc = open_stream(st)) return rc;
  DevBuf d_bits, d_data, d_part;
  const size_t data_bytes = (size_t)n * (runs ? 16 : 8);
  PB_TRY(d_bits.alloc(alloc_words * 8));
  PB_TRY(d_data.alloc(data_bytes));
  PB_TRY(d_part.alloc(kPartials * 8));
  PB_TRY(probe::up(d_bits.p, bits_io, alloc_words * 8, st.s));
  PB_TRY(probe::up(d_data.p, data, data_bytes, st.s));
  PB_TRY(probe::fill(d_part, fill, st.s));
  if (runs) PB_TRY(vk::launch_filter_set_runs(d_bits.as<uint64_t>(), nbits, d_data.as<uint64_t>(), n, d_part.as<unsigned long long>(), st.s));
  else PB_TRY(vk::launch_filter_set_ids(d_bits.as<uint64_t>(), nbits, d_data.as<uint64_t>(), n, d_part.as<unsigned long long>(), st.s));
  PB_WAIT(st.s);
  PB_TRY(probe::down(bits_io, d_bits.p, alloc_words * 8));
  PB_TRY(probe::down(out_partial, d_part.p, kPartials * 8));
  return 0;
}

// launch_filter_popcount over bits [words] onto out[0] = start; out [4] comes back whole (out[1 .. 3] show the fill)
extern "C" int fb_probe_popcount(uint32_t fill, const uint64_t *bits, uint64_t words, uint64_t start, uint64_t *out) {
  if (probe::g_leak) return probe::kRefused;
  if (words > ((uint64_t)1 << 26)) return probe::kRefused;
  Stream st;
  if (int rc = open_stream(st)) return rc;
  DevBuf d_bits, d_out;
  PB_TRY(d_bits.alloc(words * 8));
  PB_TRY(d_out.alloc(4 * 8));
  PB_TRY(probe::up(d_bits.p, bits, words * 8, st.s));
  PB_TRY(probe::fill(d_out, fill, st.s));
  PB_TRY(probe::up(d_out.p, &start, 8, st.s));
  PB_TRY(vk::launch_filter_popcount(d_bits.as<uint64_t>(), words, d_out.as<unsigned long long>(), st.s));
  PB_WAIT(st.s);
  PB_TRY(probe::down(out, d_out.p, 4 * 8));
  return 0;
}

// launch_filter_combine: a, b [words]; out_dst [words + 1 + kPad] and out_partial [kPartials] start as the fill
extern "C" int fb_probe_combine(uint32_t fill, const uint64_t *a, const uint64_t *b, uint64_t words, uint32_t op, uint64_t *out_dst,
                                uint64_t *out_partial) {
  if (probe::g_leak) return probe::kRefused;
  if (words > ((uint64_t)1 << 26) || op > 2 || vk::filter_combine_blocks(words) > kPartials) return probe::kRefused;
  Stream st;
  if (int rc = open_stream(st)) return rc;
  DevBuf d_a, d_b, d_dst, d_part;
  PB_TRY(d_a.alloc(words * 8));
  PB_TRY(d_b.alloc(words * 8));
  PB_TRY(d_dst.alloc((words + 1 + kPad) * 8));
  PB_TRY(d_part.alloc(kPartials * 8));
  PB_TRY(probe::up(d_a.p, a, words * 8, st.s));
  PB_TRY(probe::up(d_b.p, b, words * 8, st.s));
  PB_TRY(probe::fill(d_dst, fill, st.s));
  PB_TRY(probe::fill(d_part, fill, st.s));
  PB_TRY(vk::launch_filter_combine(d_dst.as<uint64_t>(), d_a.as<uint64_t>(), d_b.as<uint64_t>(), words, op, d_part.as<unsigned long long>(), st.s));
  PB_WAIT(st.s);
  PB_TRY(probe::down(out_dst, d_dst.p, (words + 1 + kPad) * 8));
  PB_TRY(probe::down(out_partial, d_part.p, kPartials * 8));
  return 0;
}

// launch_filter_combine_batch: operands [n_ops][words]; table [n][3] = (a index, b index, op); the probe builds the device
// pointer table.  counts_io [n + kPad]: in = the first n starting values, out = the whole table (the pad shows the fill);
// out_dst [n][words + 1 + kPad] starts as the fill.
extern "C" int fb_probe_combine_batch(uint32_t fill, const uint64_t *operands, uint32_t n_ops, uint64_t words, const uint32_t *table, uint32_t n,
                                      uint64_t *counts_io, uint64_t *out_dst) {
  if (probe::g_leak) return probe::kRefused;
  const uint64_t per = words + 1 + kPad;
  if (words > ((uint64_t)1 << 22) || n > (1u << 17) || (uint64_t)n * per > ((uint64_t)1 << 26) || (uint64_t)n_ops * words > ((uint64_t)1 << 26)) return probe::kRefused;
  for (uint32_t i = 0; i < n; ++i)
    if (table[3 * i] >= n_ops || table[3 * i + 1] >= n_ops || table[3 * i + 2] > 2) return probe::kRefused;
  Stream st;
  if (int rc = open_stream(st)) return rc;
  DevBuf d_ops, d_dst, d_items, d_counts;
  PB_TRY(d_ops.alloc((size_t)n_ops * words * 8));
  PB_TRY(d_dst.alloc((size_t)n * per * 8));
  PB_TRY(d_items.alloc((size_t)n * 32));
  PB_TRY(d_counts.alloc(((size_t)n + kPad) * 8));
  std::vector<uint64_t> items((size_t)n * 4);
  for (uint32_t i = 0; i < n; ++i) {
    items[4 * (size_t)i] = reinterpret_cast<uint64_t>(d_dst.as<uint64_t>() + (size_t)i * per);
    items[4 * (size_t)i + 1] = reinterpret_cast<uint64_t>(d_ops.as<uint64_t>() + (size_t)table[3 * i] * words);
    items[4 * (size_t)i + 2] = reinterpret_cast<uint64_t>(d_ops.as<uint64_t>() + (size_t)table[3 * i + 1] * words);
    items[4 * (size_t)i + 3] = table[3 * i + 2];
  }
  PB_TRY(probe::up(d_ops.p, operands, (size_t)n_ops * words * 8, st.s));
  PB_TRY(probe::up(d_items.p, items.data(), items.size() * 8, st.s));
  PB_TRY(probe::fill(d_dst, fill, st.s));
  PB_TRY(probe::fill(d_counts, fill, st.s));
  PB_TRY(probe::up(d_counts.p, counts_io, (size_t)n * 8, st.s));
  PB_WAIT(st.s);   // (`items` is pageable: its copy has left the vector before the launcher is asked anything)
  const hipError_t e = vk::launch_filter_combine_batch(d_items.as<uint64_t>(), n, words, d_counts.as<unsigned long long>(), st.s);
  if (e != hipSuccess && e != hipErrorInvalidValue) return __LINE__;
  PB_WAIT(st.s);
  PB_TRY(probe::down(out_dst, d_dst.p, (size_t)n * per * 8));
  PB_TRY(probe::down(counts_io, d_counts.p, ((size_t)n + kPad) * 8));
  return e == hipErrorInvalidValue ? kInvalid : 0;
}

// launch_filter_delta_copy, then (stop_after_copy == 0) launch_filter_delta_apply with the clears, then with the sets, in
// stream order as filter_delta.cc issues them.  n items: base_off[i] = the item's base as a word offset into bases
// [bases_words], or UINT64_MAX for none; base_words[i], dst_words[i], nbits[i] as the table carries them.  clr / set: raw
// records (label | item << kFilterDeltaLabelBits), labels at or beyond nbits included.  counts_io [n + kPad] as above;
// out_dst: the items' buffers one behind the other, dst_words[i] + 1 + kPad words each, all starting as the fill.
extern "C" int fb_probe_delta(uint32_t fill, int stop_after_copy, const uint64_t *bases, uint64_t bases_words, const uint64_t *base_off,
                              const uint64_t *base_words, const uint64_t *dst_words, const uint64_t *nbits, uint32_t n, uint64_t max_dst_words,
                              const uint64_t *clr, uint64_t n_clr, const uint64_t *set, uint64_t n_set, uint64_t *counts_io, uint64_t *out_dst) {
  if (probe::g_leak) return probe::kRefused;
  if (n == 0 || n > 65535 || bases_words > ((uint64_t)1 << 26) || n_clr > ((uint64_t)1 << 24) || n_set > ((uint64_t)1 << 24)) return probe::kRefused;
  std::vector<uint64_t> off((size_t)n + 1, 0);
  for (uint32_t i = 0; i < n; ++i) {
    // (filter_delta.cc: dst_words is the new filter's words(); the apply kernel trusts label < nbits to lie inside them, the
    //  copy kernel reads base_words words of the base whenever dst_words reaches that far)
    if (nbits[i] > ((uint64_t)1 << vk::kFilterDeltaLabelBits) || dst_words[i] != (nbits[i] + 63) / 64 || dst_words[i] > max_dst_words) return probe::kRefused;
    if (base_off[i] != UINT64_MAX && (base_off[i] > bases_words || base_words[i] > bases_words - base_off[i])) return probe::kRefused;
    off[i + 1] = off[i] + dst_words[i] + 1 + kPad;
  }
  if (off[n] > ((uint64_t)1 << 26)) return probe::kRefused;
  for (int pass = 0; pass < 2; ++pass)
    for (uint64_t j = 0, m = pass ? n_set : n_clr; j < m; ++j)
      if (((pass ? set : clr)[j] >> vk::kFilterDeltaLabelBits) >= n) return probe::kRefused;
  Stream st;
  if (int rc = open_stream(st)) return rc;
  DevBuf d_bases, d_dst, d_items, d_clr, d_set, d_counts;
  PB_TRY(d_bases.alloc(bases_words * 8));
  PB_TRY(d_dst.alloc(off[n] * 8));
  PB_TRY(d_items.alloc((size_t)n * vk::kFilterDeltaItemWords * 8));
  PB_TRY(d_clr.alloc(n_clr * 8));
  PB_TRY(d_set.alloc(n_set * 8));
  PB_TRY(d_counts.alloc(((size_t)n + kPad) * 8));
  std::vector<uint64_t> items((size_t)n * vk::kFilterDeltaItemWords);
  for (uint32_t i = 0; i < n; ++i) {
    uint64_t *t = &items[(size_t)i * vk::kFilterDeltaItemWords];
    t[0] = reinterpret_cast<uint64_t>(d_dst.as<uint64_t>() + off[i]);
    t[1] = base_off[i] == UINT64_MAX ? 0 : reinterpret_cast<uint64_t>(d_bases.as<uint64_t>() + base_off[i]);
    t[2] = base_off[i] == UINT64_MAX ? 0 : base_words[i];
    t[3] = dst_words[i];
    t[4] = nbits[i];
    t[5] = 0;
  }
  PB_TRY(probe::up(d_bases.p, bases, bases_words * 8, st.s));
  PB_TRY(probe::up(d_items.p, items.data(), items.size() * 8, st.s));
  PB_TRY(probe::up(d_clr.p, clr, n_clr * 8, st.s));
  PB_TRY(probe::up(d_set.p, set, n_set * 8, st.s));
  PB_TRY(probe::fill(d_dst, fill, st.s));
  PB_TRY(probe::fill(d_counts, fill, st.s));
  PB_TRY(probe::up(d_counts.p, counts_io, (size_t)n * 8, st.s));
  PB_WAIT(st.s);
  PB_TRY(vk::launch_filter_delta_copy(d_items.as<uint64_t>(), n, max_dst_words, st.s));
  if (!stop_after_copy) {
    PB_TRY(vk::launch_filter_delta_apply(d_items.as<uint64_t>(), d_clr.as<uint64_t>(), n_clr, 0, d_counts.as<unsigned long long>(), st.s));
    PB_TRY(vk::launch_filter_delta_apply(d_items.as<uint64_t>(), d_set.as<uint64_t>(), n_set, 1, d_counts.as<unsigned long long>(), st.s));
  }
  PB_WAIT(st.s);
  PB_TRY(probe::down(out_dst, d_dst.p, off[n] * 8));
  PB_TRY(probe::down(counts_io, d_counts.p, ((size_t)n + kPad) * 8));
  return 0;
}
