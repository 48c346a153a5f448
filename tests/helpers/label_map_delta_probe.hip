// label_map_delta_probe.hip -- TEST INFRASTRUCTURE (tests/test_label_map_delta_kernels_gpu.py), not part of libvkindex.so.
//
// The apply launch of the device label map (label_map_apply_kernel, valkey-search_amd/csrc/label_map.hip; option
// prefilter-label-map-upkeep) on buffers the test owns.  Like label_map_probe.hip this probe includes that translation unit
// itself (compile with -I valkey-search_amd/csrc and the library's flags), so the product's kernels and launchers are what
// runs.  One call is a build, then a SEQUENCE of apply launches -- each waited for before the next, as DeviceLabelMap::ready
// does -- then one resolve of a shared key list against the table they left.  Before the build every buffer the kernels
// touch -- the table with its failure word and counters, the record scratch, the resolve's outputs and scratch -- is filled
// with a word of the caller's choice; only what the product's launchers initialise themselves is initialised.  The probe
// never blocks on a launch: it polls the stream with a time limit and reports a timeout (return code 2) as a failure,
// leaving its buffers where they are.
#include "label_map.hip"

#include <algorithm>
#include <chrono>
#include <thread>
#include <vector>

namespace {

bool g_leak = false;   // after a timeout: a hipFree would wait for the kernel the probe gave up on

struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (!g_leak) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
  template <class T> T *as() const { return static_cast<T *>(p); }
};
struct Stream {
  hipStream_t s = nullptr;
  ~Stream() { if (s && !g_leak) (void)hipStreamDestroy(s); }
};

#define LM_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)
#define LM_WAIT(stream) do { const int _w = wait_for(stream, __LINE__); if (_w) return _w; } while (0)

constexpr int kTimeout = 2;
constexpr double kLimitSeconds = 20.0;

int wait_for(hipStream_t s, int line) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipStreamQuery(s);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotReady) return line;
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kLimitSeconds) {
      g_leak = true;
      return kTimeout;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

hipError_t fill_words(void *p, size_t words, uint32_t fill, hipStream_t s) {
  return words ? hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)fill, words, s) : hipSuccess;
}

}  // namespace

extern "C" uint64_t lmd_probe_max_blocks() { return vk::kLabelMapApplyMaxBlocks; }

// A build, n_launch apply launches, one resolve of the shared list keys[0 .. n_keys).
//   labels [count], links0 [count * l0_stride] or NULL, capacity a power of two >= 16 and >= 2 * count
//   launch l applies the records rec_labels / rec_slots [launch_begin[l] .. launch_begin[l + 1])
//   out_words [n_launch][5]: the failure word and the four counters as launch l left them
//   out_keys / out_vals [capacity]: the table behind the last launch; out_build_fail [1]: the build's failure word
//   out_seg / out_tile [2], out_slot / out_pos [n_keys] (what lies past out_seg[1] is the fill word)
// Returns 0, 1 = arguments refused, 2 = a launch did not finish within the time limit, or the source line that saw a HIP error.
extern "C" int lmd_probe_run(uint32_t fill, const uint64_t *labels, uint32_t count, const uint32_t *links0, uint32_t l0_stride, uint64_t capacity,
                             const uint64_t *rec_labels, const uint32_t *rec_slots, const uint32_t *launch_begin, uint32_t n_launch,
                             uint32_t *out_build_fail, uint32_t *out_words, uint64_t *out_keys, uint32_t *out_vals, const uint64_t *keys,
                             uint32_t n_keys, uint32_t *out_seg, uint32_t *out_tile, uint32_t *out_slot, uint32_t *out_pos) {
  if (g_leak) return 1;
  if (capacity < vk::label_map_capacity(count) || capacity > (1ull << 26) || (capacity & (capacity - 1))) return 1;
  if (links0 && l0_stride == 0) return 1;
  uint32_t max_records = 0;
  for (uint32_t l = 0; l < n_launch; ++l) {
    if (launch_begin[l + 1] < launch_begin[l]) return 1;
    max_records = std::max(max_records, launch_begin[l + 1] - launch_begin[l]);
  }
  if (n_launch && launch_begin[0] != 0) return 1;
  Stream st;
  LM_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
  DevBuf d_labels, d_links, d_table, d_rec, d_keys, d_csr, d_out;
  LM_TRY(d_labels.alloc((size_t)count * 8));
  if (count) LM_TRY(hipMemcpy(d_labels.p, labels, (size_t)count * 8, hipMemcpyHostToDevice));
  if (links0) {
    LM_TRY(d_links.alloc((size_t)count * l0_stride * 4));
    if (count) LM_TRY(hipMemcpy(d_links.p, links0, (size_t)count * l0_stride * 4, hipMemcpyHostToDevice));
  }
  // the table: keys | values | the failure word and the four counters, dirty
  const size_t table_words = (size_t)capacity * 3 + 8;
  LM_TRY(d_table.alloc(table_words * 4));
  LM_TRY(fill_words(d_table.p, table_words, fill, st.s));
  vk::LabelMapTable t{};
  t.keys = d_table.as<uint64_t>();
  t.vals = reinterpret_cast<uint32_t *>(t.keys + capacity);
  t.fail = reinterpret_cast<unsigned int *>(t.vals + capacity);
  t.capacity = capacity;
  vk::LabelMapBuildArgs b{};
  b.t = t;
  b.labels = d_labels.as<uint64_t>();
  b.links0 = links0 ? d_links.as<uint32_t>() : nullptr;
  b.l0_stride = l0_stride;
  b.count = count;
  LM_TRY(vk::launch_label_map_build(b, st.s));
  LM_WAIT(st.s);
  LM_TRY(hipMemcpy(out_build_fail, t.fail, 4, hipMemcpyDeviceToHost));
  // the record scratch: [labels | slots] of the longest launch, dirty; launch after launch, each waited for
  const size_t rec_words = (size_t)max_records * 3;
  LM_TRY(d_rec.alloc(rec_words * 4));
  LM_TRY(fill_words(d_rec.p, rec_words, fill, st.s));
  LM_WAIT(st.s);
  for (uint32_t l = 0; l < n_launch; ++l) {
    const uint32_t lo = launch_begin[l], n = launch_begin[l + 1] - lo;
    vk::LabelMapApplyArgs a{};
    a.t = t;
    a.labels = d_rec.as<uint64_t>();
    a.slots = reinterpret_cast<const uint32_t *>(d_rec.as<uint64_t>() + n);
    a.n = n;
    a.counters = t.fail + 1;
    if (n) {
      LM_TRY(hipMemcpy(d_rec.p, rec_labels + lo, (size_t)n * 8, hipMemcpyHostToDevice));
      LM_TRY(hipMemcpy(d_rec.as<uint64_t>() + n, rec_slots + lo, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    LM_TRY(vk::launch_label_map_apply(a, st.s));
    LM_WAIT(st.s);
    LM_TRY(hipMemcpy(out_words + (size_t)l * 5, t.fail, 20, hipMemcpyDeviceToHost));
  }
  LM_TRY(hipMemcpy(out_keys, t.keys, (size_t)capacity * 8, hipMemcpyDeviceToHost));
  LM_TRY(hipMemcpy(out_vals, t.vals, (size_t)capacity * 4, hipMemcpyDeviceToHost));
  // the resolve of one shared list: [seg_begin | tile_begin | slot | pos | raw | tile_off], dirty
  const uint32_t n_ktiles = vk::label_map_key_tiles(n_keys);
  const uint32_t h_csr[4] = {0, n_keys, 0, n_ktiles};
  const size_t out_words_n = 4 + 3 * (size_t)n_keys + n_ktiles + 1;
  LM_TRY(d_keys.alloc((size_t)n_keys * 8));
  if (n_keys) LM_TRY(hipMemcpy(d_keys.p, keys, (size_t)n_keys * 8, hipMemcpyHostToDevice));
  LM_TRY(d_csr.alloc(16));
  LM_TRY(hipMemcpy(d_csr.p, h_csr, 16, hipMemcpyHostToDevice));
  LM_TRY(d_out.alloc(out_words_n * 4));
  LM_TRY(fill_words(d_out.p, out_words_n, fill, st.s));
  vk::LabelMapResolveArgs r{};
  r.t = t;
  r.keys = d_keys.as<uint64_t>();
  r.list_begin = d_csr.as<uint32_t>();
  r.ktile_begin = r.list_begin + 2;
  r.n_seg = 1;
  r.n_keys = n_keys;
  r.n_ktiles = n_ktiles;
  r.seg_begin = d_out.as<uint32_t>();
  r.tile_begin = r.seg_begin + 2;
  r.slot = r.tile_begin + 2;
  r.pos = r.slot + n_keys;
  r.raw = r.pos + n_keys;
  r.tile_off = r.raw + n_keys;
  LM_TRY(vk::launch_label_map_resolve(r, st.s));
  LM_WAIT(st.s);
  LM_TRY(hipMemcpy(out_seg, r.seg_begin, 8, hipMemcpyDeviceToHost));
  LM_TRY(hipMemcpy(out_tile, r.tile_begin, 8, hipMemcpyDeviceToHost));
  if (n_keys) {
    LM_TRY(hipMemcpy(out_slot, r.slot, (size_t)n_keys * 4, hipMemcpyDeviceToHost));
    LM_TRY(hipMemcpy(out_pos, r.pos, (size_t)n_keys * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}
