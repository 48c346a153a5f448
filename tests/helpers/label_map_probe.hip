// label_map_probe.hip -- TEST INFRASTRUCTURE (tests/test_label_map_kernels_gpu.py), not part of libvkindex.so.
//
// The device label map (valkey-search_amd/csrc/label_map.hip) is reachable through the C ABI only behind the pre-filter
// search, whose answers hide most of what the kernels write.  This probe includes that translation unit itself (compile with
// -I valkey-search_amd/csrc and the library's flags), so the product's kernels and launchers are what runs, on buffers the
// test owns: one build, then one resolve of a CSR of key lists, and everything they wrote comes back.  Before the build every
// buffer the kernels touch -- the table, the outputs, the scratch -- is filled with a word of the caller's choice; only what
// the product's launchers initialise themselves is initialised.  The probe never blocks on a launch: it polls the stream
// with a time limit and reports a timeout (return code 2) as a failure, leaving its buffers where they are.
#include "label_map.hip"

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

extern "C" uint64_t lm_probe_capacity(uint64_t count) { return vk::label_map_capacity(count); }
extern "C" uint64_t lm_probe_bucket(uint64_t label, uint64_t capacity) { return vk::label_map_bucket(label, capacity); }
extern "C" uint32_t lm_probe_key_tiles(uint64_t keys) { return vk::label_map_key_tiles(keys); }

// One build, then (n_seg > 0) one resolve.
//   labels [count], links0 [count * l0_stride] or NULL, capacity as label_map_capacity gives it or larger
//   out_keys / out_vals [capacity], out_fail [1]: the table as the build left it
//   keys [n_keys], list_begin [n_seg + 1] from 0 to n_keys ascending (a shared list: n_seg = 1)
//   out_seg / out_tile [n_seg + 1], out_slot / out_pos [n_keys] (what lies past out_seg[n_seg] is the fill word)
// Returns 0, 1 = arguments refused, 2 = a launch did not finish within the time limit, or the source line that saw a HIP error.
extern "C" int lm_probe_run(uint32_t fill, const uint64_t *labels, uint32_t count, const uint32_t *links0, uint32_t l0_stride, uint64_t capacity,
                            uint64_t *out_keys, uint32_t *out_vals, uint32_t *out_fail, const uint64_t *keys, uint32_t n_keys,
                            const uint32_t *list_begin, uint32_t n_seg, uint32_t *out_seg, uint32_t *out_tile, uint32_t *out_slot,
                            uint32_t *out_pos) {
  if (g_leak) return 1;
  if (capacity < vk::label_map_capacity(count) || capacity > (1ull << 26) || (capacity & (capacity - 1))) return 1;
  if (links0 && l0_stride == 0) return 1;
  std::vector<uint32_t> ktile(n_seg + 1, 0);
  if (n_seg) {
    if (list_begin[0] != 0 || list_begin[n_seg] != n_keys) return 1;
    for (uint32_t s = 0; s < n_seg; ++s) {
      if (list_begin[s + 1] < list_begin[s]) return 1;
      ktile[s + 1] = ktile[s] + vk::label_map_key_tiles(list_begin[s + 1] - list_begin[s]);
    }
  }
  const uint32_t n_ktiles = ktile[n_seg];
  Stream st;
  LM_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
  DevBuf d_labels, d_links, d_table, d_keys, d_csr, d_out;
  LM_TRY(d_labels.alloc((size_t)count * 8));
  if (count) LM_TRY(hipMemcpy(d_labels.p, labels, (size_t)count * 8, hipMemcpyHostToDevice));
  if (links0) {
    LM_TRY(d_links.alloc((size_t)count * l0_stride * 4));
    if (count) LM_TRY(hipMemcpy(d_links.p, links0, (size_t)count * l0_stride * 4, hipMemcpyHostToDevice));
  }
  // the table: keys | values | the failure word, dirty
  const size_t table_words = (size_t)capacity * 3 + 4;
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
  LM_TRY(hipMemcpy(out_keys, t.keys, (size_t)capacity * 8, hipMemcpyDeviceToHost));
  LM_TRY(hipMemcpy(out_vals, t.vals, (size_t)capacity * 4, hipMemcpyDeviceToHost));
  LM_TRY(hipMemcpy(out_fail, t.fail, 4, hipMemcpyDeviceToHost));
  if (n_seg == 0) return 0;
  // the resolve: [seg_begin | tile_begin | slot | pos | raw | tile_off], dirty
  const size_t csr = (size_t)n_seg + 1, out_words = 2 * csr + 3 * (size_t)n_keys + n_ktiles + 1;
  LM_TRY(d_keys.alloc((size_t)n_keys * 8));
  if (n_keys) LM_TRY(hipMemcpy(d_keys.p, keys, (size_t)n_keys * 8, hipMemcpyHostToDevice));
  LM_TRY(d_csr.alloc(2 * csr * 4));
  LM_TRY(hipMemcpy(d_csr.p, list_begin, csr * 4, hipMemcpyHostToDevice));
  LM_TRY(hipMemcpy(d_csr.as<uint32_t>() + csr, ktile.data(), csr * 4, hipMemcpyHostToDevice));
  LM_TRY(d_out.alloc(out_words * 4));
  LM_TRY(fill_words(d_out.p, out_words, fill, st.s));
  vk::LabelMapResolveArgs r{};
  r.t = t;
  r.keys = d_keys.as<uint64_t>();
  r.list_begin = d_csr.as<uint32_t>();
  r.ktile_begin = r.list_begin + csr;
  r.n_seg = n_seg;
  r.n_keys = n_keys;
  r.n_ktiles = n_ktiles;
  r.seg_begin = d_out.as<uint32_t>();
  r.tile_begin = r.seg_begin + csr;
  r.slot = r.tile_begin + csr;
  r.pos = r.slot + n_keys;
  r.raw = r.pos + n_keys;
  r.tile_off = r.raw + n_keys;
  LM_TRY(vk::launch_label_map_resolve(r, st.s));
  LM_WAIT(st.s);
  LM_TRY(hipMemcpy(out_seg, r.seg_begin, csr * 4, hipMemcpyDeviceToHost));
  LM_TRY(hipMemcpy(out_tile, r.tile_begin, csr * 4, hipMemcpyDeviceToHost));
  if (n_keys) {
    LM_TRY(hipMemcpy(out_slot, r.slot, (size_t)n_keys * 4, hipMemcpyDeviceToHost));
    LM_TRY(hipMemcpy(out_pos, r.pos, (size_t)n_keys * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}
