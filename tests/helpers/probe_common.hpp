// probe_common.hpp -- TEST INFRASTRUCTURE: what tests/helpers/filter_build_probe.hip and tests/helpers/node_mask_probe.hip share.
//
// Device buffers that are freed on every way out but one, a stream, a fill with a 32-bit word, and the wait: a probe never
// blocks on a launch, it polls the stream with a time limit and reports a timeout (return code 2) as a failure.  After a
// timeout nothing is freed (a hipFree would wait for the kernel the probe gave up on) and every later call is refused.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <thread>

namespace probe {

inline bool g_leak = false;

struct DevBuf {
  void *p = nullptr;
  size_t words32 = 0;
  ~DevBuf() { if (!g_leak) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) {
    bytes = (bytes + 7) & ~(size_t)7;
    if (!bytes) bytes = 8;
    words32 = bytes / 4;
    return hipMalloc(&p, bytes);
  }
  template <class T> T *as() const { return static_cast<T *>(p); }
};
struct Stream {
  hipStream_t s = nullptr;
  ~Stream() { if (s && !g_leak) (void)hipStreamDestroy(s); }
};

constexpr int kRefused = 1, kTimeout = 2;
constexpr double kLimitSeconds = 20.0;   // a stop, not a performance claim: these launches take microseconds

inline int wait_for(hipStream_t s, int line) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipStreamQuery(s);
    if (e == hipSuccess) return 0;
    if (e != hipErrorNotReady) return line;
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > kLimitSeconds) {
      g_leak = true;
      return kTimeout;
    }
    std::this_thread::sleep_for(std::chrono::microseconds(100));
  }
}

// the whole buffer <- the fill word, in stream order
inline hipError_t fill(const DevBuf &b, uint32_t word, hipStream_t s) {
  return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b.p), (int)word, b.words32, s);
}
inline hipError_t up(void *dst, const void *src, size_t bytes, hipStream_t s) {   // (pageable source: returns once it is staged)
  return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
}
inline hipError_t down(void *dst, const void *src, size_t bytes) {
  return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
}

}  // namespace probe

#define PB_TRY(expr) do { if ((expr) != hipSuccess) return __LINE__; } while (0)
#define PB_WAIT(stream) do { const int _w = probe::wait_for(stream, __LINE__); if (_w) return _w; } while (0)
