// label_map_hash.hpp -- the hash and the sizing rule of the device label map (label_map.hip), shared by host and device so
// that a test can restate them (tests/helpers/label_map_cases.py) and a stand-alone host program can print them
// (tests/helpers/label_map_hash_main.cc).  No HIP header in here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VK_LM_HD __host__ __device__
#else
#define VK_LM_HD
#endif

namespace vk {

constexpr uint64_t kLabelMapEmpty = ~0ull;         // the empty key: a label the index refuses at the door
constexpr uint32_t kLabelMapNone = 0xFFFFFFFFu;    // "unknown label" where a slot is expected
constexpr uint64_t kLabelMapMinCapacity = 16;
constexpr uint64_t kLabelMapMaxCapacity = 1ull << 32;

// the fixed 64-bit mix (the finaliser of splitmix64): every input bit reaches every bucket bit
VK_LM_HD inline uint64_t label_map_mix(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}
// the first bucket of a label's probe run; capacity is a power of two
VK_LM_HD inline uint64_t label_map_bucket(uint64_t label, uint64_t capacity) { return label_map_mix(label) & (capacity - 1); }

// the smallest capacity the map of `count` published slots gets: a power of two, at least twice the count
inline uint64_t label_map_capacity(uint64_t count) {
  uint64_t c = kLabelMapMinCapacity;
  while (c < 2 * count) c <<= 1;
  return c;
}

}  // namespace vk
