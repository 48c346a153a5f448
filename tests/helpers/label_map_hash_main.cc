// label_map_hash_main.cc -- TEST INFRASTRUCTURE (tests/test_label_map_model_cpu.py): a stand-alone host program over
// valkey-search_amd/csrc/label_map_hash.hpp, the header the device label map's kernels share with the host.  It prints
//   mix <label> <label_map_mix>
//   bucket <label> <capacity> <label_map_bucket>
//   capacity <count> <label_map_capacity>
// for the labels and counts on its command line (decimal u64; "-c" switches from labels to counts), so that a test can hold
// its restated hash against the header's.  Built with -fsanitize=address,undefined: the header's shifts and multiplies must be
// clean under UBSan.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "label_map_hash.hpp"

int main(int argc, char **argv) {
  static const uint64_t caps[] = {16, 128, 512, 1ull << 14, 1ull << 25, 1ull << 32};
  bool counts = false;
  for (int i = 1; i < argc; ++i) {
    if (strcmp(argv[i], "-c") == 0) { counts = true; continue; }
    const uint64_t v = strtoull(argv[i], nullptr, 10);
    if (counts) {
      printf("capacity %" PRIu64 " %" PRIu64 "\n", v, vk::label_map_capacity(v));
      continue;
    }
    printf("mix %" PRIu64 " %" PRIu64 "\n", v, vk::label_map_mix(v));
    for (uint64_t c : caps) printf("bucket %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", v, c, vk::label_map_bucket(v, c));
  }
  return 0;
}
