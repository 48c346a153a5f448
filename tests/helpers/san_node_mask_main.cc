// san_node_mask_main.cc -- TEST INFRASTRUCTURE: the bookkeeping of the HNSW node masks (csrc/node_mask_cache.hpp) under the
// sanitizers.  The header makes no HIP call: "device memory" here is malloc'ed, the free function counts.
//   1. least recently used first out, and a hit makes an entry the most recent one
//   2. an entry of another epoch is dropped where it is met; drop_stale() drops them all
//   3. the byte budget: reserve() evicts down to it, counts evictions, never exceeds it
//   4. the fallback decision: a mask larger than the budget, or one that would need an entry the same batch holds, gets no
//      room and NOTHING is evicted for it; unreserve() gives the room back
//   5. two batches that built the same mask: the first stays, the second's memory is freed
//   6. a Ref outlives eviction and clear(): the memory goes with the last holder, exactly once
//   7. get / reserve / put / drop_stale / clear from several threads: every block freed exactly once, the resident bytes
//      never above the budget when observed, no reserved bytes left behind
// Prints "bad=<n>"; any sanitizer report fails the test that runs this.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "node_mask_cache.hpp"

using vk::NodeMaskCache;

static std::atomic<long> g_live{0}, g_freed{0};
static void free_block(void *, uint64_t *p) {
  g_freed += 1;
  g_live -= 1;
  free(p);
}
static uint64_t *block(uint64_t bytes) {
  g_live += 1;
  return static_cast<uint64_t *>(calloc(1, bytes));
}

static int bad = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      fprintf(stderr, "line %d: %s\n", __LINE__, #x);              \
      bad += 1;                                                    \
    }                                                              \
  } while (0)

static std::vector<uint64_t> order(const NodeMaskCache &c) {
  std::vector<uint64_t> ids;
  c.for_each([&](const vk::NodeMask &m) { ids.push_back(m.filter_id); });
  return ids;
}

static bool build(NodeMaskCache &c, uint64_t id, uint64_t epoch, uint64_t bytes, uint64_t budget, uint64_t batch, NodeMaskCache::Ref *out = nullptr) {
  if (!c.reserve(bytes, budget, batch)) return false;
  NodeMaskCache::Ref r = c.put(id, epoch, block(bytes), bytes, id * 10, batch);
  if (out) *out = r;
  return true;
}

static void single_threaded() {
  const uint64_t B = 64, budget = 3 * B;
  {
    NodeMaskCache c(free_block, nullptr);
    for (uint64_t id = 1; id <= 3; ++id) CHECK(build(c, id, 1, B, budget, c.begin_batch()));
    CHECK((order(c) == std::vector<uint64_t>{3, 2, 1}));
    CHECK(c.get(1, 1, c.begin_batch()) != nullptr);                 // 1. a hit: most recent
    CHECK((order(c) == std::vector<uint64_t>{1, 3, 2}));
    CHECK(build(c, 4, 1, B, budget, c.begin_batch()));              //    room for 4: the least recent (2) goes
    CHECK((order(c) == std::vector<uint64_t>{4, 1, 3}));
    CHECK(c.counters().evictions == 1 && c.counters().bytes == 3 * B && c.counters().entries == 3);
    CHECK(c.get(2, 1, c.begin_batch()) == nullptr);
    CHECK(c.get(3, 2, c.begin_batch()) == nullptr);                 // 2. another epoch: dropped on sight, not an eviction
    CHECK((order(c) == std::vector<uint64_t>{4, 1}) && c.counters().evictions == 1);
    CHECK(build(c, 5, 2, B, budget, c.begin_batch()));
    c.drop_stale(2);
    CHECK((order(c) == std::vector<uint64_t>{5}) && c.counters().bytes == B);
    CHECK(c.get(5, 2, c.begin_batch())->admitted == 50);
    CHECK(c.counters().hits == 2 && c.counters().built == 5);
  }
  CHECK(g_live == 0);
  {
    NodeMaskCache c(free_block, nullptr);
    CHECK(!c.reserve(budget + 1, budget, c.begin_batch()));         // 4. larger than the budget
    const uint64_t batch = c.begin_batch();
    CHECK(build(c, 1, 1, B, budget, batch) && build(c, 2, 1, B, budget, batch) && build(c, 3, 1, B, budget, batch));
    CHECK(!c.reserve(B, budget, batch));                            //    the batch holds all three: no room, nothing evicted
    CHECK(c.counters().entries == 3 && c.counters().evictions == 0);
    const uint64_t next = c.begin_batch();
    CHECK(c.get(3, 1, next) != nullptr);
    CHECK(!c.reserve(3 * B, budget, next));                         //    3 is held by this batch: only 2 B can be freed
    CHECK(c.counters().entries == 3 && c.counters().evictions == 0);
    CHECK(c.reserve(2 * B, budget, next));                          // 3. evicts 1 and 2, keeps 3
    CHECK((order(c) == std::vector<uint64_t>{3}) && c.counters().evictions == 2);
    c.unreserve(2 * B);
    CHECK(c.reserve(2 * B, budget, c.begin_batch()));               //    the room came back
    c.unreserve(2 * B);
    // 5. the same mask built twice
    const uint64_t b1 = c.begin_batch(), b2 = c.begin_batch();
    CHECK(c.reserve(B, budget, b1) && c.reserve(B, budget, b2));
    NodeMaskCache::Ref first = c.put(9, 1, block(B), B, 1, b1);
    const long freed = g_freed;
    NodeMaskCache::Ref second = c.put(9, 1, block(B), B, 2, b2);
    CHECK(first == second && second->admitted == 1 && g_freed == freed + 1);
    CHECK(c.counters().bytes == 2 * B && c.counters().entries == 2);
    // 6. a holder outlives the cache's entry
    NodeMaskCache::Ref held = c.get(3, 1, c.begin_batch());
    const long before = g_freed;
    c.clear();
    CHECK(c.counters().entries == 0 && c.counters().bytes == 0);
    CHECK(g_freed == before);                                       //    3 and 9 are still held
    first.reset();
    second.reset();
    CHECK(g_freed == before + 1);
    held->bits[0] = 7;                                              //    (still ours to touch: ASAN would say otherwise)
    held.reset();
    CHECK(g_freed == before + 2);
    NodeMaskCache::Ref outside = c.make(77, 1, block(B), B, 3);     //    a mask outside the cache: same ownership
    CHECK(c.counters().entries == 0);
    outside.reset();
  }
  CHECK(g_live == 0);
}

static void many_threads(int threads, int rounds) {
  const uint64_t B = 128, budget = 6 * B;
  std::atomic<uint64_t> epoch{1};
  std::atomic<int> over{0};
  {
    NodeMaskCache c(free_block, nullptr);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
      pool.emplace_back([&, t] {
        unsigned s = 12345u + (unsigned)t * 977u;
        auto rnd = [&] { s = s * 1664525u + 1013904223u; return s >> 8; };
        for (int r = 0; r < rounds; ++r) {
          const uint64_t batch = c.begin_batch(), e = epoch.load();
          std::vector<NodeMaskCache::Ref> mine;
          for (int i = 0; i < 3; ++i) {
            const uint64_t id = 1 + rnd() % 16;
            NodeMaskCache::Ref ref = c.get(id, e, batch);
            if (!ref && c.reserve(B, budget, batch)) {
              if (rnd() % 8 == 0) c.unreserve(B);                   // (the allocation failed)
              else ref = c.put(id, e, block(B), B, id, batch);
            }
            if (ref) {
              if (ref->filter_id != id || ref->admitted != id) over += 1;
              (void)__atomic_load_n(ref->bits, __ATOMIC_RELAXED);   // a search reads its mask
              mine.push_back(ref);
            }
          }
          if (c.counters().bytes > budget) over += 1;
          if (t == 0 && r % 64 == 63) c.drop_stale(epoch.fetch_add(1) + 1);
          if (t == 1 && r % 257 == 256) c.clear();
        }
      });
    for (auto &th : pool) th.join();
    CHECK(over == 0);
    CHECK(c.reserve(budget, budget, c.begin_batch()));              // nothing reserved was left behind
    c.unreserve(budget);
  }
  CHECK(g_live == 0);
}

int main(int argc, char **argv) {
  const int threads = argc > 1 ? atoi(argv[1]) : 6, rounds = argc > 2 ? atoi(argv[2]) : 4000;
  single_threaded();
  many_threads(threads, rounds);
  printf("bad=%d freed=%ld\n", bad, g_freed.load());
  return bad ? 1 : 0;
}
