// san_label_map_delta_main.cc -- TEST INFRASTRUCTURE (tests/test_label_map_delta_host_cpu.py): a stand-alone program that
// drives valkey-search_amd/csrc/label_map_delta_host.hpp (no HIP in it) under -fsanitize=address,undefined.
//
//   the touched set     duplicates kept until net_delta, the overflow to "everything" (touch and touch_many, a limit lowered
//                       below what is held), take() empties it, writers on several threads
//   net_delta           deduplicated, one record per label, slots from the truth, the empty key dropped, upserts / erases
//   the decision        every branch of label_map_plan, at and around each threshold
//   the self-check      random worlds: an index (label -> slot) and a host copy of the table go through write phases; the
//                       records of the touched labels are applied by a host restatement of the kernel's rules and the counters
//                       must add up -- and a phase with ONE touched label deliberately left out must be caught, whenever that
//                       label changed the number of live entries
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <thread>
#include <unordered_map>
#include <unordered_set>

#include "label_map_delta_host.hpp"

using namespace vk;

static int g_bad = 0;
#define EXPECT(cond) do { if (!(cond)) { ++g_bad; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

// the kernel's rules on a host copy: keys the table holds (dead ones with kLabelMapNone), counters as the launch leaves them
struct HostTable {
  std::unordered_map<uint64_t, uint32_t> keys;
  uint64_t capacity = 0;
  LabelMapApplied apply(const LabelMapDelta &d) {
    LabelMapApplied c;
    for (size_t i = 0; i < d.labels.size(); ++i) {
      const uint64_t l = d.labels[i];
      const uint32_t s = d.slots[i];
      auto it = keys.find(l);
      if (l == kLabelMapEmpty) { c.fail += 1; continue; }
      if (it == keys.end()) {
        if (keys.size() == capacity) { c.fail += 1; continue; }
        if (s == kLabelMapNone) continue;
        keys.emplace(l, s);
        c.claimed += 1;
        continue;
      }
      const uint32_t old = it->second;
      it->second = s;
      if (old == kLabelMapNone && s != kLabelMapNone) c.revived += 1;
      else if (old != kLabelMapNone && s == kLabelMapNone) c.killed += 1;
      else if (old != s) c.moved += 1;
    }
    return c;
  }
  uint64_t live() const {
    uint64_t n = 0;
    for (auto &kv : keys) n += kv.second != kLabelMapNone;
    return n;
  }
};

static void touched_set() {
  LabelTouchSet t;
  std::vector<uint64_t> got;
  bool all = true;
  EXPECT(t.empty());
  for (int r = 0; r < 3; ++r)
    for (uint64_t l = 0; l < 10; ++l) t.touch(l);
  EXPECT(!t.empty());
  t.take(&got, &all);
  EXPECT(got.size() == 30 && !all && t.empty());
  t.set_max(8);
  for (uint64_t l = 0; l < 8; ++l) t.touch(l);
  t.take(&got, &all);
  EXPECT(got.size() == 8 && !all);
  for (uint64_t l = 0; l < 9; ++l) t.touch(l);      // the ninth label tips it over
  t.touch(77);
  t.take(&got, &all);
  EXPECT(got.empty() && all && t.empty());
  const uint64_t many[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  t.touch_many(many, 8);
  t.take(&got, &all);
  EXPECT(got.size() == 8 && !all);
  t.touch_many(many, 5);
  t.touch_many(many, 4);                            // 9 > 8
  t.take(&got, &all);
  EXPECT(got.empty() && all);
  t.touch_many(many, 0);
  EXPECT(t.empty());
  t.touch_many(many, 6);
  t.set_max(4);                                     // a limit lowered below what is held
  t.take(&got, &all);
  EXPECT(got.empty() && all);
  t.set_all();
  EXPECT(!t.empty());
  t.clear();
  EXPECT(t.empty());
  // writers side by side (the set has its own mutex)
  t.set_max(1u << 20);
  std::vector<std::thread> ws;
  for (int w = 0; w < 4; ++w)
    ws.emplace_back([&t, w] {
      for (uint64_t i = 0; i < 5000; ++i) t.touch((uint64_t)w << 32 | i);
    });
  for (auto &w : ws) w.join();
  t.take(&got, &all);
  EXPECT(got.size() == 20000 && !all);
}

static void net_delta() {
  std::vector<uint64_t> touched = {9, 3, 3, kLabelMapEmpty, 9, 5, 1, 3};
  LabelMapDelta d;
  int calls = 0;
  label_map_net_delta(&touched, [&](uint64_t l) -> uint32_t { ++calls; return l == 3 || l == 1 ? (uint32_t)(l * 10) : kLabelMapNone; }, &d);
  EXPECT(calls == 4 && d.labels.size() == 4 && d.slots.size() == 4 && d.upserts == 2 && d.erases == 2);
  for (size_t i = 0; i < d.labels.size(); ++i) {
    EXPECT(d.labels[i] != kLabelMapEmpty);
    EXPECT(d.slots[i] == (d.labels[i] == 3 || d.labels[i] == 1 ? (uint32_t)(d.labels[i] * 10) : kLabelMapNone));
    for (size_t j = 0; j < i; ++j) EXPECT(d.labels[j] != d.labels[i]);
  }
  std::vector<uint64_t> none;
  label_map_net_delta(&none, [](uint64_t) -> uint32_t { return 0; }, &d);
  EXPECT(d.labels.empty() && d.upserts == 0 && d.erases == 0);
}

static void decision() {
  LabelMapState m;
  EXPECT(label_map_plan(m, false, 0, 0) == LabelMapPlan::kRebuildNoMap);
  m.usable = true;
  EXPECT(label_map_plan(m, false, 0, 0) == LabelMapPlan::kRebuildNoMap);      // usable, but no table
  m.capacity = 64;
  m.used = 20;
  m.live = 18;
  EXPECT(label_map_plan(m, false, 0, 20) == LabelMapPlan::kApply);
  EXPECT(label_map_plan(m, true, 0, 20) == LabelMapPlan::kRebuildEverything);
  EXPECT(label_map_plan(m, false, 12, 20) == LabelMapPlan::kApply);           // 20 + 12 == 32: the load is one half exactly
  EXPECT(label_map_plan(m, false, 13, 20) == LabelMapPlan::kRebuildLoad);
  m.used = 32;                                                                  // dead keys count
  m.live = 3;
  EXPECT(label_map_plan(m, false, 0, 3) == LabelMapPlan::kApply);
  EXPECT(label_map_plan(m, false, 1, 3) == LabelMapPlan::kRebuildLoad);
  m.used = 10;
  EXPECT(label_map_plan(m, false, 0, 32) == LabelMapPlan::kApply);            // 64 == 2 x 32
  EXPECT(label_map_plan(m, false, 0, 33) == LabelMapPlan::kRebuildSmall);     // HNSW: tombstoned slots count
  m.usable = false;
  EXPECT(label_map_plan(m, true, 99, 33) == LabelMapPlan::kRebuildNoMap);
  // the arithmetic of the check on its own
  uint64_t after = 0;
  LabelMapApplied c;
  EXPECT(label_map_check_applied(10, c, 10, &after) && after == 10);
  c.claimed = 3;
  c.revived = 1;
  c.killed = 2;
  c.moved = 7;
  EXPECT(label_map_check_applied(10, c, 12, &after) && after == 12);
  EXPECT(!label_map_check_applied(10, c, 11, &after));
  c.fail = 1;
  EXPECT(!label_map_check_applied(10, c, 12, &after));
  c = LabelMapApplied();
  c.killed = 5;
  EXPECT(!label_map_check_applied(3, c, 0, &after));                           // more killed than there were: never "equal" by wrap-around
}

static void self_check(uint32_t seed, int worlds, int *caught, int *silent) {
  std::mt19937_64 rng(seed);
  for (int w = 0; w < worlds; ++w) {
    std::unordered_map<uint64_t, uint32_t> index;   // the truth: FLAT's slot_of_, dense slots
    std::vector<uint64_t> by_slot;
    HostTable table;
    table.capacity = 256;
    uint64_t live = 0;
    const bool leave_one_out = w % 2 == 1;
    for (int phase = 0; phase < 12; ++phase) {
      std::vector<uint64_t> touched;
      const int ops = 1 + (int)(rng() % 12);
      for (int o = 0; o < ops; ++o) {
        const uint64_t label = rng() % 40;
        auto it = index.find(label);
        if (it == index.end() && (rng() & 1)) {           // add
          index.emplace(label, (uint32_t)by_slot.size());
          by_slot.push_back(label);
          touched.push_back(label);
        } else if (it != index.end()) {                   // remove: the last row fills the hole
          const uint32_t cur = it->second, last = (uint32_t)by_slot.size() - 1;
          index.erase(it);
          touched.push_back(label);
          if (cur != last) {
            by_slot[cur] = by_slot[last];
            index[by_slot[cur]] = cur;
            touched.push_back(by_slot[cur]);
          }
          by_slot.pop_back();
        }
      }
      bool dropped_matters = false;
      if (leave_one_out && phase == 7 && !touched.empty()) {
        const uint64_t drop = touched[rng() % touched.size()];
        std::vector<uint64_t> kept;
        for (uint64_t l : touched)
          if (l != drop) kept.push_back(l);
        touched.swap(kept);
        // the check counts live entries: it sees a missing label whose presence changed (a missing MOVE it cannot see --
        // that is what the tests through the index are for)
        const bool in_index = index.count(drop) != 0;
        auto tk = table.keys.find(drop);
        const bool in_table = tk != table.keys.end() && tk->second != kLabelMapNone;
        dropped_matters = in_index != in_table;
      }
      LabelMapDelta d;
      label_map_net_delta(&touched, [&](uint64_t l) -> uint32_t {
        auto it = index.find(l);
        return it == index.end() ? kLabelMapNone : it->second;
      }, &d);
      const LabelMapApplied c = table.apply(d);
      uint64_t after = 0;
      const bool ok = label_map_check_applied(live, c, index.size(), &after);
      if (leave_one_out && phase == 7) {
        if (dropped_matters) { EXPECT(!ok); *caught += !ok; }
        else { EXPECT(ok); *silent += 1; }
        break;   // (a real index rebuilds here)
      }
      EXPECT(ok && after == index.size() && table.live() == index.size());
      live = after;
      for (auto &kv : index) {
        auto it = table.keys.find(kv.first);
        EXPECT(it != table.keys.end() && it->second == kv.second);
      }
    }
  }
}

int main(int argc, char **argv) {
  const uint32_t seed = argc > 1 ? (uint32_t)strtoul(argv[1], nullptr, 10) : 1;
  const int worlds = argc > 2 ? atoi(argv[2]) : 400;
  touched_set();
  net_delta();
  decision();
  int caught = 0, silent = 0;
  self_check(seed, worlds, &caught, &silent);
  printf("worlds=%d caught=%d silent=%d bad=%d\n", worlds, caught, silent, g_bad);
  return g_bad ? 1 : 0;
}
