"""What tests/test_label_map_delta_kernels_gpu.py (the device label map's apply launch, through
tests/helpers/label_map_delta_probe.hip) and tests/test_label_map_delta_model_cpu.py (which checks the model against a plain
dict and that every case reaches the path it is named for, without a GPU) share:

  * a model of the table across apply launches: the live entries {label: slot}, the set of dead keys (erased labels keep their
    bucket), and per launch the failure word, the four counters and the path every record took;
  * the cases: a build (labels, tombstones, capacity), a sequence of launches of (label, slot) records -- every label at most
    once per launch, as the host guarantees -- and the key list that is resolved against the table behind the last launch.

The hash, the sizing rule and the build / resolve models are label_map_cases.py's.
"""
from collections import Counter

import numpy as np

import label_map_cases as LM

EMPTY, NONE, M64 = LM.EMPTY, LM.NONE, LM.M64
COUNTERS = ("claimed", "revived", "killed", "moved")      # the kernel's order behind the failure word


class Table:
    """the table as the host may know it: which keys it holds, which of them answer a slot"""

    def __init__(self, capacity, built):
        self.capacity = capacity
        self.live = dict(built)
        self.dead = set()

    def used(self):
        return len(self.live) + len(self.dead)

    def apply(self, records):
        """one launch: (failure word, {counter: n}, Counter of paths).  Paths: claim, revive, kill, move, same (the value
        that is there already), dead_again (an erase of a dead entry), erase_unknown, empty_key, full (a whole turn of the
        table without the key or an empty bucket)."""
        labels = [l for l, _ in records]
        assert len(set(labels)) == len(labels), "a label twice in one launch"
        fail, c, paths = 0, dict.fromkeys(COUNTERS, 0), Counter()
        for label, slot in records:
            if label == EMPTY:
                fail += 1
                paths["empty_key"] += 1
            elif label in self.live:
                old = self.live[label]
                if slot == NONE:
                    del self.live[label]
                    self.dead.add(label)
                    c["killed"] += 1
                    paths["kill"] += 1
                elif slot != old:
                    self.live[label] = slot
                    c["moved"] += 1
                    paths["move"] += 1
                else:
                    paths["same"] += 1
            elif label in self.dead:
                if slot == NONE:
                    paths["dead_again"] += 1
                else:
                    self.dead.remove(label)
                    self.live[label] = slot
                    c["revived"] += 1
                    paths["revive"] += 1
            elif self.used() == self.capacity:
                fail += 1
                paths["full"] += 1
            elif slot == NONE:
                paths["erase_unknown"] += 1
            else:
                self.live[label] = slot
                c["claimed"] += 1
                paths["claim"] += 1
        return fail, c, paths


def occupied_after(labels, capacity):
    """the buckets a linear-probing table holds after these labels went in -- the SET does not depend on the order"""
    occ = set()
    for l in labels:
        h = LM.bucket(l, capacity)
        while h in occ:
            h = (h + 1) % capacity
        occ.add(h)
    return occ


def run_model(case):
    """(table behind the last launch, [per launch (fail, counters, paths)], build failures)"""
    built, fails = LM.build_model(case["labels"], case["tomb"])
    t = Table(case["capacity"], built)
    return t, [t.apply(recs) for recs in case["launches"]], fails


def split_table(keys, vals):
    """the downloaded table as (live {label: slot}, dead key set, used buckets)"""
    used = np.nonzero(keys != np.uint64(EMPTY))[0]
    live = {int(keys[h]): int(vals[h]) for h in used if int(vals[h]) != NONE}
    dead = {int(keys[h]) for h in used if int(vals[h]) == NONE}
    return live, dead, len(used)


RECORD_COUNTS = (0, 1, 256, 257, 70000)


def cases():
    """name -> dict(labels, tomb, capacity, launches, keys, wants): `wants` = paths the case must reach, by launch index"""
    rng = np.random.default_rng(1501)
    out = {}

    def fresh(n, lo=1 << 41):
        return [int(v) for v in lo + rng.choice(1 << 30, size=n, replace=False)]

    # capacity 16, 8 labels, buckets 14 and 15 taken (two labels of bucket 15: the second lies at 0 already): a new label of
    # bucket 15 walks past the table's end
    built = LM.colliding_labels(16, 15, 2) + LM.colliding_labels(16, 14, 1, start=1 << 20) + LM.colliding_labels(16, 5, 5, start=1 << 21)
    new = LM.colliding_labels(16, 15, 1, start=1 << 30)[0]
    out["wrap16"] = dict(labels=built, tomb=None, capacity=16, launches=[[(new, 77)]], keys=built + [new, 12345], wants={0: ["claim"]},
                         wraps=new)
    # two / five new labels with the same first bucket in one launch: the compare-and-swap race, the losers probe on
    for n in (2, 5):
        built = fresh(8)
        cap = 64
        b = next(h for h in range(cap) if h not in occupied_after(built, cap))
        twins = LM.colliding_labels(cap, b, n, start=1 << 33)
        out["race_%d" % n] = dict(labels=built, tomb=None, capacity=cap, launches=[[(l, 100 + i) for i, l in enumerate(twins)]],
                                  keys=twins + built, wants={0: ["claim"]}, same_bucket=(b, twins))
    # erase, then in a later launch the same label again: the same bucket, claimed 0, revived 1
    built = fresh(40)
    out["erase_then_revive"] = dict(labels=built, tomb=None, capacity=LM.capacity_for(40), launches=[[(built[7], NONE)], [(built[7], 41)]],
                                    keys=built, wants={0: ["kill"], 1: ["revive"]})
    # erase of a label the map never held: nothing written, no bucket claimed; and of a dead entry once more
    stranger = fresh(3, lo=1 << 50)
    out["erase_unknown"] = dict(labels=built, tomb=None, capacity=LM.capacity_for(40),
                                launches=[[(s, NONE) for s in stranger], [(built[3], NONE)], [(built[3], NONE), (stranger[0], NONE)]],
                                keys=built + stranger, wants={0: ["erase_unknown"], 2: ["dead_again", "erase_unknown"]})
    # a known label to another slot, and to the slot it has
    out["move"] = dict(labels=built, tomb=None, capacity=LM.capacity_for(40), launches=[[(built[0], 39), (built[39], 0), (built[5], 5)]],
                       keys=built, wants={0: ["move", "same"]})
    # 0, 1, 256, 257 and 70 000 records in one launch (the second block; more records than the grid has threads): new labels
    # with every seventh record an erase of a built label, then a second launch that takes half of it back
    for n in RECORD_COUNTS:
        built = fresh(max(n // 7 + 1, 10), lo=1 << 42)
        new = fresh(n, lo=1 << 44)
        recs = [(built[i // 7], NONE) if i % 7 == 6 else (new[i], i) for i in range(n)]
        back = [(l, NONE if s != NONE else 9) for l, s in recs[::2]]
        out["records_%d" % n] = dict(labels=built, tomb=None, capacity=LM.capacity_for(len(built) + n), launches=[recs, back],
                                     keys=(built + new)[:3000] + fresh(50, lo=1 << 51),
                                     wants={0: ["claim"] + (["kill"] if n >= 7 else []), 1: (["kill"] if n else []) + (["revive"] if n >= 7 else [])} if n else {})
    # the extremes of the label range
    ext = [0, (1 << 32) - 1, (1 << 32) + 1, 1 << 63, M64 - 1]
    out["extremes"] = dict(labels=fresh(6), tomb=None, capacity=32, launches=[[(l, 10 + i) for i, l in enumerate(ext)], [(0, NONE), (1 << 63, 3)]],
                           keys=ext + [1, 1 << 32, (1 << 63) + 1, M64], wants={0: ["claim"], 1: ["kill", "move"]})
    # the empty key as a record: the failure word, nothing written
    out["empty_key"] = dict(labels=fresh(6), tomb=None, capacity=32, launches=[[(EMPTY, 5)], [(EMPTY, NONE)]], keys=[EMPTY, 1, 2],
                            wants={0: ["empty_key"], 1: ["empty_key"]})
    # a capacity-16 table filled to 16 used keys by successive launches (two of them dead by then), then one more: the failure
    # word is 1 and the launch ends; a lookup of an unknown label walks the whole table and answers unknown
    built = fresh(8, lo=1 << 45)
    more = fresh(9, lo=1 << 46)
    out["fill16"] = dict(labels=built, tomb=None, capacity=16,
                         launches=[[(l, 20 + i) for i, l in enumerate(more[:4])], [(built[0], NONE), (more[1], NONE)],
                                   [(l, 30 + i) for i, l in enumerate(more[4:8])], [(more[8], 99)], [(1 << 60, NONE)]],
                         keys=built + more + [1 << 61], wants={0: ["claim"], 1: ["kill"], 2: ["claim"], 3: ["full"], 4: ["full"]}, fills_to=16)
    # HNSW-shaped build: tombstoned nodes left out; the delta erases a live label and gives a tombstoned one its id back
    n = 120
    built = fresh(n, lo=1 << 47)
    tomb = [i % 4 == 2 for i in range(n)]
    out["hnsw_shape"] = dict(labels=built, tomb=tomb, capacity=LM.capacity_for(n), launches=[[(built[0], NONE), (built[2], 2)], [(built[6], 6), (built[2], NONE)]],
                             keys=built, wants={0: ["kill", "claim"], 1: ["claim", "kill"]})
    return out
