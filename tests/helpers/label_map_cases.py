"""What tests/test_label_map_kernels_gpu.py (the device label map's kernels, through tests/helpers/label_map_probe.hip) and
tests/test_label_map_model_cpu.py (which pins the restated hash, the models and the cases' reach without a GPU) share:

  * the hash and the sizing rule of csrc/label_map_hash.hpp, restated (mix, bucket, capacity);
  * a dict model of the build (label -> slot, tombstoned nodes left out, the failure count) and of the resolve (per list the
    known labels' slots and positions in list order, the segment offsets, K8b's tile offsets);
  * the build cases and the resolve cases, with the properties each is there for (so the CPU test can check that a case
    really reaches its path: a probe run longer than a wave, a run that wraps the table's end, ...).
"""
import numpy as np

M64 = (1 << 64) - 1
EMPTY = M64                 # the empty key
NONE = 0xFFFFFFFF
KEY_TILE = 256              # keys per block of the resolve launches (label_map.hip)
DIST_TILE = 64              # K8b's tile (prefilter_tiles)
TOMBSTONE = 0x00010000      # HnswGraph::kDeleteFlag, in word 0 of a node's level-0 list
MIN_CAPACITY = 16


def mix(x):
    """label_map_mix: the finaliser of splitmix64"""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def mix_np(x):
    x = x.astype(np.uint64)
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def bucket(label, capacity):
    return mix(label) & (capacity - 1)


def capacity_for(count):
    c = MIN_CAPACITY
    while c < 2 * count:
        c <<= 1
    return c


def colliding_labels(capacity, want_bucket, n, start=1):
    """n distinct labels (ascending, from `start`) that the hash sends to one bucket of a table of `capacity`"""
    out, at = [], start
    while len(out) < n:
        block = np.arange(at, at + (1 << 16), dtype=np.uint64)
        hit = block[(mix_np(block) & np.uint64(capacity - 1)) == np.uint64(want_bucket)]
        out.extend(int(v) for v in hit)
        at += 1 << 16
    return out[:n]


# ---- models ---------------------------------------------------------------------------------------------------------------
def build_model(labels, tomb=None):
    """(label -> slot of the nodes the build inserts, failure count): a tombstoned node stays out; the empty key as a label
    and every further slot of a label already met are failures (which slot of a repeated label wins is not defined)"""
    table, fails = {}, 0
    for i, l in enumerate(labels):
        if tomb is not None and tomb[i]:
            continue
        if l == EMPTY or l in table:
            fails += 1
            continue
        table[l] = i
    return table, fails


def resolve_model(table, keys, list_begin):
    """what the resolve launches write: seg_begin, tile_begin, slot, pos"""
    seg, tile, slot, pos = [0], [0], [], []
    for s in range(len(list_begin) - 1):
        for i in range(list_begin[s], list_begin[s + 1]):
            if keys[i] != EMPTY and keys[i] in table:
                slot.append(table[keys[i]])
                pos.append(i)
        seg.append(len(slot))
        tile.append(tile[-1] + (seg[-1] - seg[-2] + DIST_TILE - 1) // DIST_TILE)
    return seg, tile, slot, pos


def table_as_dict(keys, vals):
    """the downloaded table as {label: slot}; a label stored twice shows as a length mismatch to the caller"""
    used = np.nonzero(keys != np.uint64(EMPTY))[0]
    return {int(keys[h]): int(vals[h]) for h in used}, len(used)


def longest_probe(table_keys, capacity):
    """over the stored labels: (longest distance from a label's bucket to where it lies, whether some run wraps the end);
    also asserts the linear-probing invariant -- no empty bucket between a label's first bucket and its place"""
    longest, wraps = 0, False
    for h in np.nonzero(table_keys != np.uint64(EMPTY))[0]:
        b = bucket(int(table_keys[h]), capacity)
        d = (int(h) - b) % capacity
        for step in range(d):
            assert table_keys[(b + step) % capacity] != np.uint64(EMPTY), "an empty bucket inside a probe run"
        longest = max(longest, d)
        wraps |= b + d >= capacity
    return longest, wraps


# ---- build cases ------------------------------------------------------------------------------------------------------------
def build_cases():
    """name -> dict(labels, tomb or None, capacity, and what the case is there for)"""
    rng = np.random.default_rng(20240)
    cases = {}
    for n in (0, 1, 63, 64, 65, 5000):
        labels = [int(v) for v in rng.choice(1 << 40, size=n, replace=False)]
        cases["count_%d" % n] = dict(labels=labels, tomb=None, capacity=capacity_for(n))
    # the extremes, and labels that differ in one bit only (63, 32, 31): a hash or a compare that drops the high word shows
    base = 0x1234_5678_1234_5678 & ~((1 << 63) | (1 << 32) | (1 << 31))
    cases["extremes"] = dict(labels=[0, M64 - 1, base, base | (1 << 63), base | (1 << 32), base | (1 << 31), 1, 1 << 32, 1 << 63],
                             tomb=None, capacity=capacity_for(9))
    # 70 labels of one bucket among others: a probe run that crosses a wave's worth of entries (minimum capacity for the count)
    cap = capacity_for(200)
    col = colliding_labels(cap, 17, 70)
    others = [int(v) for v in rng.choice(np.arange(1 << 41, (1 << 41) + (1 << 20)), size=130, replace=False)]
    cases["collide_70"] = dict(labels=col[:35] + others + col[35:], tomb=None, capacity=cap, min_probe=64)
    # ... and a run that starts near the table's end and wraps to bucket 0
    cap = capacity_for(40)
    cases["wrap"] = dict(labels=colliding_labels(cap, cap - 3, 12) + colliding_labels(cap, cap - 1, 8, start=1 << 30), tomb=None,
                         capacity=cap, wraps=True)
    # tombstoned nodes: every third node, and one whose label a live node carries too (a slot re-used under the old label cannot
    # happen, but a tombstoned node must not count as "met twice")
    n = 300
    labels = [int(v) for v in rng.choice(1 << 40, size=n, replace=False)]
    tomb = [i % 3 == 1 for i in range(n)]
    labels[6] = labels[100]          # node 100 is tombstoned (100 % 3 == 1), node 6 is live
    assert tomb[100] and not tomb[6]
    cases["tombstones"] = dict(labels=labels, tomb=tomb, capacity=capacity_for(n))
    # a repeated label (and the empty key as a label): counted in the failure word, never a hang
    labels = [int(v) for v in rng.choice(1 << 40, size=500, replace=False)]
    labels[400] = labels[3]
    labels[401] = labels[3]
    labels[77] = EMPTY
    cases["repeated"] = dict(labels=labels, tomb=None, capacity=capacity_for(500), fails=3)
    # a table larger than the minimum
    labels = [int(v) for v in rng.choice(1 << 40, size=100, replace=False)]
    cases["roomy"] = dict(labels=labels, tomb=None, capacity=4 * capacity_for(100))
    return cases


# ---- resolve cases ----------------------------------------------------------------------------------------------------------
SEG_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 2049)


def resolve_world():
    """the table every resolve case runs against: 5000 labels, some tombstoned"""
    rng = np.random.default_rng(515)
    labels = [int(v) for v in rng.choice(1 << 40, size=5000, replace=False)]
    tomb = [i % 11 == 5 for i in range(5000)]
    unknown = [int(v) for v in (1 << 50) + rng.choice(1 << 30, size=4000, replace=False)]
    return labels, tomb, unknown


def resolve_cases():
    """name -> (keys, list_begin).  A shared list is one segment."""
    labels, tomb, unknown = resolve_world()
    live = [l for l, t in zip(labels, tomb) if not t]
    dead = [l for l, t in zip(labels, tomb) if t]
    rng = np.random.default_rng(616)
    cases = {}

    def seg(n, known=0.8):
        out = []
        for _ in range(n):
            u = rng.random()
            out.append(live[rng.integers(len(live))] if u < known else (unknown[rng.integers(len(unknown))] if u < 0.95 else dead[rng.integers(len(dead))]))
        return out

    def csr(segs):
        keys, lb = [], [0]
        for s in segs:
            keys.extend(s)
            lb.append(len(keys))
        return keys, lb

    # every tile edge, as per-query lists in one batch (with empty segments between full ones) and each as a shared list
    segs = []
    for n in SEG_LENGTHS:
        segs.append(seg(n))
        segs.append([])
    cases["edges_csr"] = csr(segs + [seg(64)])
    for n in SEG_LENGTHS:
        cases["shared_%d" % n] = csr([seg(n)])
    # unknown labels at the first, a middle and the last position; a segment of unknown labels only; a label twice; UINT64_MAX
    a = seg(300, known=1.0)
    a[0], a[150], a[299] = unknown[0], unknown[1], unknown[2]
    b = [unknown[i] for i in range(70)]
    c = seg(130, known=1.0)
    c[100] = c[5]
    c[129] = c[5]
    d = seg(65, known=1.0)
    d[64] = EMPTY
    cases["unknown_places"] = csr([a, b, c, d])
    cases["all_unknown_shared"] = csr([b + dead[:30]])
    # every key known: the kept counts sit ON K8b's 64-entry tile edges (63 / 64 / 65 / 128 / 129), which decides tile_begin
    cases["all_known_tiles"] = csr([seg(n, known=1.0) for n in (63, 64, 65, 128, 129)] + [[]] + [seg(64, known=1.0)])
    for n in (63, 64, 65, 128, 129):
        cases["all_known_shared_%d" % n] = csr([seg(n, known=1.0)])
    # 2 and 257 segments
    cases["two"] = csr([seg(257), seg(63)])
    cases["many"] = csr([seg(int(rng.integers(0, 40))) if i % 7 else [] for i in range(257)])
    return cases
