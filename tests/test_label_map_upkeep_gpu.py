"""Option prefilter-label-map-upkeep through the C ABI: the device label map brought up to date from the labels a write phase
touched (label_map_apply_kernel) instead of rebuilt from every published label.

Every scenario feeds the same operations to two indexes, one with the option 0 and one with 1 (dim 24, L2).  After every
write phase vk_index_search_labels_batch (a shared list and a CSR of lists, prefilter-device-resolve 1) and
vk_index_search_filter_exact_batch must give the same bytes on both and what the CPU oracle gives; vk_index_label_map_read
must return exactly the labels vk_index_contains answers true for, with distinct slots below the count.  The counters say
which road was taken: with 1 the table is built once and every later phase is one delta batch with no mismatch; with 0 every
phase is one build -- the behaviour before the option, which must not change.  On the commit before this option the first
set_option of this file is VK_ERR_INVALID."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, K, NQ = 24, 5, 6
NBITS = 1 << 13
UNKNOWN = np.arange(5000, 5040, dtype=np.uint64)
NOLABEL = np.iinfo(np.uint64).max


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


class Pair:
    """two indexes fed the same operations -- [0]: upkeep 0, [1]: upkeep 1 -- and what the oracle needs: label -> row"""

    def __init__(self, vsa, oracle, algo, cap, rng, **kw):
        if algo == "HNSW":
            kw = dict(m=8, ef_construction=40, **kw)
        self.vsa, self.oracle, self.rng = vsa, oracle, rng
        self.ix = [vsa.Index(algo, DIM, "L2", initial_cap=cap, **kw) for _ in range(2)]
        for i, g in enumerate(self.ix):
            g.set_option("prefilter-device-resolve", 1)
            g.set_option("prefilter-label-map-upkeep", i)      # (on the parent commit: VK_ERR_INVALID, the option does not exist)
        self.live, self.gone = {}, set()
        self.Q = self.rows(NQ)

    def set_option(self, name, value):
        for g in self.ix:
            g.set_option(name, value)

    def rows(self, n):
        return self.rng.standard_normal((n, DIM)).astype(np.float32)

    def add_batch(self, labels):
        x = self.rows(len(labels))
        for g in self.ix:
            g.add_batch(x, np.array(labels, np.uint64))
        for l, r in zip(labels, x):
            self.live[int(l)] = r
            self.gone.discard(int(l))

    def add(self, label):
        """one vk_index_add: a new label, an update in place, a deleted label again"""
        x = self.rows(1)[0]
        for g in self.ix:
            assert g.add(int(label), x) == self.vsa.VK_OK
        self.live[int(label)] = x
        self.gone.discard(int(label))

    def remove(self, label):
        for g in self.ix:
            assert g.remove(int(label)) == self.vsa.VK_OK
        del self.live[int(label)]
        self.gone.add(int(label))

    def stats(self):
        return [g.label_map_stats() for g in self.ix]

    def oracle_topk(self, q, keys):
        lab = [int(l) for l in keys if int(l) in self.live]
        rows = np.stack([self.live[l] for l in lab]) if lab else np.zeros((0, DIM), np.float32)
        return self.oracle.prefilter_topk("L2", q, rows, np.array(lab, dtype=np.uint64), K)

    def check_answer(self, out, lists):
        D, L, N = out
        for q in range(NQ):
            n = int(N[q])
            od, ol = self.oracle_topk(self.Q[q], lists[q])
            assert L[q, :n].tolist() == ol.tolist(), q
            assert D[q, :n].view(np.uint32).tolist() == od.view(np.uint32).tolist(), q
            assert np.all(np.isposinf(D[q, n:])) and np.all(L[q, n:] == NOLABEL)

    def check(self, read=True):
        """what a read phase sees, on both indexes"""
        pool = np.array(sorted(self.live) + sorted(self.gone) + UNKNOWN.tolist(), np.uint64)
        shared = self.rng.permutation(pool)
        lists = [self.rng.choice(pool, size=int(m), replace=False) for m in self.rng.integers(0, min(pool.size, 300), size=NQ)]
        lb = np.zeros(NQ + 1, np.uint64)
        lb[1:] = np.cumsum([len(l) for l in lists])
        admitted = np.sort(self.rng.choice(pool, size=pool.size * 2 // 3, replace=False))
        outs = []
        for g in self.ix:
            a = g.search_labels_batch(self.Q, K, shared)
            b = g.search_labels_batch(self.Q, K, np.concatenate(lists).astype(np.uint64), lb)
            f = g.make_filter(NBITS, admitted)
            c = g.search_filter_exact_batch(self.Q, K, f)
            outs.append((a, b, c))
        for x, y in zip(outs[0], outs[1]):
            assert all(u.tobytes() == v.tobytes() for u, v in zip(x, y))
        self.check_answer(outs[1][0], [shared] * NQ)
        self.check_answer(outs[1][1], lists)
        self.check_answer(outs[1][2], [admitted] * NQ)
        if read:
            for g in self.ix:
                labels, slots = g.label_map_read()
                assert sorted(labels.tolist()) == sorted(self.live)
                assert all(g.contains(l) for l in self.live) and not any(g.contains(l) for l in self.gone)
                assert len(set(slots.tolist())) == slots.size and (slots.size == 0 or int(slots.max()) < g.stats().count)

    def phase(self, check_read=True):
        """the read phase behind a write phase, and how the counters moved: [(builds, delta_batches, rebuilds_forced)] * 2"""
        s0 = self.stats()
        self.check(check_read)
        s1 = self.stats()
        assert all(s.delta_mismatches == 0 for s in s1)
        assert s1[0].delta_batches == 0 and s1[0].rebuilds_forced == 0      # option 0 never takes the new road
        return [(b.builds - a.builds, b.delta_batches - a.delta_batches, b.rebuilds_forced - a.rebuilds_forced) for a, b in zip(s0, s1)]


def test_flat(vsa, oracle):
    rng = np.random.default_rng(15)
    p = Pair(vsa, oracle, "FLAT", 2000, rng)
    order = list(range(10, 610))                  # the label in every row slot, as FLAT keeps them
    p.add_batch(order)
    assert p.phase() == [(1, 0, 0), (1, 0, 0)]    # the first batch builds, whatever the option says
    nxt = 1000

    def remove(label):
        at = order.index(label)
        order[at] = order[-1]                     # the last row fills the hole
        order.pop()
        p.remove(label)

    for ph in range(8):
        remove(order[-1])                         # the last row: nothing moves
        remove(order[len(order) // 2])            # a middle row: the last one -- a label the map holds -- moves into the hole
        for l in rng.choice(order, size=3, replace=False):
            remove(int(l))
        for _ in range(5):                        # new labels
            p.add(nxt)
            order.append(nxt)
            nxt += 1
        for l in rng.choice(order, size=3, replace=False):
            p.add(int(l))                         # updates in place: the label keeps its slot
        assert p.phase() == [(1, 0, 0), (0, 1, 0)], ph
    s = p.stats()
    assert s[1].builds == 1 and s[0].builds == 9 and s[1].delta_batches == 8
    assert s[1].claimed == 40 and s[1].killed == 40 and s[1].moved > 0 and s[1].dead_entries == s[1].used_entries - len(order) == 40
    # a label removed and added again within one phase: it ends in another slot
    victim = order[7]
    remove(victim)
    p.add(victim)
    order.append(victim)
    assert p.phase() == [(1, 0, 0), (0, 1, 0)]
    # a bulk run of new labels (one strided copy to the device, not the staging log)
    bulk = list(range(3000, 3256))
    p.add_batch(bulk)
    order.extend(bulk)
    assert p.phase() == [(1, 0, 0), (0, 1, 0)]
    # a phase above prefilter-label-map-delta-max: rebuilt whole, counted as forced
    p.set_option("prefilter-label-map-delta-max", 8)
    for _ in range(12):
        p.add(nxt)
        order.append(nxt)
        nxt += 1
    assert p.phase() == [(1, 0, 0), (1, 0, 1)]
    s = p.stats()
    assert s[1].dead_entries == 0 and s[1].used_entries == len(order)      # a rebuild drops the dead entries
    # ... and one below it again
    p.add(nxt)
    order.append(nxt)
    assert p.phase() == [(1, 0, 0), (0, 1, 0)]
    # prefilter-device-resolve = 0 releases the map as before; the next batch builds
    p.set_option("prefilter-device-resolve", 0)
    assert all(g.prefilter_stats().label_map_bytes == 0 for g in p.ix)
    p.set_option("prefilter-device-resolve", 1)
    remove(order[3])
    assert p.phase() == [(1, 0, 0), (1, 0, 0)]


def test_hnsw(vsa, oracle):
    rng = np.random.default_rng(16)
    p = Pair(vsa, oracle, "HNSW", 700, rng, allow_replace_deleted=True, build_threads=1)
    first = list(range(10, 410))
    p.add_batch(first)
    assert p.phase() == [(1, 0, 0), (1, 0, 0)]
    # single adds of new labels, staged and linked at the flush (hnsw-stage-adds; a graph this small stages only when told to)
    p.set_option("hnsw-build-min-graph", 1)
    for l in range(1000, 1030):
        p.add(l)
    assert all(g.stats().staged_adds == 30 for g in p.ix)
    assert p.phase() == [(1, 0, 0), (0, 1, 0)]
    # markDelete
    dead = [int(l) for l in rng.choice(first, size=10, replace=False)]
    for l in dead:
        p.remove(l)
    assert p.phase() == [(1, 0, 0), (0, 1, 0)]
    assert p.stats()[1].killed == 10
    # deleted labels again: the tombstone is cleared, the id stays
    for l in dead[:4]:
        p.add(l)
    assert p.phase() == [(1, 0, 0), (0, 1, 0)]
    assert p.stats()[1].revived == 4
    # new labels take over the six tombstoned slots that are left (deleted in an earlier phase)
    for l in range(1100, 1106):
        p.add(l)
    assert all(g.stats().deleted == 0 for g in p.ix)
    assert p.phase() == [(1, 0, 0), (0, 1, 0)]
    # delete, then add, in ONE phase: the new labels reuse the ids -- the count and the tombstone bits are what they were
    before = [g.stats().count for g in p.ix]
    gone = [int(l) for l in rng.choice(sorted(p.live), size=3, replace=False)]
    for l in gone:
        p.remove(l)
    for l in range(1200, 1203):
        p.add(l)
    assert [g.stats().count for g in p.ix] == before and all(g.stats().deleted == 0 for g in p.ix)
    assert p.phase() == [(1, 0, 0), (0, 1, 0)]
    # a batch of new labels through the host builder
    p.add_batch(list(range(1300, 1320)))
    assert p.phase() == [(1, 0, 0), (0, 1, 0)]
    s = p.stats()
    assert s[1].builds == 1 and s[1].delta_batches == 6 and s[1].dead_entries == len(dead) - 4 + 3


def test_growth_crosses_the_half_load_rule(vsa, oracle):
    rng = np.random.default_rng(17)
    p = Pair(vsa, oracle, "FLAT", 200, rng)
    p.add_batch(list(range(1, 10)))                 # 9 rows: a 32-bucket table
    assert p.phase() == [(1, 0, 0), (1, 0, 0)]
    assert [s.capacity for s in p.stats()] == [32, 32]
    nxt, forced = 100, 0
    for ph in range(5):                             # three new labels per phase: 12, 15, then 18 > 32 / 2
        for _ in range(3):
            p.add(nxt)
            nxt += 1
        moved = p.phase()
        assert moved[0] == (1, 0, 0) and moved[1] in ((0, 1, 0), (1, 0, 1)), ph
        forced += moved[1][2]
        s = p.stats()[1]
        assert 2 * s.used_entries <= s.capacity      # the load never passes one half
    s = p.stats()[1]
    assert forced == 1 and s.builds == 2 and s.rebuilds_forced == 1 and s.capacity == 64 and s.delta_batches == 4


def test_sharded(vsa, oracle):
    rng = np.random.default_rng(18)
    p = Pair(vsa, oracle, "FLAT", 1000, rng, shard_devices=[0, 0])
    assert [g.get_option("prefilter-label-map-upkeep") for g in p.ix] == [0, 1]
    p.set_option("prefilter-label-map-delta-max", 4096)
    assert all(g.get_option("prefilter-label-map-delta-max") == 4096 for g in p.ix)
    p.add_batch(list(range(10, 210)))
    assert p.phase(check_read=False) == [(2, 0, 0), (2, 0, 0)]      # one map per shard
    nxt = 1000
    for ph in range(3):
        for _ in range(6):
            p.add(nxt)
            nxt += 1
        for l in rng.choice(sorted(p.live), size=6, replace=False):
            p.remove(int(l))
        off, on = p.phase(check_read=False)
        assert on[0] == 0 and 1 <= on[1] <= 2 and on[2] == 0            # the shards that the phase touched, each one delta batch
        assert off == (on[1], 0, 0)                                     # ... where option 0 builds
    s = p.stats()
    assert s[1].builds == 2 and 0 < s[1].claimed <= 18 and s[0].builds == 2 + s[1].delta_batches
    with pytest.raises(vsa.VkError) as e:
        p.ix[1].label_map_read()
    assert e.value.code == vsa.VK_ERR_INVALID
