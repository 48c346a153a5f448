"""Option prefilter-device-resolve through the C ABI: vk_index_search_labels_batch with the label -> slot step on the device
(csrc/label_map.hip, csrc/prefilter_resolve.cc) against the same call with the host's hash lookups.

Nothing here has a tolerance.  With the option 0 and then 1, on shared and per-query lists, outputs and out_n are byte for
byte the same, and equal to the single call (vk_index_search_labels) and to the CPU oracle's heap over the known keys in list
order; keys, candidates and fallback_queries move alike; device_resolved_keys stands still with the option off and counts
every key sent with it on (a shared list once per batch; on a sharded index the keys its router passed on to the shards --
the router keeps its own host lookup).  Then the option stays 1 while the index is written to between the calls: removed,
re-added and updated labels, new labels past the old count, a resize, on HNSW with allow_replace_deleted a tombstoned slot
re-used under a new label -- after each write the answer is the oracle's, label_map_builds goes up after a write that
published a label, a count or a tombstone and stands still between two reads; option 0 brings label_map_bytes to 0; and a map
that finds no room (a prefilter-label-map-bytes budget below the table's size) leaves the batch to the host's lookups."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPT = "prefilter-device-resolve"
UNKNOWN = np.arange(10 ** 9, 10 ** 9 + 60, dtype=np.uint64)
NOLABEL = np.iinfo(np.uint64).max


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


class World:
    """an index plus what the oracle needs to know about it: label -> the row as the index stores it"""

    def __init__(self, vsa, oracle, kind, metric, dtype, dim, n, rng, cap=None, **kw):
        self.oracle, self.metric, self.dim, self.dtype, self.kind, self.rng = oracle, metric, dim, dtype, kind, rng
        algo = "HNSW" if "HNSW" in kind else "FLAT"
        if algo == "HNSW":
            kw = dict(m=8, ef_construction=40, **kw)
        if kind.startswith("SHARDED"):
            kw["shard_devices"] = [0, 0, 0, 0]
        self.g = vsa.Index(algo, dim, metric, initial_cap=cap or n, dtype=dtype, **kw)
        self.live = {}
        self.add(self.rows(n), np.arange(n, dtype=np.uint64) * 3 + 10)

    def rows(self, n):
        x = self.rng.standard_normal((n, self.dim)).astype(np.float32)
        return np.stack([self.oracle.normalize(v)[0] for v in x]) if self.metric == "COSINE" else x

    def add(self, x, labels):
        self.g.add_batch(x, labels)
        st = bf16_round(x) if self.dtype == "bf16" else x
        for i, l in enumerate(labels):
            self.live[int(l)] = st[i]

    def remove(self, labs):
        for l in labs:
            assert self.g.remove(int(l)) == 0
            del self.live[int(l)]

    def oracle_topk(self, q, keys, k):
        lab = [int(l) for l in keys.tolist() if int(l) in self.live]
        rows = np.stack([self.live[l] for l in lab]) if lab else np.zeros((0, self.dim), np.float32)
        return self.oracle.prefilter_topk(self.metric, q, rows, np.array(lab, dtype=np.uint64), k)

    def batch(self, Q, k, labels, lb):
        """one batch: (the outputs' bytes, the counters' movement)"""
        s0 = self.g.prefilter_stats()
        D, L, N = self.g.search_labels_batch(Q, k, labels, lb)
        s1 = self.g.prefilter_stats()
        moved = {f: getattr(s1, f) - getattr(s0, f) for f in ("batches", "queries", "keys", "candidates", "fallback_queries",
                                                              "device_resolved_keys", "label_map_builds")}
        return (D, L, N), moved

    def check(self, out, Q, k, labels, lb, single=True):
        D, L, N = out
        for q in range(Q.shape[0]):
            keys = labels if lb is None else labels[int(lb[q]):int(lb[q + 1])]
            n = int(N[q])
            od, ol = self.oracle_topk(Q[q], keys, k)
            assert L[q, :n].tolist() == ol.tolist(), (q, len(keys))
            assert D[q, :n].view(np.uint32).tolist() == od.view(np.uint32).tolist(), (q, len(keys))
            assert np.all(np.isposinf(D[q, n:])) and np.all(L[q, n:] == NOLABEL)
            if single:
                sd, sl = self.g.search_labels(Q[q], k, keys)
                assert L[q, :n].tolist() == sl.tolist() and D[q, :n].view(np.uint32).tolist() == sd.view(np.uint32).tolist(), q


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def make_lists(rng, pool, lengths):
    lists = []
    for m in lengths:
        keys = rng.choice(pool, size=min(m, pool.size), replace=False).astype(np.uint64)
        if keys.size >= 2:
            keys = np.concatenate([keys, keys[:1]])      # a label twice
        lists.append(keys)
    return lists


def csr(lists):
    lb = np.zeros(len(lists) + 1, np.uint64)
    lb[1:] = np.cumsum([len(l) for l in lists])
    return np.concatenate(lists).astype(np.uint64), lb


SHAPES = [  # kind, metric, dtype, dim, rows
    ("FLAT", "L2", "f32", 100, 3000),
    ("FLAT", "COSINE", "bf16", 257, 2000),
    ("FLAT", "COSINE", "f32", 1, 2000),
    ("HNSW", "COSINE", "f32", 100, 1500),
    ("HNSW", "L2", "bf16", 257, 1200),
    ("HNSW", "L2", "f32", 1, 1200),
    ("SHARDED_FLAT", "L2", "bf16", 100, 3000),
    ("SHARDED_HNSW", "COSINE", "f32", 257, 1200),
]


@pytest.mark.parametrize("kind,metric,dtype,dim,n", SHAPES)
def test_option_off_and_on_give_the_same_bytes(vsa, oracle, kind, metric, dtype, dim, n):
    rng = np.random.default_rng([len(kind), ord(metric[0]), dim, n])
    w = World(vsa, oracle, kind, metric, dtype, dim, n, rng)
    labels = np.array(sorted(w.live), np.uint64)
    w.remove(rng.choice(labels, size=n // 10, replace=False))        # FLAT: rows moved into the holes; HNSW: tombstones
    pool = np.concatenate([labels, UNKNOWN])                          # (the removed labels are still in the pool)
    k, nq = 10, 21
    Q = w.rows(nq)
    lengths = [0, 1, 9, 10, 11, 63, 64, 65, 0, 255, 256, 257, 700, n, 0, 2049, 5, 5, 5, 5, 300][:nq]
    per_query = csr(make_lists(rng, pool, lengths))
    unknown_only = (UNKNOWN.copy(), None)
    shared = (make_lists(rng, pool, [600])[0], None)
    for labs, lb in (unknown_only, per_query, shared):      # (the last one leaves a map behind on every kind of index)
        sent = int(labs.size)
        w.g.set_option(OPT, 0)
        off, m_off = w.batch(Q, k, labs, lb)
        w.g.set_option(OPT, 1)        # (on the parent commit: VK_ERR_INVALID, the option does not exist)
        on, m_on = w.batch(Q, k, labs, lb)
        assert same_bytes(off, on)
        w.check(on, Q, k, labs, lb)
        for f in ("batches", "queries", "keys", "candidates", "fallback_queries"):
            assert m_off[f] == m_on[f], f
        assert m_off["device_resolved_keys"] == 0 and m_off["label_map_builds"] == 0
        per_batch = m_on["keys"] if lb is not None else m_on["keys"] // nq     # (a shared list: `keys` counts it once per query)
        assert m_on["device_resolved_keys"] == per_batch
        if not kind.startswith("SHARDED"):
            assert m_on["device_resolved_keys"] == sent and m_on["keys"] == (sent if lb is not None else sent * nq)
        else:                           # the router passes on the keys it has a route for: FLAT shards, the live labels; HNSW
            routed = set(w.live) if "FLAT" in kind else set(labels.tolist())      # shards, the tombstoned ones too (they keep their slot)
            assert m_on["device_resolved_keys"] == sum(int(l) in routed for l in labs.tolist())
    s = w.g.prefilter_stats()
    assert s.label_map_builds >= 1 and s.label_map_bytes > 0
    dev = w.g.stats().device_bytes
    w.g.set_option(OPT, 0)
    assert w.g.prefilter_stats().label_map_bytes == 0
    assert dev - w.g.stats().device_bytes == s.label_map_bytes         # the map is counted in vk_index_stats.device_bytes


@pytest.mark.parametrize("kind,replace", [("FLAT", False), ("HNSW", False), ("HNSW", True), ("SHARDED_FLAT", False)])
def test_the_map_follows_the_writes(vsa, oracle, kind, replace):
    rng = np.random.default_rng([len(kind), int(replace), 99])
    n, dim, k, nq = 1500, 100, 10, 6
    kw = dict(allow_replace_deleted=True) if replace else {}
    w = World(vsa, oracle, kind, "COSINE", "f32", dim, n, rng, cap=n + 400, **kw)
    w.g.set_option(OPT, 1)
    Q = w.rows(nq)
    first = np.array(sorted(w.live), np.uint64)
    new = np.arange(10 ** 7, 10 ** 7 + 300, dtype=np.uint64)
    pool = np.concatenate([first, new, UNKNOWN])

    def read(expect_build):
        """a per-query batch and a shared one over everything the test ever uses; the oracle; the builds' movement"""
        labs, lb = csr(make_lists(rng, pool, [400, 0, pool.size, 65, 900, 256]))
        out, moved = w.batch(Q, k, labs, lb)
        w.check(out, Q, k, labs, lb, single=False)
        assert moved["device_resolved_keys"] > 0
        out2, moved2 = w.batch(Q, k, pool, None)
        w.check(out2, Q, k, pool, None, single=False)
        assert moved2["label_map_builds"] == 0                                # between two reads
        if expect_build is not None:
            assert (moved["label_map_builds"] > 0) == expect_build, moved
        return moved

    read(True)
    read(False)
    gone = rng.choice(first, size=200, replace=False)
    w.remove(gone)                                         # FLAT: the last rows move into the holes, the count shrinks
    read(True)
    if replace:                                            # a tombstoned slot under a new label: same id, another label
        w.add(w.rows(50), new[:50])
        read(True)
    w.add(w.rows(100), gone[:100])                         # re-added (HNSW without replace: the tombstone is lifted)
    read(True)
    kept = first[:120][~np.isin(first[:120], gone)]
    w.add(w.rows(kept.size), kept)                         # updated in place: the answers follow; a build is not required
    read(None)
    w.add(w.rows(250), new[50:])                           # new labels past the old count
    read(True)
    read(False)
    w.g.resize(n + 1000)                                   # releases the map: the next batch builds it again
    assert w.g.prefilter_stats().label_map_bytes == 0
    read(True)
    w.remove(new[60:61])                                   # one tombstone / one moved row
    read(True)
    assert w.g.prefilter_stats().label_map_bytes > 0
    w.g.set_option(OPT, 0)
    assert w.g.prefilter_stats().label_map_bytes == 0


@pytest.mark.parametrize("kind", ["FLAT", "HNSW"])
def test_a_map_without_room_leaves_the_batch_to_the_host(vsa, oracle, kind):
    """prefilter-label-map-bytes below the table's size (1000 rows: 2048 buckets of 12 bytes): the map is not built.  Never an
    error: the host resolves."""
    rng = np.random.default_rng(4242)
    w = World(vsa, oracle, kind, "L2", "f32", 100, 1000, rng)
    labels = np.array(sorted(w.live), np.uint64)
    w.remove(labels[::7])
    Q = w.rows(5)
    labs, lb = csr(make_lists(rng, np.concatenate([labels, UNKNOWN]), [300, 0, 64, 1000, 17]))
    w.g.set_option(OPT, 1)
    w.g.set_option("prefilter-label-map-bytes", 2048 * 12)       # (the table also carries its failure word: 16 bytes more)
    out, moved = w.batch(Q, 10, labs, lb)
    w.check(out, Q, 10, labs, lb)
    assert moved["device_resolved_keys"] == 0 and moved["batches"] == 1 and moved["keys"] == labs.size
    assert w.g.prefilter_stats().label_map_bytes == 0
    w.g.set_option("prefilter-label-map-bytes", 1 << 30)   # room again -- but this publication is tagged "no map": the next one
    w.remove(labels[1:2])
    out, moved = w.batch(Q, 10, labs, lb)
    w.check(out, Q, 10, labs, lb)
    assert moved["device_resolved_keys"] == labs.size and moved["label_map_builds"] == 1


def test_an_old_caller_gets_the_old_struct_and_nothing_behind_it(vsa, oracle):
    """struct_size = sizeof(vk_prefilter_stats) = 56: the seven old fields are filled, the bytes behind them are not touched"""
    import ctypes as C
    rng = np.random.default_rng(77)
    w = World(vsa, oracle, "FLAT", "L2", "f32", 16, 300, rng)
    w.g.set_option(OPT, 1)
    labs = np.array(sorted(w.live), np.uint64)
    w.batch(w.rows(3), 5, labs, None)
    buf = (C.c_uint8 * 96)(*([0xA5] * 96))
    old = C.cast(buf, C.POINTER(vsa.PrefilterStats))
    old.contents.struct_size = C.sizeof(vsa.PrefilterStats)
    assert vsa.lib().vk_index_prefilter_stats(w.g._h, old) == vsa.VK_OK
    assert old.contents.struct_size == 56 and old.contents.batches == 1 and old.contents.queries == 3 and old.contents.keys == 3 * labs.size
    assert bytes(buf)[56:] == bytes([0xA5] * 40)
    new = w.g.prefilter_stats()
    assert new.struct_size == 80 and new.batches == 1 and new.device_resolved_keys == labs.size and new.label_map_builds == 1
