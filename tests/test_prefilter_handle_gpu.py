"""vk_index_search_filter_exact_batch through the C ABI: exact kNN among the rows a device filter handle admits
(csrc/filter_expand.hip, csrc/prefilter_handle.cc) on FLAT, HNSW and four logical shards on one device.

Nothing here has a tolerance.  Every answer is compared bit for bit with vk_index_search_labels over vk_filter_read_labels'
list and with the CPU oracle's heap over the known labels in ascending order; on FLAT also with
vk_index_search_batch_filter_handles (ids, distance bits, counts).  vk_filter_read_labels itself is compared with the bits
vk_filter_read returns.  The counters are exact, on plain and on sharded indexes: `candidates` is, per query and device stage,
the number of known entries at or below the stage's k-th smallest oracle distance, and fallback_queries counts exactly the
queries a stage does not cover (k above 4096, more ties than the hand-back holds, a NaN query, no room for the label map).
For a sharded index the test restates the router (which shard a label lives on) and runs the oracle per shard."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOLABEL = np.iinfo(np.uint64).max
SLACK = 64          # kPrefilterSlack
FIELDS = ("batches", "queries", "runs", "labels_expanded", "known_keys", "candidates", "fallback_queries", "downloaded_runs")


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
        self.sharded = kind.startswith("SHARDED")
        self.g = vsa.Index(algo, dim, metric, initial_cap=cap or n, dtype=dtype, **kw)
        self.live = {}
        self.route, self.counts, self.algo = {}, [0, 0, 0, 0], algo          # the sharded index's router, restated (see deal)
        self.add(self.rows(n), np.arange(n, dtype=np.uint64) * 3 + 10)

    def rows(self, n):
        x = self.rng.standard_normal((n, self.dim)).astype(np.float32)
        return np.stack([self.oracle.normalize(v)[0] for v in x]) if self.metric == "COSINE" else x

    def deal(self, labels):
        """ShardedIndex::add_batch's routing: a known label stays where it is; the labels new in this call are dealt out in
        contiguous runs, shard after shard, each up to an even share of the size the index will have"""
        fresh, seen = [], set()
        for l in labels.tolist():
            if l not in self.route and l not in seen:
                fresh.append(l)
                seen.add(l)
        after = sum(self.counts) + len(fresh)
        s, quota = 0, 0

        def next_quota(s):
            while s < 4:
                target = after * (s + 1) // 4 - after * s // 4
                if target > self.counts[s]:
                    return s, target - self.counts[s]
                s += 1
            return 3, 1 << 62
        s, quota = next_quota(0)
        for l in fresh:
            if quota == 0:
                s, quota = next_quota(s + 1)
            self.route[l] = s
            self.counts[s] += 1
            quota -= 1

    def add(self, x, labels):
        self.g.add_batch(x, labels)
        if self.sharded:
            self.deal(np.asarray(labels, np.uint64))
        st = bf16_round(x) if self.dtype == "bf16" else x
        for i, l in enumerate(labels):
            self.live[int(l)] = st[i]

    def remove(self, labs):
        for l in labs:
            assert self.g.remove(int(l)) == 0
            del self.live[int(l)]
            if self.sharded and self.algo == "FLAT":      # the row is gone; an HNSW tombstone keeps its slot and its shard
                self.counts[self.route.pop(int(l))] -= 1

    def known(self, keys):
        lab = [int(l) for l in keys.tolist() if int(l) in self.live]
        rows = np.stack([self.live[l] for l in lab]) if lab else np.zeros((0, self.dim), np.float32)
        return rows, np.array(lab, dtype=np.uint64)

    def predict_one(self, q, keys, k):
        """one device stage over `keys`: (candidates it hands back, 1 if it marks the query for the list path), from the
        oracle's distances"""
        rows, lab = self.known(keys)
        if k > 4096:
            return 0, 1
        if len(lab) == 0:
            return 0, 0
        d, _ = self.oracle.prefilter_topk(self.metric, q, rows, lab, len(lab))      # every distance, ascending
        if np.isnan(d).any() or np.isnan(q).any():
            return 0, 1
        T = d[min(k, len(d)) - 1]
        c = int(np.count_nonzero(d <= T))
        return (c, 0) if c <= k + SLACK else (0, 1)

    def predict(self, q, keys, k):
        """the whole index: a plain index is one stage; a sharded index runs one stage per shard over the labels routed there
        (each with its own k-th distance and its own ties) -- the candidates of the shards that answer add up, and a query any
        shard marks is marked"""
        if not self.sharded:
            return self.predict_one(q, keys, k)
        parts = [self.predict_one(q, np.array([l for l in keys.tolist() if self.route.get(int(l)) == s], np.uint64), k) for s in range(4)]
        return sum(p[0] for p in parts), int(any(p[1] for p in parts))

    def run(self, Q, k, filters):
        s0 = self.g.filter_exact_stats()
        out = self.g.search_filter_exact_batch(Q, k, filters)
        s1 = self.g.filter_exact_stats()
        return out, {f: getattr(s1, f) - getattr(s0, f) for f in FIELDS}

    def check(self, out, Q, k, filters, lists, single=True):
        D, L, N = out
        for q in range(Q.shape[0]):
            keys = lists[id(filters[q])]
            n = int(N[q])
            rows, lab = self.known(keys)
            od, ol = self.oracle.prefilter_topk(self.metric, Q[q], rows, lab, k)
            assert L[q, :n].tolist() == ol.tolist(), (q, len(keys))
            assert D[q, :n].view(np.uint32).tolist() == od.view(np.uint32).tolist(), (q, len(keys))
            assert np.all(np.isposinf(D[q, n:])) and np.all(L[q, n:] == NOLABEL)
            if single:
                sd, sl = self.g.search_labels(Q[q], k, keys)
                assert L[q, :n].tolist() == sl.tolist() and D[q, :n].view(np.uint32).tolist() == sd.view(np.uint32).tolist(), q

    def check_stats(self, moved, Q, k, filters, lists, runs):
        pred = [self.predict(Q[q], lists[id(filters[q])], k) for q in range(Q.shape[0])]
        assert moved["batches"] == 1 and moved["queries"] == Q.shape[0] and moved["runs"] == runs
        assert moved["fallback_queries"] == sum(p[1] for p in pred)
        assert moved["candidates"] == sum(p[0] for p in pred)
        # downloaded runs: the runs with a marked query; per run and shard the whole list is expanded, and the label maps
        # together know the list's live labels (a label lives on one shard)
        first = [q for q in range(Q.shape[0]) if q == 0 or filters[q] is not filters[q - 1]]
        assert moved["downloaded_runs"] == sum(1 for i, q in enumerate(first)
                                               if any(p[1] for p in pred[q:(first[i + 1] if i + 1 < len(first) else len(pred))]))
        if k <= 4096:
            assert moved["labels_expanded"] == sum(len(lists[id(filters[q])]) for q in first) * (4 if self.sharded else 1)
            assert moved["known_keys"] == sum(len(self.known(lists[id(filters[q])])[1]) for q in first)
        return pred


def count_runs(filters):
    return sum(1 for i, f in enumerate(filters) if i == 0 or f is not filters[i - 1])


def read_list(f):
    """vk_filter_read_labels, checked against vk_filter_read's bits"""
    nbits, allowed = f.info()
    bits = f.read()
    want = np.flatnonzero(np.unpackbits(bits.view(np.uint8), bitorder="little")[:nbits]).astype(np.uint64)
    got = f.read_labels()
    assert got.tolist() == want.tolist() and len(got) == allowed
    part, total = f.read_labels(cap=max(len(want) - 1, 0))
    assert total == len(want) and part.tolist() == want[:max(len(want) - 1, 0)].tolist()
    return got


def make_filters(w, rng, k, max_label):
    """filters of every origin and admitted size: {name: Filter}"""
    g = w.g
    live = np.array(sorted(w.live), np.uint64)
    unknown = np.array([0, 1, 2, 11, 12, 14], np.uint64)                 # labels the index never held (labels are 3 i + 10)
    top = int(max_label) + 1
    F = {}
    for name, m in (("empty", 0), ("one", 1), ("k_minus_1", k - 1), ("k", k), ("k_plus_1", k + 1), ("edge_2049", 2049)):
        ids = rng.choice(live, size=min(m, live.size), replace=False)
        F[name] = g.make_filter(top, labels=np.concatenate([ids, ids[:1]]))          # from ids, one twice
    F["with_unknown"] = g.make_filter(top + 1000, labels=np.concatenate([rng.choice(live, 300, replace=False), unknown,
                                                                         np.array([top + 5, top + 999], np.uint64)]))   # nbits above
    F["runs"] = g.make_filter(top, runs=[[0, 200], [1000, 1600], [top - 50, top + 50]])                                   # from runs
    F["nbits_below"] = g.make_filter(top // 2 + 7, runs=[[0, top]])                  # nbits below the largest label: every bit set
    F["delta"] = g.filter_apply_delta(F["runs"], top + 64, set=rng.choice(live, 500, replace=False), clear=np.arange(0, 150, dtype=np.uint64))
    return F


SHAPES = [  # kind, metric, dtype, dim, rows
    ("FLAT", "L2", "f32", 100, 3000),
    ("FLAT", "COSINE", "bf16", 257, 3000),
    ("FLAT", "IP", "f32", 1, 3000),
    ("HNSW", "COSINE", "f32", 100, 3000),
    ("HNSW", "L2", "bf16", 257, 3000),
    ("HNSW", "IP", "f32", 1, 3000),
    ("SHARDED_FLAT", "IP", "bf16", 100, 3000),
    ("SHARDED_HNSW", "COSINE", "f32", 257, 3000),
]


@pytest.mark.parametrize("kind,metric,dtype,dim,n", SHAPES)
def test_every_answer_is_the_list_paths_and_the_oracles(vsa, oracle, kind, metric, dtype, dim, n):
    rng = np.random.default_rng([len(kind), ord(metric[0]), dim, n])
    w = World(vsa, oracle, kind, metric, dtype, dim, n, rng)
    labels = np.array(sorted(w.live), np.uint64)
    w.remove(rng.choice(labels, size=n // 10, replace=False))        # FLAT: rows moved into the holes; HNSW: tombstones
    k = 10
    F = make_filters(w, rng, k, labels.max())
    lists = {id(f): read_list(f) for f in F.values()}
    assert len(lists[id(F["edge_2049"])]) == 2049 and len(lists[id(F["empty"])]) == 0
    names = list(F)
    # one run per filter (nq 1), the same with 17 queries, then tables of alternating handles and of runs of unequal length
    tables = [[F[nm]] for nm in names] + [[F[nm]] * 17 for nm in ("edge_2049", "delta", "empty")]
    tables.append([F[names[i % 3 + 1]] for i in range(17)])                                   # alternating: 17 runs
    tables.append([F["k"]] * 5 + [F["runs"]] * 1 + [F["with_unknown"]] * 9 + [F["k"]] * 2)    # unequal runs, a handle twice
    for tab in tables:
        Q = w.rows(len(tab))
        out, moved = w.run(Q, k, tab)
        w.check(out, Q, k, tab, lists, single=len(tab) <= 17)
        pred = w.check_stats(moved, Q, k, tab, lists, count_runs(tab))
        assert sum(p[1] for p in pred) == 0 and moved["fallback_queries"] == 0 and moved["downloaded_runs"] == 0   # tie-free, NaN-free
        if kind == "FLAT":      # the candidate-filter path of FLAT over the same handles: ids, distance bits, counts
            D2, L2, N2 = w.g.search_batch_filter_handles(Q, k, tab)
            assert N2.tolist() == out[2].tolist() and L2.tobytes() == out[1].tobytes()
            assert D2.view(np.uint32).tobytes() == out[0].view(np.uint32).tobytes()


@pytest.mark.parametrize("kind", ["FLAT", "HNSW", "SHARDED_FLAT"])
def test_batch_sizes_and_k(vsa, oracle, kind):
    rng = np.random.default_rng([len(kind), 7])
    w = World(vsa, oracle, kind, "L2", "f32", 100, 3000, rng)
    labels = np.array(sorted(w.live), np.uint64)
    big = w.g.make_filter(int(labels.max()) + 1, runs=[[0, int(labels.max())]])      # admits every row: k = 4096 has enough
    small = w.g.make_filter(int(labels.max()) + 1, labels=labels[:700])
    lists = {id(big): read_list(big), id(small): read_list(small)}
    for nq, k, f in ((257, 1, small), (1, 64, big), (17, 4096, big), (3, 5000, big), (257, 10, big)):
        Q = w.rows(nq)
        tab = [f] * nq
        out, moved = w.run(Q, k, tab)
        w.check(out, Q, k, tab, lists, single=nq <= 3)
        w.check_stats(moved, Q, k, tab, lists, 1)
        assert moved["fallback_queries"] == (nq if k > 4096 else 0) and moved["downloaded_runs"] == (1 if k > 4096 else 0)
    assert w.g.search_filter_exact_batch(w.rows(4), 0, small)[2].tolist() == [0, 0, 0, 0]
    assert w.g.search_filter_exact_batch(np.zeros((0, 100), np.float32), 5, [])[2].size == 0


@pytest.mark.parametrize("kind", ["FLAT", "HNSW", "SHARDED_HNSW"])
def test_ties_and_a_nan_query(vsa, oracle, kind):
    """duplicate rows under distinct labels straddling the k-th place (the smaller labels win); with more ties than the
    hand-back holds, and with a NaN query, the query takes the list path -- and only that query"""
    rng = np.random.default_rng([len(kind), 13])
    w = World(vsa, oracle, kind, "L2", "f32", 100, 1500, rng, cap=2000)
    k = 10
    dup = w.rows(1)
    few = np.arange(20000, 20000 + 14, dtype=np.uint64)                  # 14 copies straddle the 10th place and fit in the hand-back
    # more copies than k + 64 -- on EVERY shard of a sharded index (the copies are dealt out evenly: each shard's own ties overflow)
    many = np.arange(30000, 30000 + (k + SLACK + 5) * (4 if kind.startswith("SHARDED") else 1), dtype=np.uint64)
    w.add(np.repeat(dup, few.size, axis=0), few)
    w.add(np.repeat(dup * np.float32(2), many.size, axis=0), many)
    base = np.array(sorted(w.live), np.uint64)[::3][:400]                # (every third row: some on every shard of a sharded index)
    f_few = w.g.make_filter(40000, labels=np.concatenate([base, few]))
    f_many = w.g.make_filter(40000, labels=np.concatenate([base, many]))
    lists = {id(f_few): read_list(f_few), id(f_many): read_list(f_many)}
    Q = np.concatenate([w.rows(2), dup + np.float32(1e-3), dup * np.float32(2)])     # the last two sit on the duplicates
    # (the copies of 2 * dup are nearer to dup than any random row is, so with f_many both of the last two queries meet them)
    for f, fell in ((f_few, [0, 0, 0, 0]), (f_many, [0, 0, 1, 1])):
        tab = [f] * 4
        out, moved = w.run(Q, k, tab)
        w.check(out, Q, k, tab, lists)
        pred = w.check_stats(moved, Q, k, tab, lists, 1)
        assert [p[1] for p in pred] == fell and moved["downloaded_runs"] == (1 if any(fell) else 0)
    Qn = w.rows(3)
    Qn[1, 5] = np.nan
    out, moved = w.run(Qn, k, [f_few] * 3)
    assert moved["fallback_queries"] == 1 and moved["downloaded_runs"] == 1 and moved["runs"] == 1
    for q in (0, 2):
        w.check((out[0][q:q + 1], out[1][q:q + 1], out[2][q:q + 1]), Qn[q:q + 1], k, [f_few], lists)
    sd, sl = w.g.search_labels(Qn[1], k, lists[id(f_few)])               # the NaN query: whatever the list path says
    n = int(out[2][1])
    assert out[1][1, :n].tolist() == sl.tolist() and out[0][1, :n].view(np.uint32).tolist() == sd.view(np.uint32).tolist()


@pytest.mark.parametrize("kind,replace", [("FLAT", False), ("HNSW", False), ("HNSW", True), ("SHARDED_FLAT", False)])
def test_the_answer_follows_the_writes(vsa, oracle, kind, replace):
    """rows removed, re-added and updated between calls, tombstoned HNSW nodes, an HNSW slot reused under a new label, a
    resize: the handle stays the same, the answer is the oracle's after every write"""
    rng = np.random.default_rng([len(kind), int(replace), 99])
    n, dim, k, nq = 1500, 100, 10, 6
    kw = dict(allow_replace_deleted=True) if replace else {}
    w = World(vsa, oracle, kind, "COSINE", "f32", dim, n, rng, cap=n + 400, **kw)
    labels = np.array(sorted(w.live), np.uint64)
    new = np.arange(10 ** 5, 10 ** 5 + 300, dtype=np.uint64)
    f = w.g.make_filter(10 ** 5 + 400, labels=np.concatenate([rng.choice(labels, 600, replace=False), new]))
    lists = {id(f): read_list(f)}
    Q = w.rows(nq)

    def read():
        out, moved = w.run(Q, k, [f] * nq)
        w.check(out, Q, k, [f] * nq, lists)
        w.check_stats(moved, Q, k, [f] * nq, lists, 1)
        assert moved["fallback_queries"] == 0
        return out

    read()
    gone = lists[id(f)][:40]
    w.remove([l for l in gone.tolist() if l in w.live])          # removed rows / tombstones
    read()
    w.add(w.rows(50), new[:50])                                  # new labels (HNSW with replace: into the tombstoned slots)
    read()
    back = [l for l in gone.tolist()[:10]]
    w.add(w.rows(len(back)), np.array(back, np.uint64))          # re-added under their old labels, other rows
    read()
    upd = lists[id(f)][100:110]
    upd = np.array([l for l in upd.tolist() if l in w.live], np.uint64)
    w.remove(upd.tolist())
    w.add(w.rows(len(upd)), upd)                                 # updated: the same labels, other rows
    read()
    b0 = w.g.prefilter_stats().label_map_builds
    a = read()
    assert w.g.prefilter_stats().label_map_builds == b0          # two reads, one publication
    w.g.resize(n + 1000)                                         # releases the map: the next handle search builds it again
    assert w.g.prefilter_stats().label_map_bytes == 0
    b = read()
    shards = 4 if kind.startswith("SHARDED") else 1
    assert w.g.prefilter_stats().label_map_builds == b0 + shards
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["FLAT", "HNSW"])
def test_a_map_without_room_is_a_downloaded_run(vsa, oracle, kind):
    rng = np.random.default_rng(4242)
    w = World(vsa, oracle, kind, "L2", "f32", 100, 1000, rng)
    labels = np.array(sorted(w.live), np.uint64)
    w.g.set_option("prefilter-label-map-bytes", 2048 * 12)       # below the table's size (2048 buckets of 12 bytes + the failure word)
    f = w.g.make_filter(int(labels.max()) + 1, labels=labels[::3])
    lists = {id(f): read_list(f)}
    Q = w.rows(5)
    out, moved = w.run(Q, 10, [f] * 5)
    w.check(out, Q, 10, [f] * 5, lists)
    assert moved["fallback_queries"] == 5 and moved["downloaded_runs"] == 1 and moved["candidates"] == 0
    assert w.g.prefilter_stats().label_map_bytes == 0


def test_argument_errors_touch_nothing_and_the_struct_sizes_stand(vsa, oracle):
    rng = np.random.default_rng(5)
    w = World(vsa, oracle, "FLAT", "L2", "f32", 16, 200, rng)
    other = World(vsa, oracle, "FLAT", "L2", "f32", 16, 50, rng)
    f = w.g.make_filter(1000, runs=[[0, 999]])
    alien = other.g.make_filter(1000, runs=[[0, 999]])
    lib = vsa.lib()
    Q = w.rows(3)
    od = np.full((3, 4), 7.0, np.float32)
    ol = np.full((3, 4), 7, np.uint64)
    on = np.full(3, 7, np.uint64)
    s0 = w.g.filter_exact_stats()

    def call(tab, queries=Q):
        t = None if tab is None else (C.c_void_p * 3)(*[None if x is None else x._h for x in tab])
        return lib.vk_index_search_filter_exact_batch(w.g._h, None if queries is None else queries.ctypes.data, 3, 4, t, od.ctypes.data,
                                                      ol.ctypes.data, on.ctypes.data)

    for tab, queries in (([f, None, f], Q), ([f, f, alien], Q), (None, Q), ([f, f, f], None)):
        assert call(tab, queries) == vsa.VK_ERR_INVALID
        assert np.all(od == 7.0) and np.all(ol == 7) and np.all(on == 7)
    s1 = w.g.filter_exact_stats()
    assert all(getattr(s0, x) == getattr(s1, x) for x in FIELDS)
    assert call([f, f, f]) == 0 and on.tolist() == [4, 4, 4]
    assert C.sizeof(vsa.Stats) == 568 and C.sizeof(vsa.Params) == 144
    assert C.sizeof(vsa.PrefilterStats) == 56 and C.sizeof(vsa.PrefilterStatsV2) == 80 and C.sizeof(vsa.FilterExactStats) == 72
