"""vk_index_search_labels_batch where the device stage changes path: lists longer than the 2048 keys the select kernel holds
in registers, batches cut into several device passes (by query count and by entry count), a list beyond the scratch in the
middle of a live CSR, NaN / +-inf / zero distances, and an HNSW index whose rows are all one vector.

The discipline is that of test_prefilter_batch_gpu.py: every query's ids and distance bits equal the single call
(search_labels) and the CPU oracle's heap over the known keys in list order, and prefilter_stats agrees EXACTLY with counts
derived from the oracle's distances: fallback_queries = the queries with more than k + 64 entries at or below T (the k-th
smallest distance of the list) or a NaN among their distances, candidates = the entries at or below T summed over the others.
Labels are resolved to rows with a dense label -> row array, so lists of millions of keys cost no Python loop."""
import re
import time
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CSRC = Path(__file__).resolve().parent.parent / "valkey-search_amd" / "csrc"
UNKNOWN = np.arange(10 ** 6, 10 ** 6 + 40, dtype=np.uint64)
NOLABEL = np.iinfo(np.uint64).max
SLACK = 64


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class World:
    """an index plus what the oracle needs to know about it: label -> row (dense array), the rows as the index stores them"""

    def __init__(self, vsa, oracle, algo, metric, dtype, dim, x, pairwise=False, **kw):
        self.oracle, self.metric, self.dim, self.pairwise = oracle, metric, dim, pairwise
        if metric == "COSINE":
            x = np.stack([oracle.normalize(v)[0] for v in x])
        n = x.shape[0]
        self.labels = np.arange(n, dtype=np.uint64) + 10
        if algo == "HNSW":
            kw = dict(m=8, ef_construction=40, **kw)
        self.g = vsa.Index(algo, dim, metric, initial_cap=n, dtype=dtype, **kw)
        self.g.add_batch(x, self.labels)
        self.table = np.ascontiguousarray(bf16_round(x) if dtype == "bf16" else x, np.float32)
        self.row_of = np.full(n + 10, -1, np.int64)
        self.row_of[10:] = np.arange(n)
        self._dist = {}

    def remove(self, labs):
        for l in labs:
            assert self.g.remove(int(l)) == 0
        self.row_of[labs.astype(np.int64)] = -1

    def live(self):
        return self.labels[self.row_of[10:] >= 0]

    def queries(self, rng, nq):
        Q = rng.standard_normal((nq, self.dim)).astype(np.float32)
        if self.metric == "COSINE":
            Q = np.stack([self.oracle.normalize(v)[0] for v in Q])
        return Q

    def rows(self, keys):
        """row of every key, -1 = not in the index (unknown or removed)"""
        k = keys.astype(np.int64)
        r = np.full(k.size, -1, np.int64)
        m = k < self.row_of.size
        r[m] = self.row_of[k[m]]
        return r

    def distances(self, q):
        """the oracle's distance from q to every row of the table, [n]"""
        key = q.tobytes()
        if key not in self._dist:
            n = self.table.shape[0]
            if self.pairwise:      # NaN / inf in play: the bare distance call, pair by pair (no heap order involved)
                d = np.array([self.oracle.distance(self.metric, q, r) for r in self.table], np.float32)
            else:                  # k = n: every distance, with its label
                od, ol = self.oracle.prefilter_topk(self.metric, q, self.table, self.labels, n)
                assert od.size == n
                d = np.empty(n, np.float32)
                d[(ol - np.uint64(10)).astype(np.int64)] = od
            self._dist[key] = d
        return self._dist[key]

    def oracle_topk(self, q, keys, k):
        r = self.rows(keys)
        m = r >= 0
        return self.oracle.prefilter_topk(self.metric, q, self.table[r[m]], keys[m], k)

    def at_or_below_T(self, q, keys, k):
        """from the oracle's distances: (known entries, entries at or below the k-th smallest -- the largest when there are
        fewer than k; None when a distance is NaN)"""
        r = self.rows(keys)
        r = r[r >= 0]
        if r.size == 0:
            return 0, 0
        d = self.distances(q)[r]
        if np.isnan(d).any():
            return int(r.size), None
        kk = min(k, d.size)
        T = np.partition(d, kk - 1)[kk - 1]
        return int(r.size), int((d <= T).sum())

    def expect(self, Q, lists, k):
        """(fallback_queries, candidates) this batch must add to the counters"""
        fell = cands = 0
        for q, keys in enumerate(lists):
            _, c = self.at_or_below_T(Q[q], keys, k)
            if c is None or c > k + SLACK:
                fell += 1
            else:
                cands += c
        return fell, cands

    def stats(self):
        s = self.g.prefilter_stats()
        return np.array([s.batches, s.queries, s.fallback_queries, s.candidates], np.int64)

    def check(self, Q, k, labels, list_begin=None, single=None, oracle_too=True):
        """the batch against the oracle (every query) and the single call (every query, or those in `single`); returns the lists"""
        D, L, N = self.g.search_labels_batch(Q, k, labels, list_begin)
        nq = Q.shape[0]
        assert D.shape == (nq, k) and L.shape == (nq, k)
        lists = []
        for q in range(nq):
            keys = labels if list_begin is None else labels[int(list_begin[q]):int(list_begin[q + 1])]
            lists.append(keys)
            n = int(N[q])
            what = (q, keys.size, k)
            assert np.all(np.isposinf(D[q, n:])) and np.all(L[q, n:] == NOLABEL), what      # the padding past out_n
            if oracle_too:
                od, ol = self.oracle_topk(Q[q], keys, k)
                assert n == ol.size and np.array_equal(L[q, :n], ol), what
                assert np.array_equal(bits(D[q, :n]), bits(od)), what
            if single is None or q in single:
                sd, sl = self.g.search_labels(Q[q], k, keys)
                assert n == sl.size and np.array_equal(L[q, :n], sl), what
                assert np.array_equal(bits(D[q, :n]), bits(sd)), what
        return lists


def csr(lists):
    lb = np.zeros(len(lists) + 1, np.uint64)
    lb[1:] = np.cumsum([len(l) for l in lists])
    return np.concatenate(lists).astype(np.uint64), lb


def make_list(rng, pool, m):
    """m keys of the pool in random order; a pool smaller than m is used whole, the rest are repeats"""
    if m <= pool.size:
        return rng.choice(pool, size=m, replace=False).astype(np.uint64)
    return rng.permutation(np.concatenate([pool, rng.choice(pool, size=m - pool.size)])).astype(np.uint64)


# ---- long lists ----------------------------------------------------------------------------------------------------------
LONG = 10000
FAR_POOL = 1000


def far_list(w, rng, q, k, m=LONG):
    """every live label once, unknown labels, and repeats dealt evenly over the FAR_POOL farthest live labels: strictly
    farther than the k-th smallest distance wherever the index has that many labels beyond it, and in every case few
    enough copies of any one label that the entries at or below T stay within the hand-back"""
    live = w.live()
    d = w.distances(q)[w.rows(live)]
    order = np.argsort(d, kind="stable")
    far = live[order[-FAR_POOL:]]
    if live.size >= k + FAR_POOL:
        assert d[order[-FAR_POOL]] > d[order[k - 1]]                     # the repeats: strictly farther than the k-th smallest
    base = np.concatenate([live, UNKNOWN])
    reps = np.resize(far, m - base.size)
    assert -(-reps.size // FAR_POOL) + 1 <= SLACK                        # copies of one label: T's ties fit the slack
    return rng.permutation(np.concatenate([base, reps])).astype(np.uint64)


def near_list(w, rng, q, k, m=LONG):
    """every live label once, unknown labels, and the nearest label again and again: more than k + 64 entries at T"""
    live = w.live()
    d = w.distances(q)[w.rows(live)]
    base = np.concatenate([live, UNKNOWN])
    assert m - base.size > k + SLACK
    reps = np.full(m - base.size, live[np.argmin(d)], np.uint64)
    return rng.permutation(np.concatenate([base, reps])).astype(np.uint64)


def long_lists(w, rng, k, q_far, q_near):
    """nine lists: around the 2048 keys the select kernel holds in registers, every live label, and two 10 000-entry lists of
    repeats (position 2: built for q_far, the device answers; position 6: built for q_near, handed over); an all-unknown
    list sits in the middle"""
    pool = np.concatenate([w.labels, UNKNOWN])                           # (the removed labels are still in the pool)
    return [make_list(rng, pool, 2047), make_list(rng, pool, 2048), far_list(w, rng, q_far, k), make_list(rng, pool, 2049),
            UNKNOWN.copy(), make_list(rng, pool, 2305), near_list(w, rng, q_near, k), make_list(rng, pool, 4097), rng.permutation(w.live())]


_worlds = {}


def long_world(vsa, oracle, algo, metric, dtype, **kw):
    """one index per (algo, metric, dtype) for the whole module: 6000 / 3000 rows, a tenth of them removed"""
    key = (algo, metric, dtype, tuple(sorted(kw)))
    if key not in _worlds:
        rng = np.random.default_rng([ord(algo[0]), ord(metric[0]), len(dtype), len(kw)])
        n = 6000 if algo == "FLAT" else 3000
        w = World(vsa, oracle, algo, metric, dtype, 16, rng.standard_normal((n, 16)).astype(np.float32), **kw)
        w.remove(rng.choice(w.labels, size=n // 10, replace=False))
        _worlds[key] = w
    return _worlds[key]


def expect_sharded(w, Q, lists, k, own_near):
    """fallback_queries of a sharded index, where the oracle's distances decide it.  A shard's entries at or below ITS T are
    at most k - 1 plus the entries that share one distance, so a list without more than 64 - k + 1 such entries anywhere is
    answered by every shard; the near list is handed over by the shard that holds the nearest label of the query it was
    built for (`own_near`: that (query, list) pair).  Anything else is not decided here and must not occur."""
    fell = 0
    for q, keys in enumerate(lists):
        r = w.rows(keys)
        r = r[r >= 0]
        ties = int(np.unique(w.distances(Q[q])[r], return_counts=True)[1].max()) if r.size else 0
        if k - 1 + ties <= k + SLACK:
            continue
        assert own_near == (q, id(keys)), (q, keys.size, ties)
        fell += 1
    return fell


def run_long(w, rng, k, shared, sharded=False):
    cap = k + SLACK
    Q = w.queries(rng, 3 if shared else 9)
    nq = Q.shape[0]
    if not shared:
        lists = long_lists(w, rng, k, Q[2], Q[6])
        # before the GPU call, from the oracle's distances: the far list is answered, the near one handed over, and the
        # batch has queries on both sides
        assert w.at_or_below_T(Q[2], lists[2], k)[1] <= cap < w.at_or_below_T(Q[6], lists[6], k)[1]
        fell, cands = w.expect(Q, lists, k)
        assert 0 < fell < nq
        if sharded:
            assert expect_sharded(w, Q, lists, k, (6, id(lists[6]))) == fell
        labels, lb = csr(lists)
        s0 = w.stats()
        w.check(Q, k, labels, lb)
        d = w.stats() - s0
        assert d[2] == fell, (d, fell)
        if not sharded:                                                  # (candidates are counted per shard)
            assert d.tolist() == [1, nq, fell, cands], (d, fell, cands)
        return
    lists = long_lists(w, rng, k, Q[0], Q[1])
    assert w.at_or_below_T(Q[0], lists[2], k)[1] <= cap < w.at_or_below_T(Q[1], lists[6], k)[1]
    for i, keys in enumerate(lists):
        Qs = Q[1:2] if sharded and i == 6 else Q                         # (sharded: the near list with its own query only)
        fell, cands = w.expect(Qs, [keys] * Qs.shape[0], k)
        if sharded:
            assert expect_sharded(w, Qs, [keys] * Qs.shape[0], k, (0, id(keys)) if i == 6 else None) == fell
        s0 = w.stats()
        w.check(Qs, k, keys)
        d = w.stats() - s0
        assert d[2] == fell, (keys.size, d, fell)
        if not sharded:
            assert d.tolist() == [1, Qs.shape[0], fell, cands], (keys.size, d, fell, cands)


@pytest.mark.parametrize("shared", [False, True], ids=["lists", "shared"])
@pytest.mark.parametrize("k", [10, 64, 4096])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["L2", "COSINE"])
@pytest.mark.parametrize("algo", ["FLAT", "HNSW"])
def test_long_lists(vsa, oracle, algo, metric, dtype, k, shared):
    w = long_world(vsa, oracle, algo, metric, dtype)
    run_long(w, np.random.default_rng([k, shared, ord(algo[0]), ord(metric[0]), len(dtype)]), k, shared)


@pytest.mark.parametrize("shared", [False, True], ids=["lists", "shared"])
def test_long_lists_sharded(vsa, oracle, shared):
    """four logical shards on one device.  Candidates are counted per shard (each shard's T is its own), so answers and
    fallback_queries only, as far as the oracle's distances decide what a shard does (expect_sharded)."""
    w = long_world(vsa, oracle, "FLAT", "L2", "f32", shard_devices=[0, 0, 0, 0])
    assert w.g.shard_count() == 4
    run_long(w, np.random.default_rng([41, shared]), 10, shared, sharded=True)


# ---- the chunk loop ------------------------------------------------------------------------------------------------------
def chunk_constants():
    """the driver's scratch bounds, read from the sources"""
    host = (CSRC / "prefilter_host.hpp").read_text()
    batch = (CSRC / "prefilter_batch.cc").read_text()
    a, b = re.search(r"kPrefilterChunkBytes\s*=\s*(\d+)ull\s*<<\s*(\d+)\s*;", host).groups()
    c, d = re.search(r"kPrefilterChunkEntries\s*=\s*(\d+)ull\s*<<\s*(\d+)\s*;", host).groups()
    slack = int(re.search(r"kPrefilterSlack\s*=\s*(\d+)\s*;", host).group(1))
    e, f = re.search(r"kPrefilterChunkBytes\s*/\s*per_q_bytes\s*,\s*(\d+)u\s*<<\s*(\d+)\s*\)", batch).groups()
    assert "std::max<uint64_t>(q_bytes, cap * 8)" in batch
    return int(a) << int(b), int(c) << int(d), slack, int(e) << int(f)


def max_queries_per_pass(dim, k):
    chunk_bytes, chunk_entries, slack, q_limit = chunk_constants()
    stride = (dim + 63) // 64 * 64                                       # rows and staged queries: zero padded to 64 elements
    return min(chunk_bytes // max(stride * 4, (k + slack) * 8), q_limit), chunk_entries


def test_the_constants_are_todays():
    assert chunk_constants() == (64 << 20, 1 << 24, SLACK, 65536)
    assert max_queries_per_pass(16, 4096) == (2016, 1 << 24)


@pytest.mark.parametrize("shared", [False, True], ids=["lists", "shared"])
def test_a_batch_cut_by_query_count(vsa, oracle, shared):
    """k = 4096: the hand-back of one query is 33 280 bytes, so a device pass takes 2016 queries and a batch of 2053 takes two.
    Everything the second pass indexes by its first query -- the staged queries, the candidates' owner, the answers' offsets --
    is wrong for all 37 queries of it if the offset is lost."""
    k, dim, n = 4096, 16, 600
    max_q, chunk_entries = max_queries_per_pass(dim, k)
    nq = max_q + 37
    rng = np.random.default_rng(2016 + shared)
    w = World(vsa, oracle, "FLAT", "L2", "f32", dim, rng.standard_normal((n, dim)).astype(np.float32))
    pool = np.concatenate([w.labels, UNKNOWN])
    Q = w.queries(rng, nq)
    near_cut = set(range(max_q - 8, max_q + 8)) | set(range(0, nq, 50))
    assert nq > max_q
    if shared:
        keys = make_list(rng, pool, 600)
        known = int((w.rows(keys) >= 0).sum())
        assert chunk_entries // known > max_q                            # the query bound cuts, not the entry bound
        w.check(Q, k, keys, single=near_cut)
        want = nq * known
    else:
        lengths = [0, 1, 5, 40, 600]
        lists = [make_list(rng, pool, lengths[q % 5]) for q in range(nq)]
        lists[max_q - 1] = np.zeros(0, np.uint64)                        # an empty list ends the first pass,
        lists[max_q] = make_list(rng, w.labels, 40)                      # a known key starts the second
        assert sum(l.size for l in lists) < chunk_entries
        labels, lb = csr(lists)
        w.check(Q, k, labels, lb, single=near_cut)
        want = sum(int((w.rows(l) >= 0).sum()) for l in lists)
    # every list is shorter than k: T is its maximum, every known entry is a candidate, nothing falls back
    assert w.stats().tolist() == [1, nq, 0, want]


def test_a_batch_cut_by_entry_count(vsa, oracle):
    """The distances of one device pass hold 2^24 entries.  Lists of 2^23 + 1, 2^23 + 1 and 100 keys: the second list does
    not fit behind the first, so the batch takes two passes.  Then a list of 2^24 + 1 keys in a CSR (beyond the scratch: that
    query alone goes to the per-query path, an empty segment inside a live CSR) and as a shared list (every query does).
    Each long list is a permutation of every label followed by repeats of labels strictly farther than that query's T, so
    the device stage answers with exactly k candidates per query."""
    t0 = time.perf_counter()
    k, dim, n = 10, 4, 5000
    _, chunk_entries = max_queries_per_pass(dim, k)
    rng = np.random.default_rng(24)
    w = World(vsa, oracle, "FLAT", "L2", "f32", dim, rng.standard_normal((n, dim)).astype(np.float32))
    Q = w.queries(rng, 3)

    def long_list(q, m):
        d = w.distances(q)
        T = np.sort(d)[k - 1]
        far = w.labels[d > T]
        assert far.size == n - k                                         # no ties at T
        return np.concatenate([rng.permutation(w.labels), rng.choice(far, size=m - n)]).astype(np.uint64)

    half = chunk_entries // 2 + 1
    lists = [long_list(Q[0], half), long_list(Q[1], half), make_list(rng, w.labels, 100)]
    assert lists[0].size + lists[1].size > chunk_entries >= lists[1].size + lists[2].size
    assert w.expect(Q, lists, k) == (0, 30)
    labels, lb = csr(lists)
    w.check(Q, k, labels, lb)
    assert w.stats().tolist() == [1, 3, 0, 30]
    del labels
    # one list beyond the scratch in a CSR: the first query is handed over, the second answered by the device
    lists = [long_list(Q[0], chunk_entries + 1), lists[2]]
    assert lists[0].size > chunk_entries
    assert w.at_or_below_T(Q[1], lists[1], k)[1] == k
    labels, lb = csr(lists)
    w.check(Q[:2], k, labels, lb, single=())
    assert w.stats().tolist() == [2, 5, 1, 40]
    del labels
    # ... and as the shared list: both queries are handed over, no candidate is counted
    w.check(Q[:2], k, lists[0], single=())
    assert w.stats().tolist() == [3, 7, 3, 40]
    print(f"entry-count cut: {time.perf_counter() - t0:.1f} s")


# ---- NaN and the special values ------------------------------------------------------------------------------------------
def run_specials(w, rng, Q, k, lists, oracle_too):
    """a CSR batch and the shared batches of its lists, against the single call; the counters against the oracle's distances"""
    nq = Q.shape[0]
    fell, cands = w.expect(Q, lists, k)
    labels, lb = csr(lists)
    s0 = w.stats()
    w.check(Q, k, labels, lb, oracle_too=oracle_too)
    assert (w.stats() - s0).tolist() == [1, nq, fell, cands]
    for keys in lists:
        f2, c2 = w.expect(Q, [keys] * nq, k)
        s0 = w.stats()
        w.check(Q, k, keys, oracle_too=oracle_too)
        assert (w.stats() - s0).tolist() == [1, nq, f2, c2], keys.size
    return fell


@pytest.mark.parametrize("metric", ["L2", "IP"])
@pytest.mark.parametrize("algo", ["FLAT", "HNSW"])
def test_a_nan_query_falls_back_alone(vsa, oracle, algo, metric):
    """one NaN component in three of eight queries: every distance of such a query is NaN, which has no place in the select
    kernel's order.  Exactly the NaN queries whose list holds a known key are handed over -- one with an empty list and one
    with unknown labels only have no distance at all.  Answers against the single call only: bit equality with it is the
    contract, and the oracle's NaN order is pinned nowhere."""
    rng = np.random.default_rng([78, ord(algo[0]), ord(metric[0])])
    n, dim, nq, k = (1200 if algo == "FLAT" else 400), 16, 8, 10
    w = World(vsa, oracle, algo, metric, "f32", dim, rng.standard_normal((n, dim)).astype(np.float32), pairwise=True)
    pool = np.concatenate([w.labels, UNKNOWN])
    Q = w.queries(rng, nq)
    for q in (2, 5, 6):
        Q[q, rng.integers(0, dim)] = np.nan
    lists = [make_list(rng, pool, m) for m in (40, 300, 300, 5, n, 0, 0, 40)]
    lists[5] = UNKNOWN[:7].copy()
    assert all(np.isnan(w.distances(Q[q])).all() for q in (2, 5, 6))
    assert all(not np.isnan(w.distances(Q[q])).any() for q in (0, 1, 3, 4, 7))
    labels, lb = csr(lists)
    s0 = w.stats()
    w.check(Q, k, labels, lb, oracle_too=False)
    fell, cands = w.expect(Q, lists, k)
    assert fell == 1                                                     # query 2 alone
    assert (w.stats() - s0).tolist() == [1, nq, fell, cands]
    # a shared list: all three NaN queries have distances now
    s0 = w.stats()
    w.check(Q, k, lists[1], oracle_too=False)
    f2, c2 = w.expect(Q, [lists[1]] * nq, k)
    assert f2 == 3
    assert (w.stats() - s0).tolist() == [1, nq, f2, c2]


def test_an_infinite_row_makes_one_query_nan(vsa, oracle):
    """IP, a row with +inf at a component where one query holds 0: 0 * inf is NaN for that query alone; the other queries
    see -inf or +inf there, which have their place in the order"""
    rng = np.random.default_rng(91)
    n, dim, nq, k = 1200, 16, 6, 10
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[77, 3] = np.inf
    w = World(vsa, oracle, "FLAT", "IP", "f32", dim, x, pairwise=True)
    Q = w.queries(rng, nq)
    Q[4, 3] = 0.0
    bad = w.labels[77:78]
    lists = [np.concatenate([make_list(rng, w.labels[100:], m), bad]) for m in (40, 300, 1000)]
    lists = [lists[0], make_list(rng, w.labels[100:], 300), lists[1], UNKNOWN.copy(), lists[2], lists[2][::-1].copy()]
    d = np.stack([w.distances(q) for q in Q])
    assert np.isnan(d[4, 77]) and np.isnan(d).sum() == 1 and np.isinf(d[[0, 1, 2, 3, 5], 77]).all()
    fell = run_specials(w, rng, Q, k, lists, oracle_too=False)
    assert fell == 1                                                     # query 4: its list holds the row


def test_ties_at_infinity(vsa, oracle):
    """L2, 200 rows scaled by 1e20: their distances are +inf.  A list with fewer than k finite distances has T = +inf, and
    with more than k + 64 infinite ones it is handed over; with 5 of them the device answers, +inf in the answer."""
    rng = np.random.default_rng(92)
    n, dim, nq, k = 1200, 16, 4, 10
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[:200] *= np.float32(1e20)
    w = World(vsa, oracle, "FLAT", "L2", "f32", dim, x, pairwise=True)
    Q = w.queries(rng, nq)
    d = np.stack([w.distances(q) for q in Q])
    assert np.isposinf(d[:, :200]).all() and np.isfinite(d[:, 200:]).all()
    huge, plain = w.labels[:200], w.labels[200:]
    lists = [rng.permutation(np.concatenate([make_list(rng, plain, 5), make_list(rng, huge, 100)])),     # T = +inf, 100 ties: handed over
             rng.permutation(np.concatenate([make_list(rng, plain, 5), make_list(rng, huge, 5)])),       # all ten are the answer
             rng.permutation(np.concatenate([make_list(rng, plain, 300), make_list(rng, huge, 200)])),   # T finite: the infinite ones are out
             rng.permutation(np.concatenate([make_list(rng, plain, 9), make_list(rng, huge, 65), UNKNOWN]))]   # 74 at or below T: just fits
    assert [w.at_or_below_T(Q[q], lists[q], k)[1] for q in range(nq)] == [105, 10, 10, 74]
    fell = run_specials(w, rng, Q, k, lists, oracle_too=False)
    assert fell == 1
    D, L, N = w.g.search_labels_batch(Q[1:2], k, lists[1])
    assert int(N[0]) == 10 and np.isposinf(D[0]).sum() == 5


@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_rows_of_zeros(vsa, oracle, metric):
    """200 rows that are exactly zero, signs mixed (+0 and -0 components), and a zero query among the queries: every zero row
    has one and the same distance to a query (its products are +0 or -0, their sum a zero of either sign, and a zero of
    either sign leaves |q|^2 or 1 - 0 untouched), the smallest one under L2 for the zero query, where T lands on 0."""
    rng = np.random.default_rng(93)
    n, dim, nq, k = 1200, 16, 5, 10
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[:200] = rng.choice(np.array([0.0, -0.0], np.float32), (200, dim))
    w = World(vsa, oracle, "FLAT", metric, "f32", dim, x, pairwise=True)
    Q = w.queries(rng, nq)
    Q[3] = rng.choice(np.array([0.0, -0.0], np.float32), dim)
    Q[1] = np.abs(Q[1]) * np.float32(1e-3)                               # small and positive: under L2 the zero rows are its nearest
    d = np.stack([w.distances(q) for q in Q])
    assert all(np.unique(d[q, :200]).size == 1 for q in range(nq)) and not np.isnan(d).any()
    if metric == "L2":
        assert (d[3, :200] == 0).all() and (d[3, 200:] > 0).all()
    zeros, plain = w.labels[:200], w.labels[200:]
    lists = [rng.permutation(np.concatenate([make_list(rng, plain, 300), make_list(rng, zeros, 200)])),
             rng.permutation(np.concatenate([make_list(rng, plain, 300), make_list(rng, zeros, 200), UNKNOWN])),
             rng.permutation(np.concatenate([make_list(rng, plain, 40), make_list(rng, zeros, 60)])),
             rng.permutation(np.concatenate([make_list(rng, plain, 300), make_list(rng, zeros, 150)])),
             rng.permutation(np.concatenate([make_list(rng, plain, 3), make_list(rng, zeros, 70)]))]
    fell = run_specials(w, rng, Q, k, lists, oracle_too=True)
    if metric == "L2":
        assert fell >= 2                                                 # the zero query and the small one: T is the zero rows' distance


# ---- HNSW, every row the same vector -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10])
def test_hnsw_all_rows_identical(vsa, oracle, k):
    """400 copies of one vector in a graph: every distance of a query ties.  A list longer than k + 64 is handed over, the
    60-key list is not (60 <= k + 64 entries at or below T)."""
    rng = np.random.default_rng(94 + k)
    n, dim, nq = 400, 100, 6
    x = np.tile(rng.standard_normal((1, dim)).astype(np.float32), (n, 1))
    w = World(vsa, oracle, "HNSW", "L2", "f32", dim, x)
    Q = w.queries(rng, nq)
    lengths = [60, 300, 400, 300, 60, 400]
    lists = [make_list(rng, w.labels, m) for m in lengths]
    fell, cands = w.expect(Q, lists, k)
    assert (fell, cands) == (4, 120)
    labels, lb = csr(lists)
    w.check(Q, k, labels, lb)
    assert w.stats().tolist() == [1, nq, fell, cands]
    for i, keys in enumerate(lists[:3]):
        w.check(Q, k, keys)
        fell, cands = fell + (nq if keys.size > k + SLACK else 0), cands + (nq * 60 if keys.size == 60 else 0)
        assert w.stats().tolist() == [2 + i, nq * (2 + i), fell, cands]
