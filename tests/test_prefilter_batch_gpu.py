"""vk_index_search_labels_batch (Index.search_labels_batch): nq pre-filter searches in one device pass -- batched K8 over a CSR
of row-slot lists, a per-query select of everything at or below the k-th smallest distance, the reference's heap rule
(vector_base.cc:509-530) over that hand-back on the host.  Every query's ids and distance bits must equal BOTH the single
call (search_labels) and the CPU oracle's heap over the known keys in list order; the counters must show that the device
stage answered exactly the queries it can (no more ties at the k-th distance than the hand-back holds) and no others."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNKNOWN = np.arange(10 ** 6, 10 ** 6 + 40, dtype=np.uint64)
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

    def __init__(self, vsa, oracle, algo, metric, dtype, dim, x, labels=None, **kw):
        self.oracle, self.metric, self.dim = oracle, metric, dim
        self._memo = None
        if metric == "COSINE":
            x = np.stack([oracle.normalize(v)[0] for v in x])
        n = x.shape[0]
        self.labels = (np.arange(n, dtype=np.uint64) + 10) if labels is None else labels
        if algo == "HNSW":
            kw = dict(m=8, ef_construction=40, **kw)
        self.g = vsa.Index(algo, dim, metric, initial_cap=kw.pop("cap", n), dtype=dtype, **kw)
        self.g.add_batch(x, self.labels)
        self.stored = bf16_round(x) if dtype == "bf16" else x
        self.live = {int(l): self.stored[i] for i, l in enumerate(self.labels)}

    def add(self, x, labels, dtype="f32"):
        self.g.add_batch(x, labels)
        st = bf16_round(x) if dtype == "bf16" else x
        for i, l in enumerate(labels):
            self.live[int(l)] = st[i]
        self._memo = None

    def remove(self, labs):
        for l in labs:
            assert self.g.remove(int(l)) == 0
            del self.live[int(l)]
        self._memo = None

    def queries(self, rng, nq):
        Q = rng.standard_normal((nq, self.dim)).astype(np.float32)
        if self.metric == "COSINE":
            Q = np.stack([self.oracle.normalize(v)[0] for v in Q])
        return Q

    def known(self, keys):
        if self._memo is not None and self._memo[0] is keys:           # (a shared list: once, not once per query)
            return self._memo[1]
        lab = [int(l) for l in keys.tolist() if int(l) in self.live]
        rows = np.stack([self.live[l] for l in lab]) if lab else np.zeros((0, self.dim), np.float32)
        self._memo = (keys, (rows, np.array(lab, dtype=np.uint64)))
        return self._memo[1]

    def oracle_topk(self, q, keys, k):
        rows, lab = self.known(keys)
        return self.oracle.prefilter_topk(self.metric, q, rows, lab, k)

    def at_or_below_T(self, q, keys, k):
        """from the oracle's distances: (known entries of the list, how many lie at or below the k-th smallest -- the largest
        when there are fewer than k)"""
        rows, lab = self.known(keys)
        if lab.size == 0:
            return 0, 0
        d, _ = self.oracle.prefilter_topk(self.metric, q, rows, lab, lab.size)   # k = the whole list: every distance, ascending
        assert d.size == lab.size
        T = d[min(k, d.size) - 1]
        return int(lab.size), int((d <= T).sum())

    def check(self, Q, k, labels, list_begin=None, oracle_too=True):
        """the batch against the single call and the oracle, query by query; returns the lists"""
        D, L, N = self.g.search_labels_batch(Q, k, labels, list_begin)
        assert D.shape == (Q.shape[0], k) and L.shape == (Q.shape[0], k)
        lists = []
        for q in range(Q.shape[0]):
            keys = labels if list_begin is None else labels[int(list_begin[q]):int(list_begin[q + 1])]
            lists.append(keys)
            n = int(N[q])
            sd, sl = self.g.search_labels(Q[q], k, keys)
            assert L[q, :n].tolist() == sl.tolist(), (q, len(keys), k)
            assert D[q, :n].view(np.uint32).tolist() == sd.view(np.uint32).tolist(), (q, len(keys), k)
            assert np.all(np.isposinf(D[q, n:])) and np.all(L[q, n:] == NOLABEL)      # the padding past out_n
            if oracle_too:
                od, ol = self.oracle_topk(Q[q], keys, k)
                assert L[q, :n].tolist() == ol.tolist(), (q, len(keys), k)
                assert D[q, :n].view(np.uint32).tolist() == od.view(np.uint32).tolist(), (q, len(keys), k)
        return lists


def make_list(rng, pool, m, dup=True):
    """m keys of the pool (known, removed and unknown labels mixed) in random order; a key repeated at the end"""
    keys = rng.choice(pool, size=min(m, pool.size), replace=False).astype(np.uint64)
    if dup and keys.size >= 2:
        keys = np.concatenate([keys, keys[:1]])
    return keys


def csr(lists):
    lb = np.zeros(len(lists) + 1, np.uint64)
    lb[1:] = np.cumsum([len(l) for l in lists])
    return (np.concatenate(lists) if lists else np.zeros(0, np.uint64)).astype(np.uint64), lb


SHAPES = [  # algo, metric, dtype, dim, nq, k
    ("FLAT", "L2", "f32", 100, 257, 10),
    ("FLAT", "IP", "f32", 768, 64, 64),
    ("FLAT", "COSINE", "bf16", 1100, 3, 1),
    ("FLAT", "L2", "bf16", 1, 64, 10),
    ("FLAT", "IP", "f32", 1, 1, 64),
    ("HNSW", "COSINE", "f32", 100, 64, 10),
    ("HNSW", "L2", "f32", 768, 3, 64),
    ("HNSW", "IP", "bf16", 1, 257, 1),
    ("HNSW", "L2", "bf16", 1100, 1, 10),
]


@pytest.mark.parametrize("shared", [False, True], ids=["lists", "shared"])
@pytest.mark.parametrize("algo,metric,dtype,dim,nq,k", SHAPES)
def test_shapes(vsa, oracle, algo, metric, dtype, dim, nq, k, shared):
    """every list length around k, 1 000 and n; empty lists in the middle of the CSR; unknown labels, labels removed before
    the call (FLAT: rows moved into the holes, HNSW: tombstones) and a repeated label in the lists.  Random normal rows: no
    ties beyond the repeated key, so the device stage answers every query (dim 1 can tie -- bf16 scalars, squares of
    opposite offsets: there the expected number of handed-over queries is counted from the oracle's distances)."""
    rng = np.random.default_rng([ord(algo[0]), ord(metric[0]), dim, nq, k])
    n = 1200 if algo == "FLAT" else 400
    w = World(vsa, oracle, algo, metric, dtype, dim, rng.standard_normal((n, dim)).astype(np.float32))
    removed = rng.choice(w.labels, size=n // 10, replace=False)
    w.remove(removed)
    pool = np.concatenate([w.labels, UNKNOWN])        # (the removed labels are still in the pool)
    Q = w.queries(rng, nq)
    lengths = [0, 1, k - 1, k, k + 1, 1000, n]
    used = []
    if shared:
        for m in lengths:
            used += w.check(Q, k, make_list(rng, pool, m))
        batches, queries = len(lengths), nq * len(lengths)
    else:
        lists = [make_list(rng, pool, lengths[(q + 3) % len(lengths)]) for q in range(nq)]   # (q = 4, 11, ...: empty, mid-CSR)
        labels, lb = csr(lists)
        used = w.check(Q, k, labels, lb)
        batches, queries = 1, nq
    want = sum(w.at_or_below_T(Q[i % nq], keys, k)[1] > k + 64 for i, keys in enumerate(used)) if dim == 1 else 0
    s = w.g.prefilter_stats()
    assert (s.batches, s.queries, s.fallback_queries, s.candidate_cap) == (batches, queries, want, k + 64)


TIES = [("half", "FLAT", 10), ("half", "HNSW", 10), ("few", "FLAT", 1), ("few", "FLAT", 10), ("few", "HNSW", 10),
        ("same", "FLAT", 10), ("same", "FLAT", 1)]


@pytest.mark.parametrize("data,algo,k", TIES)
def test_ties_fall_back_exactly_when_the_hand_back_overflows(vsa, oracle, data, algo, k):
    """half the rows duplicates / rows drawn from 12 (HNSW, 400 rows: 4) distinct vectors / all rows identical.  From the oracle's distances: the
    number of entries of each list at or below its k-th smallest distance; fallback_queries must be EXACTLY the number of
    queries where that exceeds candidate_cap -- a build that always falls back fails, and so does one that never does."""
    rng = np.random.default_rng(77 + k)
    dim, nq = 100, 16
    n = 1200 if algo == "FLAT" else 400
    x = rng.standard_normal((n, dim)).astype(np.float32)
    if data == "half":
        x[n // 2:] = x[:n - n // 2]
    elif data == "few":
        nd = 12 if algo == "FLAT" else 4                 # (a class of ties must outgrow the cap in the long lists only)
        x = x[:nd][rng.integers(0, nd, n)]
    else:
        x[:] = x[0]
    w = World(vsa, oracle, algo, "L2", "f32", dim, x)
    Q = w.queries(rng, nq)
    lengths = [300, 1000, n] if data == "same" else [5, 40, 90, 150, 300, 1000, n]
    lists = [make_list(rng, np.concatenate([w.labels, UNKNOWN]), lengths[q % len(lengths)]) for q in range(nq)]
    labels, lb = csr(lists)
    cap = k + 64
    want = sum(w.at_or_below_T(Q[q], lists[q], k)[1] > cap for q in range(nq))
    w.check(Q, k, labels, lb)
    s = w.g.prefilter_stats()
    assert s.candidate_cap == cap
    assert s.fallback_queries == want, (s.fallback_queries, want)
    if data == "same":
        assert want == nq            # every list is longer than the hand-back and all of it ties
    if data == "few":
        assert 0 < want < nq         # both sides of the cap are in this case
    # the shared list: the same count for every query
    shared = make_list(rng, w.labels, 500)
    want2 = sum(w.at_or_below_T(Q[q], shared, k)[1] > cap for q in range(nq))
    w.check(Q, k, shared)
    assert w.g.prefilter_stats().fallback_queries == want + want2


def test_statistics_add_up(vsa, oracle):
    rng = np.random.default_rng(5)
    n, dim, nq, k = 1000, 100, 20, 10
    w = World(vsa, oracle, "FLAT", "IP", "f32", dim, rng.standard_normal((n, dim)).astype(np.float32))
    Q = w.queries(rng, nq)
    pool = np.concatenate([w.labels, UNKNOWN])
    lists = [make_list(rng, pool, [0, 3, 9, 10, 11, 200, 1000][q % 7], dup=False) for q in range(nq)]
    labels, lb = csr(lists)
    found = [w.at_or_below_T(Q[q], lists[q], k) for q in range(nq)]
    assert all(c == min(k, f) for f, c in found)                      # tie-free: exactly min(k, found) entries at or below T
    w.check(Q, k, labels, lb)
    s1 = w.g.prefilter_stats()
    assert (s1.batches, s1.queries, s1.keys, s1.fallback_queries) == (1, nq, labels.size, 0)
    assert s1.candidates == sum(min(k, f) for f, _ in found)
    assert s1.candidates <= s1.queries * s1.candidate_cap
    shared = make_list(rng, w.labels, 300, dup=False)
    w.check(Q[:7], k, shared)
    s2 = w.g.prefilter_stats()
    assert (s2.batches, s2.queries, s2.keys, s2.fallback_queries) == (2, nq + 7, labels.size + 7 * 300, 0)
    assert s2.candidates == s1.candidates + 7 * k
    assert s2.candidates <= s2.queries * s2.candidate_cap


@pytest.mark.parametrize("algo,metric,dtype", [("FLAT", "COSINE", "f32"), ("FLAT", "L2", "bf16"), ("HNSW", "IP", "f32")])
def test_sharded(vsa, oracle, algo, metric, dtype):
    """four logical shards on one device: each shard's device stage over its part of every list, the union of the candidates
    in the caller's order, the heap rule on the host"""
    rng = np.random.default_rng(11)
    dim, nq, k = 100, 33, 10
    n = 1200 if algo == "FLAT" else 400
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[n - 100:] = x[:100]                                              # some ties across shards
    w = World(vsa, oracle, algo, metric, dtype, dim, x, shard_devices=[0, 0, 0, 0])
    assert w.g.shard_count() == 4
    w.remove(rng.choice(w.labels, size=n // 10, replace=False))
    pool = np.concatenate([w.labels, UNKNOWN])
    Q = w.queries(rng, nq)
    lengths = [0, 1, k - 1, k, k + 1, 1000, n]
    lists = [make_list(rng, pool, lengths[(q + 3) % len(lengths)]) for q in range(nq)]
    lists[5] = w.labels[: n // 4][::-1].copy()                         # a bulk load deals rows [0, n/4) to shard 0: one shard only
    labels, lb = csr(lists)
    w.check(Q, k, labels, lb)
    w.check(Q, k, make_list(rng, pool, 700))
    w.check(Q, k, w.labels[n // 4: n // 2].copy())                     # a shared list that lives on shard 1 alone
    s = w.g.prefilter_stats()
    assert s.fallback_queries == 0 and s.candidate_cap == k + 64 and s.batches >= 3


@pytest.mark.parametrize("algo", ["FLAT", "HNSW"])
def test_after_writes_without_a_flush(vsa, oracle, algo):
    """rows added and removed between calls, no explicit flush: staged and unpublished labels behave as in the single call"""
    rng = np.random.default_rng(23)
    dim, nq, k, n = 100, 9, 10, 300
    x = rng.standard_normal((2 * n, dim)).astype(np.float32)
    w = World(vsa, oracle, algo, "L2", "f32", dim, x[:n], cap=2 * n)
    Q = w.queries(rng, nq)
    more = np.arange(n, 2 * n, dtype=np.uint64) + 10
    everything = np.concatenate([w.labels, more, UNKNOWN])
    lists = [make_list(rng, everything, m) for m in (0, 5, 50, 400, 640, 11, 0, 9, 300)]
    labels, lb = csr(lists)
    w.check(Q, k, labels, lb)                                          # `more` is unknown so far
    w.add(x[n:], more)
    w.check(Q, k, labels, lb)
    w.check(Q, k, lists[4])
    w.remove(rng.choice(np.concatenate([w.labels, more]), size=120, replace=False))
    w.check(Q, k, labels, lb)
    w.check(Q, k, lists[3])
    assert w.g.prefilter_stats().fallback_queries == 0


@pytest.mark.parametrize("shards", [0, 4])
def test_a_k_beyond_the_device_stage_takes_the_single_path(vsa, oracle, shards):
    """the device stage hands back at most k + 64 entries per query for k up to 4096 (kPrefilterMaxK, csrc/prefilter_host.hpp);
    k = 5000 is not covered: every query is answered by the per-query path -- same answer, fallback_queries == nq,
    candidate_cap 0.  k = 4096, the last covered value, is answered by the device stage."""
    rng = np.random.default_rng(31)
    dim, nq, n = 16, 5, 1500
    kw = dict(shard_devices=[0] * shards) if shards else {}
    w = World(vsa, oracle, "FLAT", "L2", "f32", dim, rng.standard_normal((n, dim)).astype(np.float32), **kw)
    Q = w.queries(rng, nq)
    shared = make_list(rng, np.concatenate([w.labels, UNKNOWN]), 1400)
    w.check(Q, 5000, shared)
    s = w.g.prefilter_stats()
    assert s.fallback_queries == nq and s.candidate_cap == 0 and s.candidates == 0
    w.check(Q, 4096, shared, oracle_too=False)
    s = w.g.prefilter_stats()
    assert s.fallback_queries == nq and s.candidate_cap == 4096 + 64


def test_argument_errors_and_the_trivial_calls(vsa):
    import ctypes as C
    g = vsa.Index("FLAT", 8, "L2", initial_cap=16)
    g.add_batch(np.eye(8, dtype=np.float32))
    Q = np.zeros((2, 8), np.float32)
    lab = np.arange(8, dtype=np.uint64)
    D, L, N = g.search_labels_batch(Q, 0, lab)                         # k == 0: every out_n is 0
    assert N.tolist() == [0, 0]
    D, L, N = g.search_labels_batch(Q[:0], 3, lab)                     # nq == 0: nothing
    assert N.size == 0
    with pytest.raises(vsa.VkError) as e:
        g.search_labels_batch(Q, 3, lab, np.array([0, 5, 4], np.uint64))
    assert e.value.code == vsa.VK_ERR_INVALID
    with pytest.raises(vsa.VkError) as e:
        g.search_labels_batch(Q, 3, lab, np.array([0, 4, 7], np.uint64))
    assert e.value.code == vsa.VK_ERR_INVALID
    D, L, N = g.search_labels_batch(Q, 3, lab, np.array([0, 0, 8], np.uint64))
    assert N.tolist() == [0, 3]
    s = vsa.PrefilterStats()
    s.struct_size = 8
    assert vsa.lib().vk_index_prefilter_stats(g._h, C.byref(s)) == vsa.VK_ERR_INVALID
