"""vk_index_search_labels_submit through the C ABI: single pre-filter requests collected by the dispatcher into
vk_index_search_labels_batch calls (csrc/dispatcher.hpp: lanes of their own kind, keyed by k).

With vk_index_set_coalescing(8, 1 000 000), eight submissions from one thread travel in ONE batch: vk_prefilter_stats.batches
moves by one and queries by eight, coalesced_batches / coalesced_queries / submitted and the latency histogram count them,
and every answer is bit for bit the blocking call's (vk_index_search_labels).  Distinct lists go as a CSR; eight submissions of
the same (pointer, length) take the shared path, which the counters show: `keys` counts the list once per query and, with
prefilter-device-resolve on, device_resolved_keys counts it once.  The same through vk_index_set_batch_completion; VK_ERR_BUSY
at max-query-queue-depth = 1; VK_ERR_INVALID with coalescing off; vk_index_destroy answers what is still queued.

The submissions of a burst are made back to back from buffers prepared beforehand (the batching window closes after 200 us
without an arrival); nothing sleeps."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
OPT = "prefilter-device-resolve"


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


class Completion(C.Structure):
    """vk_completion"""
    _fields_ = [("user", C.c_void_p), ("status", C.c_int32), ("reserved", C.c_uint32)]


BATCH_DONE = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(Completion), C.c_uint64)


def make_index(vsa, algo):
    rng = np.random.default_rng([7, len(algo)])
    n, dim = 2000, 100
    x = rng.standard_normal((n, dim)).astype(np.float32)
    kw = dict(m=8, ef_construction=40) if algo == "HNSW" else {}
    g = vsa.Index(algo, dim, "L2", initial_cap=n, **kw)
    labels = np.arange(n, dtype=np.uint64) * 5 + 3
    g.add_batch(x, labels)
    for l in labels[::9]:
        assert g.remove(int(l)) == 0
    g.flush()
    pool = np.concatenate([labels, np.arange(10 ** 8, 10 ** 8 + 30, dtype=np.uint64)])
    Q = rng.standard_normal((8, dim)).astype(np.float32)
    return g, rng, pool, Q


class Burst:
    """n submissions prepared beforehand and made back to back; completions by callback (or by the bulk hook)"""

    def __init__(self, vsa, g, Q, k, lists):
        self.vsa, self.g, self.Q, self.k, self.lists = vsa, g, np.ascontiguousarray(Q), k, lists
        n = len(lists)
        self.d = np.zeros((n, k), np.float32)
        self.l = np.zeros((n, k), np.uint64)
        self.n = np.zeros(n, np.uint64)
        self.status = {}
        self.calls = 0
        self.sem = threading.Semaphore(0)

        def _done(user, status):
            self.calls += 1
            self.status[int(user or 0)] = status
            self.sem.release()

        self.cb = vsa.SEARCH_DONE(_done)

    def fire(self):
        fn, h = self.vsa.lib().vk_index_search_labels_submit, self.g._h
        args = [(h, self.Q[i].ctypes.data, self.k, self.lists[i].ctypes.data, self.lists[i].size, self.d[i].ctypes.data, self.l[i].ctypes.data,
                 self.n[i:].ctypes.data, self.cb, C.c_void_p(i + 1)) for i in range(len(self.lists))]
        return [fn(*a) for a in args]

    def wait(self, count, sem=None):
        for _ in range(count):
            assert (sem or self.sem).acquire(timeout=60), "a submitted request was never completed"

    def check(self, which=None):
        """every answer bit for bit the blocking call's"""
        for i in (range(len(self.lists)) if which is None else which):
            sd, sl = self.g.search_labels(self.Q[i], self.k, self.lists[i])
            m = int(self.n[i])
            assert self.l[i, :m].tolist() == sl.tolist() and self.d[i, :m].view(np.uint32).tolist() == sd.view(np.uint32).tolist(), i


def moved(g, before):
    p, s = g.prefilter_stats(), g.stats()
    now = dict(batches=p.batches, queries=p.queries, keys=p.keys, resolved=p.device_resolved_keys, cb=s.coalesced_batches,
               cq=s.coalesced_queries, submitted=s.submitted, rejected=s.rejected, hist=sum(s.latency_hist))
    return now if before is None else {f: now[f] - before[f] for f in now}, now


@pytest.mark.parametrize("algo", ["FLAT", "HNSW"])
def test_eight_submissions_travel_in_one_batch(vsa, algo):
    g, rng, pool, Q = make_index(vsa, algo)
    g.set_coalescing(8, 1_000_000)
    try:
        for option in (0, 1):
            g.set_option(OPT, option)
            # distinct lists: a CSR
            lists = [np.ascontiguousarray(rng.choice(pool, size=m, replace=False)) for m in (300, 1, 0, 64, 65, 700, 257, 12)]
            b = Burst(vsa, g, Q, 10, lists)
            _, at = moved(g, None)
            assert b.fire() == [vsa.VK_OK] * 8
            b.wait(8)
            d, _ = moved(g, at)
            assert d["batches"] == 1 and d["queries"] == 8 and d["cb"] == 1 and d["cq"] == 8 and d["submitted"] == 8 and d["hist"] == 8
            total = sum(l.size for l in lists)
            assert d["keys"] == total and d["resolved"] == (total if option else 0)
            assert b.calls == 8 and b.status == {i + 1: vsa.VK_OK for i in range(8)}
            b.check()
            # the same (pointer, length) eight times: one shared list
            one = np.ascontiguousarray(rng.choice(pool, size=500, replace=False))
            b = Burst(vsa, g, Q, 10, [one] * 8)
            _, at = moved(g, None)
            assert b.fire() == [vsa.VK_OK] * 8
            b.wait(8)
            d, _ = moved(g, at)
            assert d["batches"] == 1 and d["queries"] == 8 and d["keys"] == 8 * one.size and d["resolved"] == (one.size if option else 0)
            b.check()
            # equal contents at another address are not "the same list"
            b = Burst(vsa, g, Q, 10, [one] * 7 + [one.copy()])
            _, at = moved(g, None)
            assert b.fire() == [vsa.VK_OK] * 8
            b.wait(8)
            d, _ = moved(g, at)
            assert d["batches"] == 1 and d["keys"] == 8 * one.size and d["resolved"] == (8 * one.size if option else 0)
            b.check()
    finally:
        g.set_coalescing(0, 0)


@pytest.mark.parametrize("algo", ["FLAT", "HNSW"])
def test_completions_through_the_bulk_hook(vsa, algo):
    g, rng, pool, Q = make_index(vsa, algo)
    g.set_option(OPT, 1)
    g.set_coalescing(8, 1_000_000)
    told, sem = [], threading.Semaphore(0)

    def _hook(_hook_user, items, n):
        for i in range(n):
            told.append((int(items[i].user or 0), items[i].status))
        for _ in range(n):
            sem.release()

    hook = BATCH_DONE(_hook)
    lib = vsa.lib()
    lib.vk_index_set_batch_completion.argtypes = [C.c_void_p, BATCH_DONE, C.c_void_p]
    assert lib.vk_index_set_batch_completion(g._h, hook, None) == vsa.VK_OK
    try:
        lists = [np.ascontiguousarray(rng.choice(pool, size=m, replace=False)) for m in (100, 200, 0, 63, 64, 65, 900, 5)]
        b = Burst(vsa, g, Q, 10, lists)
        _, at = moved(g, None)
        assert b.fire() == [vsa.VK_OK] * 8
        b.wait(8, sem)
        d, _ = moved(g, at)
        assert d["batches"] == 1 and d["queries"] == 8 and d["hist"] == 8 and d["resolved"] == sum(l.size for l in lists)
        assert sorted(told) == [(i + 1, vsa.VK_OK) for i in range(8)] and b.calls == 0      # once each, through the hook only
        b.check()
    finally:
        assert lib.vk_index_set_batch_completion(g._h, BATCH_DONE(), None) == vsa.VK_OK
        g.set_coalescing(0, 0)


def test_a_full_queue_coalescing_off_and_destroy(vsa):
    g, rng, pool, Q = make_index(vsa, "FLAT")
    lists = [np.ascontiguousarray(rng.choice(pool, size=200, replace=False)) for _ in range(8)]
    b = Burst(vsa, g, Q, 10, lists)
    assert b.fire() == [vsa.VK_ERR_INVALID] * 8 and b.calls == 0                     # coalescing is off
    assert b"coalescing" in vsa.lib().vk_last_error()
    # a queue of depth 1 under a burst: the first request waits for company, what comes behind it is refused
    g.set_option("max-query-queue-depth", 1)
    g.set_coalescing(8, 1_000_000)
    _, at = moved(g, None)
    rcs = b.fire()
    ok = [i for i, rc in enumerate(rcs) if rc == vsa.VK_OK]
    assert rcs[0] == vsa.VK_OK and set(rcs) == {vsa.VK_OK, vsa.VK_ERR_BUSY}
    b.wait(len(ok))
    d, _ = moved(g, at)
    assert d["rejected"] == len(rcs) - len(ok) and d["submitted"] == len(ok) and b.calls == len(ok)
    b.check(ok)
    # vk_index_destroy answers what is still queued
    g.set_option("max-query-queue-depth", 100000)
    b = Burst(vsa, g, Q[:3], 10, lists[:3])
    want = [g.search_labels(Q[i], 10, lists[i]) for i in range(3)]
    assert b.fire() == [vsa.VK_OK] * 3
    g.close()
    assert b.calls == 3 and b.status == {1: vsa.VK_OK, 2: vsa.VK_OK, 3: vsa.VK_OK}   # (fired before destroy returned)
    for i, (sd, sl) in enumerate(want):
        m = int(b.n[i])
        assert b.l[i, :m].tolist() == sl.tolist() and b.d[i, :m].view(np.uint32).tolist() == sd.view(np.uint32).tolist()
