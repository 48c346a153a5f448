"""HNSW node masks (options hnsw-node-mask / hnsw-node-mask-bytes; csrc/node_mask.hip, csrc/node_mask_cache.hpp).

A device filter is a bitmap over labels; the graph is walked by internal ids.  Per (filter, graph publication) the index
builds one bit per node, "live and allowed", and the search kernel tests that bit instead of tombstone word -> label ->
filter word.  Pinned here:
  * the mask equals the numpy expression over (labels in insertion order, tombstones, filter bits) word for word, its
    population count included;
  * option 0 and option 1 give identical ids, distance bits, out_n, last_n_eval and last_n_hops, and both equal the CPU
    oracle on the same graph;
  * the cache: built once, hit afterwards, rebuilt after a flush that changed the graph, kept by one that did not, bounded
    by hnsw-node-mask-bytes with the label path as the fallback, released by option 0;
  * unfiltered searches over tombstones, four logical shards, and the dispatcher."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


def _build(vsa, oracle, metric="L2", dtype="f32", n=4000, dim=32, dead_share=0.0, seed=1, M=8, **kw):
    """a graph whose rows arrive in shuffled label order (one host thread: internal id = arrival order), some removed"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    if metric == "COSINE":
        x = np.stack([oracle.normalize(v)[0] for v in x])
    labels = rng.permutation(n + n // 4)[:n].astype(np.uint64)        # sparse labels: the largest is beyond n
    g = vsa.Index("HNSW", dim, metric, initial_cap=n + 64, m=M, ef_construction=60, build_threads=1, dtype=dtype, **kw)
    g.add_batch(x, labels)
    dead = rng.choice(n, int(n * dead_share), replace=False)
    for i in dead:
        assert g.remove(int(labels[i])) == 0
    g.flush()
    live = np.ones(n, bool)
    live[dead] = False
    return {"g": g, "x": x, "labels": labels, "live": live, "n": n, "dim": dim, "metric": metric, "M": M, "rng": rng,
            "nbits": int(labels.max()) + 1}


def _oracle_of(oracle, b):
    return oracle.HNSW.from_product_index(b["g"].save_raw, b["dim"], b["metric"], b["M"], ef_construction=60)


def _queries(oracle, b, nq):
    Q = b["rng"].standard_normal((nq, b["dim"])).astype(np.float32)
    if b["metric"] == "COSINE":
        Q = np.stack([oracle.normalize(v)[0] for v in Q])
    return Q


def _want_mask(labels, live, bits, nbits, n_words=None):
    lab = labels.astype(np.int64)
    ok = live & (lab < nbits)
    idx = np.flatnonzero(ok)
    ok[idx] = ((bits[lab[idx] >> 6] >> (lab[idx] & 63).astype(np.uint64)) & np.uint64(1)).astype(bool)
    words = (len(labels) + 63) // 64 if n_words is None else n_words
    out = np.zeros(words * 64, bool)
    out[:len(ok)] = ok
    return np.packbits(out.reshape(-1, 64), axis=1, bitorder="little").view(np.uint64).reshape(-1), int(ok.sum())


def _counters(g):
    s = g.stats()
    return s.last_n_eval, s.last_n_hops, s.last_frontier_dropped


def _same(a, b):
    (D1, L1, N1), (D2, L2, N2) = a, b
    assert N1.tolist() == N2.tolist() and L1.tolist() == L2.tolist() and D1.view(np.uint32).tolist() == D2.view(np.uint32).tolist()


def _on_off(g, run):
    """run() with the option off and on: identical answers and counters; returns the answer and the on-run's mask statistics"""
    g.set_option("hnsw-node-mask", 0)
    off = run()
    c_off = _counters(g)
    g.set_option("hnsw-node-mask", 1)
    on = run()
    c_on = _counters(g)
    _same(off, on)
    assert c_off == c_on and c_on[2] == 0, (c_off, c_on)
    return on, g.node_mask_stats()


# ---- mask content -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4000, 4033, 63])
def test_the_mask_is_live_and_allowed_by_internal_id(vsa, oracle, n):
    b = _build(vsa, oracle, n=n, dead_share=0.1, seed=n)
    g, labels, live, rng = b["g"], b["labels"], b["live"], b["rng"]
    g.set_option("hnsw-node-mask", 1)
    top = int(labels.max())
    cases = [("half", top + 1, labels[rng.random(n) < 0.5]),
             ("short", top // 2, labels[rng.random(n) < 0.5]),            # nbits below the largest label: those are rejected
             ("empty", top + 1, np.zeros(0, np.uint64)),
             ("full", top + 1, None)]
    for name, nbits, ids in cases:
        if ids is None:
            f = g.make_filter(nbits, runs=np.array([[0, nbits - 1]], dtype=np.uint64))
        else:
            f = g.make_filter(nbits, labels=ids)
        bits = f.read()
        words, admitted = g.node_mask_read(f)
        want, want_n = _want_mask(labels, live, bits, nbits)
        assert words.tolist() == want.tolist(), name
        assert admitted == want_n == int(sum(bin(int(w)).count("1") for w in words)), name
        if n % 64:
            assert int(words[-1]) >> (n % 64) == 0                         # tail bits are zero
    # more words than the graph has: zero filled
    words, _ = g.node_mask_read(f, n_words=(n + 63) // 64 + 3)
    assert words[-3:].tolist() == [0, 0, 0]
    # the option off: the mask is still built for the reader, nothing is cached
    g.set_option("hnsw-node-mask", 0)
    assert g.node_mask_stats().resident_entries == 0
    words2, adm2 = g.node_mask_read(f)
    assert words2.tolist() == want.tolist() and adm2 == want_n and g.node_mask_stats().resident_entries == 0


def test_read_is_refused_on_flat(vsa):
    f = vsa.Index("FLAT", 16, "L2", initial_cap=128)
    f.add_batch(np.ones((4, 16), np.float32))
    fl = f.make_filter(8, labels=np.arange(3, dtype=np.uint64))
    with pytest.raises(vsa.VkError) as e:
        f.node_mask_read(fl, n_words=1)
    assert e.value.code == vsa.VK_ERR_INVALID
    assert f.node_mask_stats().masks_built == 0


# ---- on = off = oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,dtype,dead_share", [("L2", "f32", 0.0), ("IP", "bf16", 0.01), ("COSINE", "f32", 0.3),
                                                     ("L2", "bf16", 0.3), ("IP", "f32", 0.0), ("COSINE", "bf16", 0.01)])
def test_option_on_equals_option_off_equals_the_oracle(vsa, oracle, metric, dtype, dead_share):
    b = _build(vsa, oracle, metric=metric, dtype=dtype, dead_share=dead_share, seed=7)
    g, labels, n, nbits, rng = b["g"], b["labels"], b["n"], b["nbits"], b["rng"]
    o = _oracle_of(oracle, b)
    Q = _queries(oracle, b, 24)
    sets = [labels[rng.random(n) < p] for p in (0.5, 0.05, 0.001)]
    sets[2] = np.union1d(sets[2], labels[:2])                             # (never empty)
    bitmaps = [oracle.allow_bitmap(s, nbits) for s in sets]
    handles = [g.make_filter(nbits, labels=s) for s in sets]
    k = 10
    for ef in (10, 64, 300, 600, 1024):        # result list in registers (<= 512), in LDS (beyond); the frontier in HBM throughout
        for w in range(3):                                                # one handle for the whole batch (single-query entry point)
            for i in (0, 1):
                def run(i=i, w=w, ef=ef):
                    d, l = g.search_filter(Q[i], k, handles[w], ef=ef)
                    return d[None, :], l[None, :], np.array([len(l)])
                (D, L, N), st = _on_off(g, run)
                assert st.last_batch_served == 1
                od, ol = o.search(Q[i], k, ef=ef, allow=bitmaps[w], allow_nbits=nbits)
                assert L[0].tolist() == ol.tolist() and D[0].view(np.uint32).tolist() == od.view(np.uint32).tolist()
        which = [None if i % 4 == 3 else i % 3 for i in range(len(Q))]    # one per query, NULL entries mixed in
        (D, L, N), st = _on_off(g, lambda: g.search_batch_filter_handles(Q, k, [None if w is None else handles[w] for w in which], ef=ef))
        assert st.last_batch_served == sum(w is not None for w in which)
        for i in range(0, len(Q), 2):
            w = which[i]
            od, ol = o.search(Q[i], k, ef=ef, allow=None if w is None else bitmaps[w], allow_nbits=nbits)
            assert L[i, :N[i]].tolist() == ol.tolist() and D[i, :N[i]].view(np.uint32).tolist() == od.view(np.uint32).tolist()


def test_the_redo_launch_reads_the_mask_too(vsa, oracle):
    b = _build(vsa, oracle, n=6000, dead_share=0.01, seed=11)
    g, labels, n, nbits, rng = b["g"], b["labels"], b["n"], b["nbits"], b["rng"]
    # the smallest frontier memory the options allow (fewer resident waves) and a first-launch frontier of 128 entries per wave
    # (the byte budget alone never shrinks a wave's frontier): sparse filters outgrow it and the graph-sized launch answers
    g.set_option("hnsw-pool-bytes", 1 << 20)
    g.set_option("hnsw-gpool-cap", 128)
    o = _oracle_of(oracle, b)
    Q = _queries(oracle, b, 32)
    s = labels[rng.random(n) < 0.02]
    f, bits = g.make_filter(nbits, labels=s), oracle.allow_bitmap(s, nbits)
    (D, L, N), st = _on_off(g, lambda: g.search_batch_filter_handles(Q, 10, [f] * len(Q), ef=64))
    assert g.stats().last_frontier_redo > 0 and st.last_batch_served == len(Q)
    for i in range(0, len(Q), 4):
        od, ol = o.search(Q[i], 10, ef=64, allow=bits, allow_nbits=nbits)
        assert L[i, :N[i]].tolist() == ol.tolist() and D[i, :N[i]].view(np.uint32).tolist() == od.view(np.uint32).tolist()


@pytest.mark.parametrize("dead_share", [0.01, 0.3])
def test_tombstones_without_a_filter(vsa, oracle, dead_share):
    b = _build(vsa, oracle, dead_share=dead_share, seed=13)
    g = b["g"]
    o = _oracle_of(oracle, b)
    Q = _queries(oracle, b, 40)
    for ef in (10, 100, 600):
        (D, L, N), st = _on_off(g, lambda: g.search_batch(Q, 10, ef=ef))
        assert st.last_batch_served == 0 and st.masks_built == 0          # (the live bitmap is no cached mask)
        for i in range(0, len(Q), 5):
            od, ol = o.search(Q[i], 10, ef=ef)
            assert L[i, :N[i]].tolist() == ol.tolist() and D[i, :N[i]].view(np.uint32).tolist() == od.view(np.uint32).tolist()
        def one(ef=ef):                                                      # ... and the single-query entry point
            d, l = g.search(Q[0], 10, ef=ef)
            return d[None, :], l[None, :], np.array([len(l)])
        _on_off(g, one)


# ---- cache behaviour ---------------------------------------------------------------------------------------------------------
def test_built_once_then_hit_and_rebuilt_after_the_graph_changed(vsa, oracle):
    b = _build(vsa, oracle, seed=17)
    g, x, labels, n, nbits, rng = b["g"], b["x"], b["labels"], b["n"], b["nbits"], b["rng"]
    g.set_option("hnsw-node-mask", 1)
    target = int(labels[5])
    new_label = nbits + 7
    f = g.make_filter(new_label + 1, labels=np.concatenate([labels[:200], np.array([new_label], np.uint64)]))
    q = x[5]
    s0 = g.node_mask_stats()
    d, l = g.search_filter(q, 5, f, ef=64)
    assert l[0] == target
    s1 = g.node_mask_stats()
    assert (s1.masks_built - s0.masks_built, s1.cache_hits - s0.cache_hits, s1.resident_entries) == (1, 0, 1)
    assert s1.resident_bytes == (n + 63) // 64 * 8
    g.search_filter(q, 5, f, ef=64)
    g.flush()                                                              # nothing changed: the entry stays
    g.search_filter(q, 5, f, ef=64)
    s2 = g.node_mask_stats()
    assert (s2.masks_built - s1.masks_built, s2.cache_hits - s1.cache_hits) == (0, 2)
    # add + remove + flush: the mask is rebuilt; the removed label is gone although the filter still allows it, the new one is in
    assert g.add(new_label, q) == 0 and g.remove(target) == 0
    g.flush()
    assert g.node_mask_stats().resident_entries == 0                      # stale masks go with the publication
    d, l = g.search_filter(q, 5, f, ef=64)
    assert target not in l.tolist() and l[0] == new_label
    s3 = g.node_mask_stats()
    assert s3.masks_built - s2.masks_built == 1 and s3.evictions == 0
    words, admitted = g.node_mask_read(f)
    live = np.ones(n + 1, bool)
    live[5] = False
    want, want_n = _want_mask(np.concatenate([labels, np.array([new_label], np.uint64)]), live, f.read(), new_label + 1)
    assert words.tolist() == want.tolist() and admitted == want_n


def test_a_reused_slot_is_judged_by_its_new_label(vsa, oracle):
    b = _build(vsa, oracle, n=2000, seed=19, allow_replace_deleted=1)
    g, x, labels, n, nbits = b["g"], b["x"], b["labels"], b["n"], b["nbits"]
    g.set_option("hnsw-node-mask", 1)
    allowed_new, rejected_new = nbits + 1, nbits + 2
    f = g.make_filter(nbits + 3, labels=np.concatenate([labels[:300], np.array([allowed_new], np.uint64)]))
    q = x[9]
    assert g.search_filter(q, 3, f, ef=50)[1][0] == labels[9]
    for new in (rejected_new, allowed_new):
        # between two flushes: the label goes, its slot comes back under another label -- the slot's live bit never changes
        holder = int(labels[9]) if new == rejected_new else rejected_new
        assert g.remove(holder) == 0 and g.add(new, q) == 0
        g.flush()
        st = g.stats()
        assert st.count == n and st.deleted == 0                          # (the slot was reused)
        g.set_option("hnsw-node-mask", 0)
        off = g.search_filter(q, 3, f, ef=50)
        g.set_option("hnsw-node-mask", 1)
        on = g.search_filter(q, 3, f, ef=50)
        assert on[1].tolist() == off[1].tolist() and on[0].view(np.uint32).tolist() == off[0].view(np.uint32).tolist()
        assert (new in on[1].tolist()) == (new == allowed_new) and int(labels[9]) not in on[1].tolist()
        words, _ = g.node_mask_read(f)
        assert (int(words[9 >> 6]) >> 9) & 1 == (1 if new == allowed_new else 0)


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def test_the_byte_budget_and_the_fallback(vsa, oracle):
    b = _build(vsa, oracle, seed=23)
    g, labels, n, nbits, rng = b["g"], b["labels"], b["n"], b["nbits"], b["rng"]
    Q = _queries(oracle, b, 20)
    mask_bytes = (n + 63) // 64 * 8
    handles = [g.make_filter(nbits, labels=labels[rng.random(n) < 0.2]) for _ in range(5)]
    per_query = [handles[i % 5] for i in range(len(Q))]
    g.set_option("hnsw-node-mask", 0)
    bytes_off = g.stats().device_bytes
    want = g.search_batch_filter_handles(Q, 10, per_query, ef=80)
    c_want = _counters(g)
    g.set_option("hnsw-node-mask", 1)
    # below one mask: nothing is built, the answers are the label path's
    g.set_option("hnsw-node-mask-bytes", mask_bytes - 1)
    _same(g.search_batch_filter_handles(Q, 10, per_query, ef=80), want)
    st = g.node_mask_stats()
    assert (st.last_batch_served, st.resident_entries, st.masks_built) == (0, 0, 0) and _counters(g) == c_want
    # room for two of five: two filters of the batch get a mask, the others fall back; one filter after another evicts
    g.set_option("hnsw-node-mask-bytes", 2 * mask_bytes)
    _same(g.search_batch_filter_handles(Q, 10, per_query, ef=80), want)
    st = g.node_mask_stats()
    assert (st.last_batch_served, st.resident_entries, st.resident_bytes, st.evictions) == (8, 2, 2 * mask_bytes, 0)
    assert _counters(g) == c_want and g.stats().device_bytes == bytes_off + 2 * mask_bytes
    for i in range(5):
        d, l = g.search_filter(Q[i], 10, handles[i], ef=80)
        assert l.tolist() == want[1][i, :want[2][i]].tolist()
    st = g.node_mask_stats()
    assert st.evictions == 3 and st.resident_entries == 2 and st.resident_bytes == 2 * mask_bytes
    # option 0 releases them
    g.set_option("hnsw-node-mask", 0)
    st = g.node_mask_stats()
    assert (st.resident_entries, st.resident_bytes) == (0, 0) and g.stats().device_bytes == bytes_off
    g.set_option("hnsw-node-mask-bytes", 1 << 30)


# ---- sharded, dispatcher --------------------------------------------------------------------------------------------------------
def test_four_logical_shards_with_one_handle_per_query(vsa, oracle):
    rng = np.random.default_rng(29)
    n, dim, S = 4000, 32, 4
    x = rng.standard_normal((n, dim)).astype(np.float32)
    kw = dict(m=8, ef_construction=60, build_threads=1)
    sh = vsa.Index("HNSW", dim, "L2", initial_cap=n, shard_devices=[0] * S, **kw)
    sh.add_batch(x)                                                        # rows [s*n/S, (s+1)*n/S) to shard s
    singles = []
    for s in range(S):
        lo, hi = s * n // S, (s + 1) * n // S
        g = vsa.Index("HNSW", dim, "L2", initial_cap=max(1024, hi - lo), **kw)
        g.add_batch(x[lo:hi], np.arange(lo, hi, dtype=np.uint64))
        singles.append(g)
    for lab in rng.choice(n, 100, replace=False):
        assert sh.remove(int(lab)) == 0 and singles[int(lab) * S // n].remove(int(lab)) == 0
    sets = [np.flatnonzero(rng.random(n) < p).astype(np.uint64) for p in (0.4, 0.1, 0.02)]
    bitmaps = [oracle.allow_bitmap(s, n) for s in sets]
    handles = [sh.make_filter(n, labels=s) for s in sets]
    Q = rng.standard_normal((18, dim)).astype(np.float32)
    which = [None if i % 6 == 5 else i % 3 for i in range(len(Q))]
    per_query = [None if w is None else handles[w] for w in which]
    sh.set_option("hnsw-node-mask", 0)
    off = sh.search_batch_filter_handles(Q, 10, per_query, ef=100)
    sh.set_option("hnsw-node-mask", 1)
    s0 = sh.node_mask_stats()
    D, L, N = on = sh.search_batch_filter_handles(Q, 10, per_query, ef=100)
    _same(off, on)
    for i in range(len(Q)):
        w = which[i]
        parts = [g.search(Q[i], 10, ef=100, allow=None if w is None else bitmaps[w], allow_nbits=None if w is None else n) for g in singles]
        want = sorted((float(d), int(l)) for Dp, Lp in parts for d, l in zip(Dp, Lp))[:10]
        assert [int(v) for v in L[i, :N[i]]] == [l for _, l in want] and [float(v) for v in D[i, :N[i]]] == [d for d, _ in want]
    s1 = sh.node_mask_stats()
    served = sum(w is not None for w in which)
    assert s1.masks_built - s0.masks_built == 3 * S and s1.resident_entries == 3 * S        # one cache per shard's graph: the sum
    assert s1.last_batch_served == served * S and s1.resident_bytes == 3 * S * ((n // S + 63) // 64 * 8)
    with pytest.raises(vsa.VkError) as e:
        sh.node_mask_read(handles[0], n_words=4)
    assert e.value.code == vsa.VK_ERR_INVALID


def test_submitted_searches_from_several_threads(vsa, oracle):
    b = _build(vsa, oracle, dead_share=0.05, seed=31)
    g, labels, n, nbits, rng = b["g"], b["labels"], b["n"], b["nbits"], b["rng"]
    g.set_option("hnsw-node-mask", 1)
    Q = _queries(oracle, b, 96)
    sets = [labels[rng.random(n) < p] for p in (0.5, 0.05)]
    handles = [g.make_filter(nbits, labels=s) for s in sets]
    bitmap = oracle.allow_bitmap(sets[0], nbits)
    # query i: a handle, a host bitmap (no mask: nothing to cache), or nothing -- all in the same device batches
    kind = [i % 4 for i in range(len(Q))]
    want = []
    for i in range(len(Q)):
        if kind[i] < 2:
            want.append(g.search_filter(Q[i], 10, handles[kind[i]], ef=80))
        elif kind[i] == 2:
            want.append(g.search(Q[i], 10, ef=80, allow=bitmap, allow_nbits=nbits))
        else:
            want.append(g.search(Q[i], 10, ef=80))
    g.set_coalescing(64, 2000)
    try:
        done = threading.Semaphore(0)
        pend = [None] * len(Q)

        def worker(t):
            for i in range(t, len(Q), 4):
                if kind[i] < 2:
                    pend[i] = g.submit_filter(Q[i], 10, lambda st: done.release(), handles[kind[i]], ef=80)
                elif kind[i] == 2:
                    pend[i] = g.submit(Q[i], 10, lambda st: done.release(), ef=80, allow=bitmap, allow_nbits=nbits)
                else:
                    pend[i] = g.submit(Q[i], 10, lambda st: done.release(), ef=80)

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        for _ in pend:
            assert done.acquire(timeout=60)
        for i, p in enumerate(pend):
            d, l = p.result()
            assert p.status == 0 and l.tolist() == want[i][1].tolist() and d.view(np.uint32).tolist() == want[i][0].view(np.uint32).tolist()
    finally:
        g.set_coalescing(0, 0)
    assert g.node_mask_stats().cache_hits > 0 and g.stats().last_frontier_dropped == 0
