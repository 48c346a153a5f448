"""Filters derived on the device from an older filter plus a delta of labels (vk_filter_apply_delta[_batch],
csrc/filter_delta.cc, the delta kernels of csrc/filter_build.hip).

The tag index mutates per key (src/indexes/tag.cc AddRecord / ModifyRecord / RemoveRecord) and the schema switches from
writing back to reading every few milliseconds (src/index_schema.cc:285-292); the filter of a predicate after a write phase
is the filter before it with a few bits changed and perhaps a longer label range.  Pinned here, every comparison exact
(these are integers):
  * the derived bitmap and its population count equal a numpy model and a vk_filter_create of the model's id list, over
    growth by 0 / 1 / 63 / 64 / 65 bits and many words, duplicates, a label in both lists, labels beyond nbits, no base;
  * the base is untouched, may be released at once, and a search in flight with it sees it;
  * a batch equals its single calls; one bad item fails the whole call and leaves no handle behind;
  * fifty deltas in a row do not drift;
  * FLAT / HNSW, plain and sharded: a search with the derived filter answers like one with the rebuilt filter and like
    the CPU oracle;
  * the adaptor's maintained predicates (include/vk_vector_adaptor.h) over write phases from several writer threads."""
import ctypes as C
import subprocess
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


@pytest.fixture(scope="module")
def ix(vsa):
    g = vsa.Index("FLAT", 8, "L2", initial_cap=1024)
    g.add_batch(np.zeros((4, 8), np.float32))
    return g


def words_of(model):
    """the bitmap of a boolean model: bit i of word i // 64, zero padding behind the last label"""
    nb = model.size
    by = np.packbits(model, bitorder="little")
    pad = (-by.size) % 8
    return np.concatenate([by, np.zeros(pad, np.uint8)]).view(np.uint64) if nb else np.zeros(0, np.uint64)


def check(f, model):
    assert f.info() == (model.size, int(model.sum()))
    assert np.array_equal(f.read(), words_of(model))


def random_base(g, rng, nbits):
    """ids + runs + host bits -> (filter, boolean model)"""
    model = np.zeros(nbits, bool)
    ids = rng.integers(0, max(nbits, 1) + 50, size=int(rng.integers(0, 3000)), dtype=np.uint64)
    model[ids[ids < nbits].astype(np.int64)] = True
    lo = rng.integers(0, max(nbits, 1), size=5)
    runs = np.stack([lo, lo + rng.integers(0, 300, size=5)], axis=1).astype(np.uint64)
    for a, b in runs.tolist():
        model[a:min(b, nbits - 1) + 1] = True
    host = rng.random(nbits) < 0.1
    model |= host
    return g.make_filter(nbits, labels=ids, runs=runs, base_bits=words_of(host) if nbits else None), model


def random_delta(rng, old_bits, nbits):
    """(set, clear, model update): duplicates, a label in both lists, labels >= nbits, sometimes empty"""
    def some(n):
        a = rng.integers(0, nbits + 100, size=n, dtype=np.uint64)
        return np.concatenate([a, a[: n // 3]])                      # duplicates
    st = some(int(rng.integers(0, 2000))) if rng.random() < 0.85 else np.zeros(0, np.uint64)
    cl = some(int(rng.integers(0, 2000))) if rng.random() < 0.85 else np.zeros(0, np.uint64)
    if st.size and cl.size:
        cl = np.concatenate([cl, st[:5]])                             # in both lists: ends up set
    return st, cl


def apply_model(model, nbits, st, cl):
    out = np.zeros(nbits, bool)
    out[: model.size] = model
    out[cl[cl < nbits].astype(np.int64)] = False
    out[st[st < nbits].astype(np.int64)] = True                      # clears first, then sets
    return out


def test_a_derived_filter_equals_a_rebuild(vsa, ix):
    rng = np.random.default_rng(701)
    for nbits0 in (1_000_003, 640, 100, 1):
        for grow in (0, 1, 63, 64, 65, 200_001):
            base, model = random_base(ix, rng, nbits0)
            nbits = nbits0 + grow
            st, cl = random_delta(rng, nbits0, nbits)
            got = ix.filter_apply_delta(base, nbits, set=st, clear=cl)
            want = apply_model(model, nbits, st, cl)
            print(f"nbits {nbits0} -> {nbits}: base {int(model.sum())} set {st.size} clear {cl.size} -> allowed {got.info()[1]} (model {int(want.sum())})")
            check(got, want)
            rebuilt = ix.make_filter(nbits, labels=np.flatnonzero(want).astype(np.uint64))
            assert np.array_equal(got.read(), rebuilt.read()) and got.info() == rebuilt.info()
            assert not got.read((nbits + 63) // 64 + 3)[(nbits + 63) // 64:].any()
            check(base, model)                                        # the base is untouched
    # no base: from the empty set; empty lists; None lists; a recycled block that held all ones starts clean
    for nbits in (0, 1, 64, 65, 100_000):
        ones = ix.make_filter(nbits, base_bits=np.full((nbits + 63) // 64 + 1, ~np.uint64(0)))
        ones.release()
        st = rng.integers(0, nbits + 10, size=500, dtype=np.uint64)
        check(ix.filter_apply_delta(None, nbits, set=st, clear=st[:100]), apply_model(np.zeros(0, bool), nbits, st, st[:100]))
        check(ix.filter_apply_delta(None, nbits), np.zeros(nbits, bool))
        check(ix.filter_apply_delta(None, nbits, set=np.zeros(0, np.uint64), clear=st), np.zeros(nbits, bool))
    # every bit cleared, every bit set
    base, model = random_base(ix, rng, 70_001)
    every = np.arange(70_001, dtype=np.uint64)
    check(ix.filter_apply_delta(base, 70_001, clear=every), np.zeros(70_001, bool))
    check(ix.filter_apply_delta(base, 70_001, set=every), np.ones(70_001, bool))
    check(ix.filter_apply_delta(base, 70_001, set=every, clear=every), np.ones(70_001, bool))


def test_the_base_is_immutable_and_may_leave_first(vsa, oracle):
    rng = np.random.default_rng(702)
    n, dim, k = 5000, 24, 8
    x = rng.standard_normal((n, dim)).astype(np.float32)
    g = vsa.Index("FLAT", dim, "L2", initial_cap=n)
    g.add_batch(x)
    g.flush()
    allowed = np.flatnonzero(rng.random(n) < 0.3).astype(np.uint64)
    model = np.zeros(n, bool)
    model[allowed.astype(np.int64)] = True
    base = g.make_filter(n, labels=allowed)
    q = rng.standard_normal(dim).astype(np.float32)
    want_d, want_l = g.search(q, k, allow=words_of(model), allow_nbits=n)
    # a search submitted with the base waits in the dispatcher for company while the base is derived from and released
    g.set_coalescing(64, 300_000)
    try:
        done = threading.Semaphore(0)
        pend = g.submit_filter(q, k, lambda st: done.release(), base)
        other = np.setdiff1d(np.arange(n, dtype=np.uint64), allowed)
        derived = g.filter_apply_delta(base, n + 77, set=other, clear=allowed)     # the complement, and longer
        base.release()                                                             # before the result is first used
        want = np.zeros(n + 77, bool)
        want[other.astype(np.int64)] = True
        check(derived, want)
        assert done.acquire(timeout=60)
        d, l = pend.result()
        assert pend.status == 0 and l.tolist() == want_l.tolist() and d.view(np.uint32).tolist() == want_d.view(np.uint32).tolist()
    finally:
        g.set_coalescing(0, 0)
    d1, l1 = g.search_filter(q, k, derived)
    d2, l2 = g.search(q, k, allow=words_of(want), allow_nbits=n + 77)
    assert l1.tolist() == l2.tolist() and d1.view(np.uint32).tolist() == d2.view(np.uint32).tolist()
    assert not set(l1.tolist()) & set(allowed.tolist())


def test_a_batch_equals_its_single_calls_and_fails_as_a_whole(vsa, ix):
    rng = np.random.default_rng(703)
    b0, m0 = random_base(ix, rng, 100_003)
    b1, m1 = random_base(ix, rng, 64)
    items, models = [], []
    for base, model, nbits in ((b0, m0, 100_003), (b0, m0, 100_003 + 64), (None, np.zeros(0, bool), 777), (b1, m1, 5000),
                               (b0, m0, 250_000), (b1, m1, 64)) * 4:
        st, cl = random_delta(rng, model.size, nbits)
        items.append((base, nbits, st, cl))
        models.append(apply_model(model, nbits, st, cl))
    s0 = ix.stats()
    batch = ix.filter_apply_delta_batch(items)
    assert ix.stats().filters_built - s0.filters_built == len(items)
    assert len(batch) == len(items)
    for it, f, want in zip(items, batch, models):
        check(f, want)
        one = ix.filter_apply_delta(*it[:2], set=it[2], clear=it[3])
        assert np.array_equal(one.read(), f.read()) and one.info() == f.info()
    check(b0, m0)
    check(b1, m1)
    assert ix.filter_apply_delta_batch([]) == []
    # ---- argument errors: VK_ERR_INVALID, every out[i] still NULL, nothing built
    L = vsa.lib()
    s0 = ix.stats()
    ids = np.arange(10, dtype=np.uint64)

    def call(tab, n, out):
        return L.vk_filter_apply_delta_batch(ix._h, tab, n, out)

    def item(base, nbits, st=None, n_set=None, cl=None, n_clear=None):
        return vsa.FilterDelta(None if base is None else base._h, nbits, vsa._ptr(cl), (0 if cl is None else cl.size) if n_clear is None else n_clear,
                               vsa._ptr(st), (0 if st is None else st.size) if n_set is None else n_set)

    out = (C.c_void_p * 3)()
    tab = (vsa.FilterDelta * 3)(item(b0, 100_003, ids), item(b0, 100_002, ids), item(None, 50, ids))   # one item below its base
    assert call(tab, 3, out) == vsa.VK_ERR_INVALID and [out[i] for i in range(3)] == [None] * 3
    tab = (vsa.FilterDelta * 3)(item(b0, 100_003, ids), item(None, 50, None, n_set=4), item(None, 50, ids))   # a NULL list with a length
    assert call(tab, 3, out) == vsa.VK_ERR_INVALID and [out[i] for i in range(3)] == [None] * 3
    tab = (vsa.FilterDelta * 3)(item(b0, 100_003, ids), item(None, 50, None, cl=None, n_clear=1), item(None, 50, ids))
    assert call(tab, 3, out) == vsa.VK_ERR_INVALID and [out[i] for i in range(3)] == [None] * 3
    other = vsa.Index("FLAT", 8, "L2", initial_cap=64)
    foreign = other.make_filter(100_003, labels=ids)
    tab = (vsa.FilterDelta * 3)(item(b0, 100_003, ids), item(None, 50, ids), item(foreign, 100_003, ids))  # a base of another index
    assert call(tab, 3, out) == vsa.VK_ERR_INVALID and [out[i] for i in range(3)] == [None] * 3
    assert b"another index" in L.vk_last_error()
    ok = (vsa.FilterDelta * 3)(item(b0, 100_003, ids), item(None, 50, ids), item(b1, 64, ids))
    assert call(None, 3, out) == vsa.VK_ERR_INVALID                                   # NULL items with n > 0
    assert call(ok, 3, None) == vsa.VK_ERR_INVALID                                    # out == NULL
    big = (vsa.FilterDelta * 65536)(*([item(None, 8)] * 65536))
    big_out = (C.c_void_p * 65536)()
    assert call(big, 65536, big_out) == vsa.VK_ERR_INVALID and not any(big_out)       # n > 65535
    one_out = C.c_void_p()
    assert L.vk_filter_apply_delta(ix._h, None, C.byref(one_out)) == vsa.VK_ERR_INVALID
    assert L.vk_filter_apply_delta(ix._h, ok, None) == vsa.VK_ERR_INVALID
    with pytest.raises(vsa.VkError) as e:
        ix.filter_apply_delta(b0, 100_002)
    assert e.value.code == vsa.VK_ERR_INVALID
    assert ix.stats().filters_built == s0.filters_built
    assert call(ok, 0, None) == vsa.VK_OK                                              # n == 0: nothing done
    assert call(ok, 3, out) == vsa.VK_OK and all(out[i] for i in range(3))            # ... and the good table works
    for i in range(3):
        L.vk_filter_release(out[i])


def test_a_chain_of_deltas_does_not_drift(vsa, ix):
    rng = np.random.default_rng(704)
    nbits = 300_007
    f, model = random_base(ix, rng, nbits)
    for step in range(50):
        grow = int(rng.choice([0, 0, 1, 64, 1000]))
        st, cl = random_delta(rng, nbits, nbits + grow)
        nxt = ix.filter_apply_delta(f, nbits + grow, set=st, clear=cl)
        f.release()                                                   # the lineage keeps one filter alive
        f, nbits = nxt, nbits + grow
        model = apply_model(model, nbits, st, cl)
        check(f, model)


def _same(a, b):
    assert a[1].tolist() == b[1].tolist() and a[0].view(np.uint32).tolist() == b[0].view(np.uint32).tolist()


@pytest.mark.parametrize("algo,shards", [("FLAT", 0), ("FLAT", 4), ("HNSW", 0), ("HNSW", 4)])
def test_searches_with_a_derived_filter(vsa, oracle, algo, shards):
    rng = np.random.default_rng(705 + shards)
    n, extra, dim, k, ef, M = 6000, 500, 32, 10, 96, 16
    x = rng.standard_normal((n + extra, dim)).astype(np.float32)
    kw = dict(m=M, ef_construction=100, build_threads=1) if algo == "HNSW" else {}
    if shards:
        kw["shard_devices"] = [0] * shards
    g = vsa.Index(algo, dim, "L2", initial_cap=n + extra, **kw)
    g.add_batch(x[:n])
    g.flush()
    model = rng.random(n) < 0.2                                       # `@tag:{x}` before the write phase
    base = g.make_filter(n, labels=np.flatnonzero(model).astype(np.uint64))
    # the write phase: rows added (some match the tag), rows removed, tags of existing rows changed
    for lab in range(n, n + extra):
        g.add(lab, x[lab])
    dead = rng.choice(n, 300, replace=False)
    for lab in dead:
        g.remove(int(lab))
    g.flush()
    alive = np.ones(n + extra, bool)
    alive[dead] = False
    now = rng.choice(n + extra, 400, replace=False)                   # start matching (new rows among them)
    gone = np.concatenate([rng.choice(n, 400, replace=False), dead])  # stop matching; a removed row matches nothing
    want = apply_model(model, n + extra, now.astype(np.uint64), gone.astype(np.uint64))
    want[dead] = False
    now = now[alive[now]]
    derived = g.filter_apply_delta(base, n + extra, set=now.astype(np.uint64), clear=gone.astype(np.uint64))
    check(derived, want)
    rebuilt = g.make_filter(n + extra, labels=np.flatnonzero(want).astype(np.uint64))
    bits = words_of(want)
    Q = rng.standard_normal((12, dim)).astype(np.float32)
    if algo == "HNSW":
        graphs = (oracle.HNSW.shards_from_product_index(g.save_raw, dim, "L2", M, ef_construction=100) if shards
                  else [oracle.HNSW.from_product_index(g.save_raw, dim, "L2", M, ef_construction=100)])
    ids = np.flatnonzero(want).astype(np.uint64)
    for q in Q:
        a = g.search_filter(q, k, derived, ef=ef)
        _same(a, g.search_filter(q, k, rebuilt, ef=ef))
        _same(a, g.search(q, k, ef=ef, allow=bits, allow_nbits=n + extra))
        if algo == "FLAT":   # (exact: the k best allowed live rows, by the oracle's pre-filter heap)
            od, ol = oracle.prefilter_topk("L2", q, x[ids.astype(np.int64)], ids, k)
            assert a[1].tolist() == ol.tolist() and a[0].view(np.uint32).tolist() == od.view(np.uint32).tolist()
        else:                # (every shard's own graph searched by the oracle with the model bitmap, merged by (distance, label))
            parts = [o.search(q, k, ef=ef, allow=bits, allow_nbits=n + extra) for o in graphs]
            merged = sorted((float(d), int(l)) for D, Lb in parts for d, l in zip(D, Lb))[:k]
            assert a[1].tolist() == [l for _, l in merged] and [float(v) for v in a[0]] == [d for d, _ in merged]
    D1, L1, N1 = g.search_batch_filter_handles(Q, k, [derived] * len(Q), ef=ef)
    D2, L2, N2 = g.search_batch_filter_handles(Q, k, [rebuilt] * len(Q), ef=ef)
    assert N1.tolist() == N2.tolist() and L1.tolist() == L2.tolist() and D1.view(np.uint32).tolist() == D2.view(np.uint32).tolist()


def test_the_adaptor_maintains_filters_over_write_phases(vsa, tmp_path):
    """include/vk_vector_adaptor.h MaintainFilter / NoteFilterChange / OnWritePhaseEnd, driven by
    tests/helpers/adaptor_filter_delta_check.cc through the mocked VectorBase: three maintained tags and one unmaintained,
    adds / tag changes / removals from several writer threads per phase.  The program checks, after every phase: a
    maintained key is a cache HIT under the new epoch, filters_built went up by exactly the number of keys that had
    changes, each bitmap equals the one built from the fetchers, the unmaintained key misses; and an evicted maintained
    key is rebuilt correctly.  It prints one line per check and `bad=0` at the end."""
    exe = tmp_path / "adaptor_filter_delta_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"), "-I", str(ROOT / "tests" / "helpers"),
                           str(ROOT / "tests" / "helpers" / "adaptor_filter_delta_check.cc"), "-o", str(exe),
                           "-L", str(vsa.LIB_PATH.parent), "-lvkindex", "-lpthread", f"-Wl,-rpath,{vsa.LIB_PATH.parent}"])
    for algo in ("flat", "hnsw"):
        out = subprocess.run([str(exe), algo], capture_output=True, text=True, timeout=300)
        print(out.stdout[-6000:])
        assert out.returncode == 0 and "bad=0" in out.stdout and "phases=5" in out.stdout, out.stdout[-4000:] + out.stderr[-4000:]
