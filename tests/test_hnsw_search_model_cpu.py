"""The CPU side of tests/test_hnsw_search_kernels_gpu.py: oracle.HNSW.from_arrays, the heapq model of
tests/helpers/hnsw_search_cases.py and the case list itself.

  * from_arrays(export_graph(o)) answers exactly like o: labels, distance bits, evaluations, hops.
  * The model is pinned to the oracle -- answers, evaluations, hops -- on every graph maker, with and without a filter.
  * Rows and queries of every case: all n distances of a query are distinct (the oracle's own distances), so no answer
    depends on how ties are broken.
  * Every case reaches the path it is there for; a case that stops reaching it fails here, without a GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import hnsw_search_cases as HC


def same(a, b):
    return a.tolist() == b.tolist()


def test_from_arrays_answers_like_the_graph_it_was_exported_from():
    rows = HC.make_rows(500, 24, 77)
    for space in ("L2", "IP"):
        o = O.HNSW(24, space, max_elements=500, M=6, ef_construction=50)
        o.add_many(rows, labels=np.arange(500, dtype=np.uint64) * np.uint64(7))
        for lab in (7, 70, 700):
            o.mark_delete(lab)
        g = o.export_graph()
        l0 = g["l0"].copy()
        l0[:, 0] |= g["deleted"].astype(np.uint32) << 16
        c = O.HNSW.from_arrays(g["rows"], g["labels"], l0, g["upper"], g["max_level"], g["entry_point"], space, 6)
        assert c.count == o.count and c.deleted_count == 3 and c.max_level == o.max_level and c.entry_point == o.entry_point
        allow = O.allow_bitmap(np.arange(0, 3500, 14), 3500)
        for q in HC.make_queries(5, 24, 1):
            for ef, al in ((10, None), (80, None), (40, allow)):
                d0, l0_, e0, h0 = o.search(q, 10, ef=ef, allow=al, allow_nbits=3500 if al is not None else None, stats=True)
                d1, l1, e1, h1 = c.search(q, 10, ef=ef, allow=al, allow_nbits=3500 if al is not None else None, stats=True)
                assert same(l0_, l1) and same(d0.view(np.uint32), d1.view(np.uint32)) and (e0, h0) == (e1, h1)


MAKERS = {
    "oracle_built": lambda: HC.oracle_built(600, 16, 8, "L2", 4),
    "oracle_built-IP": lambda: HC.oracle_built(600, 16, 8, "IP", 4),
    "random_digraph-3": lambda: HC.random_digraph(400, 3),
    "random_digraph-16": lambda: HC.random_digraph(400, 16),
    "random_digraph-64": lambda: HC.random_digraph(400, 64),
    "random_digraph-96": lambda: HC.random_digraph(400, 96, "IP"),
    "with_repeats-16": lambda: HC._repeats(16),
    "with_repeats-64": lambda: HC._repeats(64),
    "with_tombstones": lambda: HC.with_tombstones(HC.oracle_built(600, 16, 8, "L2", 4), 0.3),
    "with_tombstones-digraph": lambda: HC.with_tombstones(HC.random_digraph(400, 16), 0.2),
}


@pytest.mark.parametrize("maker", sorted(MAKERS))
def test_model_is_the_oracle(maker):
    g = MAKERS[maker]()
    o = g.oracle()
    flt = HC._third(g, 1)
    for q in HC.make_queries(4, g.dim, 3):
        for k, ef, f in ((1, 1, None), (10, 30, None), (10, 30, flt), (g.n, g.n, None), (5, 100, flt)):
            m = HC.model(g, q, k, ef, HC.allowed_nodes(g, *(f or (None, None))))
            d, l, ev, hp = o.search(q, k, ef=ef, allow=None if f is None else f[0], allow_nbits=None if f is None else f[1], stats=True)
            assert same(l, m["labels"]) and same(d.view(np.uint32), m["dist"].view(np.uint32)), (maker, k, ef)
            assert (ev, hp) == (m["evals"], m["hops"]), (maker, k, ef)
            # the kernels' lazily pruned frontier decides like the unbounded one as long as nothing is dropped
            mc = HC.model(g, q, k, ef, HC.allowed_nodes(g, *(f or (None, None))), cap=max(2 * ef, 64) if f is None and not g.deleted.any() else g.n)
            assert mc["over"] == 0 and same(mc["labels"], m["labels"]) and (mc["evals"], mc["hops"]) == (m["evals"], m["hops"])


def test_graph_makers_have_the_lists_they_promise():
    for M in (3, 16, 64, 96):
        g = HC.random_digraph(400, M)
        cnt = g.l0[:, 0] & 0xFFFF
        assert cnt.min() == 0 and cnt.max() == 2 * M and g.l0.shape[1] == 2 * M + 1 and g.max_level == 3
        if M >= 64:
            assert max(v.size for v in g.upper.values()) > 16          # two rounds of sixteen in the descent
    t = HC.with_tombstones(HC.oracle_built(600, 16, 8, "L2", 4), 0.3)
    assert t.deleted[t.entry_point] and 100 < t.deleted.sum() < 300


@pytest.mark.parametrize("name", [c.name for c in HC.CASES])
def test_case_reaches_its_path(name):
    c = HC.BY_NAME[name]
    g = c.graph()
    a, b = c.launches(g)
    assert HC.kernel_of(a, c.nq)[0] == c.kernel
    Q = c.queries(g)
    for q in Q:      # no two nodes equidistant from a query
        assert np.unique(g.distances(q).view(np.uint32)).size == g.n
    text, reaches = c.path
    models = c.first_models(g)
    assert reaches(models), text
    if a["vis_hash_log2"] and a["vis_mode"] in (3, 5):      # which queries the spill table gives up is certain, either way
        assert None not in [HC.lds_verdict(a, g, m) for m in models]
    if not c.ref_from_model:
        assert sum(m["over"] for m in models) == 0
