"""Option flat-large-k-device-sort through the C ABI: FLAT searches with k > 1024 under flat-large-k = 1 with the hand-back
ordered by the host (option 0) and by the device's merge sort (option 1, csrc/flat_large_k.hip) -- distances, labels and out_n
byte-identical to each other, to the paged path and to the CPU oracle's ranking.  The counters of vk_index_large_k_sort_stats:
sorted_queries grows with one_pass_queries exactly while the option is on, downloaded_entries by k per such query, merge_passes
by the header's function of cap per chunk.  (Data and oracle helpers: tests/test_flat_large_k_gpu.py's.)"""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "tests" / "helpers"):
    sys.path.insert(0, str(p))
import flat_large_k_cases as LK  # noqa: E402
import test_flat_large_k_gpu as G  # noqa: E402

env = G.env
N, NQ = 5000, 9
SORT_FIELDS = ("sorted_queries", "merge_passes", "downloaded_entries")


def passes(cap):
    return ((cap + 4095) // 4096 - 1).bit_length()           # large_k_sort_passes of flat_large_k_host.hpp


def sorted_chunks(nq, count, k, budget):
    """large_k_plan_sorted: a query costs its row of distances, two lists of cap slots and k dense slots"""
    ld = (count + 63) & ~63
    c = min(max(1, budget // (ld * 4 + (2 * LK.cap_of(k) + k) * 12)), nq, 65535)
    c = c & ~7 if c >= 8 else c
    return (nq + c - 1) // c


def counters(ix):
    a, b = ix.large_k_stats(), ix.large_k_sort_stats()
    return {**{f: getattr(a, f) for f in G.FIELDS}, **{f: getattr(b, f) for f in SORT_FIELDS}}


def trio(ix, search, k, chunks=None):
    """search() on the paged path, then one-pass with the host's sort, then with the device's: the same bytes.  The sort's
    counters stand still while its option is off and follow the one-pass path's while it is on; returns the answer and that growth."""
    outs, grew = [], []
    for large_k, dsort in ((0, 1), (1, 0), (1, 1)):
        ix.set_option("flat-large-k", large_k)
        ix.set_option("flat-large-k-device-sort", dsort)
        c0 = counters(ix)
        outs.append([np.ascontiguousarray(x) for x in search()])
        c1 = counters(ix)
        grew.append({f: c1[f] - c0[f] for f in c0})
    ix.set_option("flat-large-k", 0)
    ix.set_option("flat-large-k-device-sort", 0)
    for d, l, n in outs[1:]:
        assert n.tolist() == outs[0][2].tolist() and np.array_equal(l, outs[0][1]) and np.array_equal(d.view(np.uint32), outs[0][0].view(np.uint32))
    assert all(grew[i][f] == 0 for i in (0, 1) for f in SORT_FIELDS)
    g = grew[2]
    assert g["sorted_queries"] == g["one_pass_queries"] and g["downloaded_entries"] == g["sorted_queries"] * k
    assert g["merge_passes"] == g["chunks"] * passes(LK.cap_of(k)) and (chunks is None or g["chunks"] == chunks)
    assert g["fallback_queries"] == grew[1]["fallback_queries"] and g["emitted_entries"] == grew[1]["emitted_entries"]
    return (*outs[2], g)


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
@pytest.mark.parametrize("space", ("L2", "IP", "COSINE"))
def test_device_sort_agrees_with_host_sort_and_oracle(env, space, dtype):
    vsa, O = env
    X, Q = G.make_data(O, N, 64, NQ, space, 1)
    labels = np.arange(N, dtype=np.uint64)
    ranks = G.ranking(O, X, labels, Q, space, dtype == "bf16")
    ix = vsa.Index("FLAT", 64, space, initial_cap=N, device_id=0, dtype=dtype)
    ix.add_batch(X, labels)
    assert ix.get_option("flat-large-k-device-sort") == 0                               # ships off
    for k in (1025, 2500, 5000):                                                        # cap 2049 (one tile), 3524, 6250 (one pass)
        for nq in (1, NQ):
            d, l, n, g = trio(ix, lambda: ix.search_batch(Q[:nq], k), k, sorted_chunks(nq, N, k, 1 << 30))
            G.check_oracle(d, l, n, ranks[:nq], k)
            assert g["sorted_queries"] == nq
    ix.close()


def test_bitmap_nan_query_and_byte_budgets(env):
    vsa, O = env
    X, Q = G.make_data(O, N, 100, NQ, "L2", 2)
    rng = np.random.default_rng(22)
    labels = rng.permutation(3 * N)[:N].astype(np.uint64) + np.uint64(7)
    ix = vsa.Index("FLAT", 100, "L2", initial_cap=N, device_id=0)
    ix.add_batch(X, labels)
    ranks = G.ranking(O, X, labels, Q, "L2")
    nbits = 3 * N - 93
    allowed = labels[(rng.random(N) < 0.6) & (labels < nbits)]
    bits = O.allow_bitmap(allowed, nbits)
    for k in (1025, 2500, 5000):                                                        # 5000: fewer admitted rows than k
        d, l, n, g = trio(ix, lambda: ix.search_batch(Q, k, allow=bits, allow_nbits=nbits), k)
        G.check_oracle(d, l, n, ranks, k, allowed)
    Qn = Q[:3].copy()
    Qn[1, 5] = np.nan                                                                   # no candidate at all: n = 0 on the device
    d, l, n, g = trio(ix, lambda: ix.search_batch(Qn, 2500), 2500)
    assert n.tolist() == [2500, 0, 2500] and g["sorted_queries"] == 3
    G.check_oracle(d[[0, 2]], l[[0, 2]], n[[0, 2]], [ranks[0], ranks[2]], 2500)
    # budgets: five queries per chunk with the host's sort are two with the device's buffers counted; and one that pays for one
    # query's distances and list but not for the sort's buffers still runs, a query per chunk
    k, ld = 2500, (N + 63) & ~63
    for budget in (5 * (ld * 4 + LK.cap_of(k) * 12) + 100, ld * 4 + LK.cap_of(k) * 12 + 100):
        ix.set_option("flat-large-k-bytes", budget)
        want = sorted_chunks(NQ, N, k, budget)
        assert want == (5 if budget > 200000 else 9) and LK.plan(NQ, N, k, budget)[3] in (2, 9)
        d, l, n, g = trio(ix, lambda: ix.search_batch(Q, k), k, want)
        G.check_oracle(d, l, n, ranks, k)
    ix.close()


def test_ties_are_ordered_by_label_and_flagged_queries_fall_back(env):
    vsa, O = env
    X, Q = G.make_data(O, 1700, 16, NQ, "L2", 4)
    X3 = np.concatenate([X, X, X])
    labels = np.random.default_rng(4).permutation(len(X3)).astype(np.uint64)
    ix = vsa.Index("FLAT", 16, "L2", initial_cap=len(X3), device_id=0)
    ix.add_batch(X3, labels)
    ranks = G.ranking(O, X3, labels, Q, "L2")
    for k in (1025, 2500, len(X3)):
        d, l, n, g = trio(ix, lambda: ix.search_batch(Q, k), k)
        G.check_oracle(d, l, n, ranks, k)
        assert g["sorted_queries"] == NQ
    ix.close()
    one = np.repeat(X[:1], 6000, axis=0)                      # 6 000 copies of one row: every place ties, the label alone orders
    labels = np.random.default_rng(5).permutation(6000).astype(np.uint64) + np.uint64(100)
    ix = vsa.Index("FLAT", 16, "L2", initial_cap=6000, device_id=0)
    ix.add_batch(one, labels)
    ranks = G.ranking(O, one, labels, Q[:5], "L2")
    for k in (1025, 2500, 5000, 6000):
        d, l, n, g = trio(ix, lambda: ix.search_batch(Q[:5], k), k)
        G.check_oracle(d, l, n, ranks, k)
        want = G.expected_fallbacks(ranks, k)
        assert want == (5 if LK.cap_of(k) < 6000 else 0) and g["fallback_queries"] == want and g["sorted_queries"] == 5 - want
    ix.close()


def test_four_logical_shards(env):
    vsa, O = env
    X, Q = G.make_data(O, 2 * N, 64, NQ, "IP", 3)
    labels = np.arange(2 * N, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    ix = vsa.Index("FLAT", 64, "IP", initial_cap=2 * N, device_id=0, shard_devices=[0, 0, 0, 0])
    ix.add_batch(X, labels)
    ranks = G.ranking(O, X, labels, Q, "IP")
    ix.set_option("flat-large-k-device-sort", 1)
    assert ix.get_option("flat-large-k-device-sort") == 1                               # forwarded like the other options
    d, l, n, g = trio(ix, lambda: ix.search_batch(Q, 2000), 2000)                        # every shard (2 500 rows) sorts its own 2 000
    G.check_oracle(d, l, n, ranks, 2000)
    assert g["sorted_queries"] == 4 * NQ and g["chunks"] == 8
    ix.close()
