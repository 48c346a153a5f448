"""FLAT search with k > 1024 through the C ABI: option flat-large-k = 1 (one dense distance pass per chunk of queries, a device
select, a host finish -- csrc/flat_large_k.hip) against option 0 (the paged path: one scan per 1024 results) and against the
CPU oracle.  Distances, labels and out_n must be byte-identical between the two options and equal the oracle's ranking.

5 000 rows of D 64.  The case of 300 rows of D 2 500 clamps k to the count (300 <= 1024), so it pins that such a request never
reaches either large-k path; 1 300 rows of the same width are what drives the wide-row distance kernel (four queries per block).

Tie-free Gaussian data: fallback_queries == 0 and one_pass_queries == queries are CONDITIONS (the oracle's distances for these
seeds are checked on the CPU to have no tie at any k-th place).  Tie data: the number of fallbacks is exactly what the oracle's
distances give for the hand-back's slack."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests" / "helpers"))
import flat_large_k_cases as LK  # noqa: E402

N, DIM, NQ = 5000, 64, 33
KS = (1025, 2500, 5000, 6000)
NQS = (1, 9, 33)
FIELDS = ("queries", "one_pass_queries", "fallback_queries", "chunks", "emitted_entries", "row_passes")


@pytest.fixture(scope="module")
def env():
    import _pkg
    from oracle import oracle as O
    return _pkg.vsa, O


def bf16_round(x):
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def make_data(O, n, dim, nq, space, seed, bf16=False):
    rng = np.random.default_rng([n, dim, seed])
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    if space == "COSINE":
        X = np.stack([O.normalize(v)[0] for v in X])
        Q = np.stack([O.normalize(v)[0] for v in Q])
    return X, Q


def ranking(O, X, labels, Q, space, bf16=False):
    """per query the oracle's (distance bits, label) of every row in (distance, label) order"""
    rows = bf16_round(np.ascontiguousarray(X)) if bf16 else X
    o = O.Flat(X.shape[1], space, max_elements=len(X))
    o.add_many(rows, np.asarray(labels, np.uint64))
    out = []
    for q in Q:
        od, ol = o.search(q, len(X))
        assert ol.size == len(X)
        out.append((od.view(np.uint32).copy(), ol.copy()))
    return out


def expect(rank, k, allowed=None):
    bits, lab = rank
    if allowed is not None:
        keep = np.isin(lab, allowed)
        bits, lab = bits[keep], lab[keep]
    return bits[:k], lab[:k]


def stats(ix):
    s = ix.large_k_stats()
    return {f: getattr(s, f) for f in FIELDS}


def delta(a, b):
    return {f: b[f] - a[f] for f in FIELDS}


def both(ix, search):
    """search() under option 0, then 1: byte-identical outputs; returns them and the counters' growth under option 1"""
    ix.set_option("flat-large-k", 0)
    d0, l0, n0 = search()
    ix.set_option("flat-large-k", 1)
    s0 = stats(ix)
    d1, l1, n1 = search()
    s1 = stats(ix)
    ix.set_option("flat-large-k", 0)
    assert n0.tolist() == n1.tolist()
    assert np.array_equal(np.ascontiguousarray(d0).view(np.uint32), np.ascontiguousarray(d1).view(np.uint32)) and np.array_equal(l0, l1)
    return d1, l1, n1, delta(s0, s1)


def check_oracle(d, l, n, ranks, k, allowed=None):
    for q in range(len(n)):
        wb, wl = expect(ranks[q], k, allowed)
        assert n[q] == len(wb), (q, n[q], len(wb))
        assert np.array_equal(l[q, :n[q]], wl) and np.array_equal(np.ascontiguousarray(d[q, :n[q]]).view(np.uint32), wb), q


def no_tie_at(ranks, places):
    for bits, lab in ranks:
        key = LK.key_of(bits)
        for k in places:
            if 0 < k < len(key):
                assert key[k - 1] != key[k]


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
@pytest.mark.parametrize("space", ("L2", "IP", "COSINE"))
def test_options_agree_and_equal_the_oracle(env, space, dtype):
    vsa, O = env
    X, Q = make_data(O, N, DIM, NQ, space, 1)
    labels = np.arange(N, dtype=np.uint64)
    ranks = ranking(O, X, labels, Q, space, dtype == "bf16")
    no_tie_at(ranks, KS)                                   # (on the CPU: the condition below is about the code, not the seed)
    ix = vsa.Index("FLAT", DIM, space, initial_cap=N, device_id=0, dtype=dtype)
    ix.add_batch(X, labels)
    assert ix.get_option("flat-large-k") == 0 and ix.get_option("flat-large-k-bytes") == 1 << 30      # ships off
    for k in KS:
        for nq in NQS:
            d, l, n, grew = both(ix, lambda: ix.search_batch(Q[:nq], k))
            check_oracle(d, l, n, ranks[:nq], k)
            fits, ld, chunk_q, chunks = LK.plan(nq, N, min(k, N), 1 << 30)
            assert grew["queries"] == nq and grew["one_pass_queries"] == nq and grew["fallback_queries"] == 0
            assert grew["chunks"] == chunks and grew["row_passes"] == chunks
            assert grew["emitted_entries"] == nq * min(k, N)
    before = stats(ix)
    ix.search_batch(Q[:4], 1024)                            # k <= 1024 is none of this path's business
    assert stats(ix) == before
    ix.close()


def test_bitmap_filter_handle_nan_query_and_label_churn(env):
    vsa, O = env
    X, Q = make_data(O, N, DIM, 9, "L2", 2)
    rng = np.random.default_rng(22)
    labels = rng.permutation(3 * N)[:N].astype(np.uint64) + np.uint64(7)            # labels permuted, with gaps
    ix = vsa.Index("FLAT", DIM, "L2", initial_cap=N, device_id=0)
    ix.add_batch(X, labels)
    ranks = ranking(O, X, labels, Q, "L2")
    nbits = 3 * N + 7 - 100                                                          # some labels lie at or beyond nbits
    allowed = labels[(rng.random(N) < 0.6) & (labels < nbits)]
    bits = O.allow_bitmap(allowed, nbits)
    for k in (1025, 2500, 5000):
        d, l, n, grew = both(ix, lambda: ix.search_batch(Q, k, allow=bits, allow_nbits=nbits))
        check_oracle(d, l, n, ranks, k, allowed)
        assert grew["fallback_queries"] == 0 and grew["one_pass_queries"] == 9
    f = ix.make_filter(nbits, labels=allowed)
    d, l, n, grew = both(ix, lambda: ix.search_batch_filter_handles(Q, 2500, [f] * 9))
    check_oracle(d, l, n, ranks, 2500, allowed)
    assert grew["one_pass_queries"] == 9
    f.release()
    # a NaN query: every distance is a NaN, K3 lists none of them and neither does the select -- the same (empty) answer
    Qn = Q[:3].copy()
    Qn[1, 5] = np.nan
    d, l, n, grew = both(ix, lambda: ix.search_batch(Qn, 2500))
    assert n.tolist() == [2500, 0, 2500] and grew["one_pass_queries"] == 3
    check_oracle(d[[0, 2]], l[[0, 2]], n[[0, 2]], [ranks[0], ranks[2]], 2500)
    # rows removed and re-added between calls (the last row moves into the hole; re-added rows take new slots)
    gone = rng.permutation(N)[:700]
    for i in gone:
        ix.remove(int(labels[i]))
    keep = np.setdiff1d(np.arange(N), gone)
    d, l, n, grew = both(ix, lambda: ix.search_batch(Q, 3000))
    check_oracle(d, l, n, ranking(O, X[keep], labels[keep], Q, "L2"), 3000)
    back = gone[:400]
    ix.add_batch(X[back], labels[back])
    now = np.concatenate([keep, back])
    d, l, n, grew = both(ix, lambda: ix.search_batch(Q, 4700))
    check_oracle(d, l, n, ranking(O, X[now], labels[now], Q, "L2"), 4700)
    assert grew["fallback_queries"] == 0 and grew["one_pass_queries"] == 9
    ix.close()


def test_four_logical_shards(env):
    vsa, O = env
    X, Q = make_data(O, N, DIM, 9, "IP", 3)
    labels = np.arange(N, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    ix = vsa.Index("FLAT", DIM, "IP", initial_cap=N, device_id=0, shard_devices=[0, 0, 0, 0])
    ix.add_batch(X, labels)
    ranks = ranking(O, X, labels, Q, "IP")
    ix.set_option("flat-large-k-bytes", 1 << 29)
    assert ix.get_option("flat-large-k-bytes") == 1 << 29                 # forwarded like the other options
    for k in (2500, 6000):
        d, l, n, grew = both(ix, lambda: ix.search_batch(Q, k))
        check_oracle(d, l, n, ranks, k)
        # every shard serves its own large-k search: the sums of four shards (each holds more than 1024 rows)
        assert grew["queries"] == 4 * 9 and grew["one_pass_queries"] == 4 * 9 and grew["fallback_queries"] == 0
        assert grew["chunks"] == 4 * LK.plan(9, N // 4, N // 4, 1 << 29)[3] == 8
    ix.close()


def expected_fallbacks(ranks, k):
    """queries whose tie group at the k-th place does not fit the hand-back, by the oracle's distances"""
    out = 0
    for bits, lab in ranks:
        key = LK.key_of(bits)
        T = key[min(k, len(key)) - 1]
        out += int((key <= T).sum() > LK.cap_of(k))
    return out


def test_ties_every_row_three_times_and_one_row_six_thousand_times(env):
    vsa, O = env
    X, Q = make_data(O, 1700, DIM, 9, "L2", 4)
    X3 = np.concatenate([X, X, X])
    labels = np.random.default_rng(4).permutation(len(X3)).astype(np.uint64)
    ix = vsa.Index("FLAT", DIM, "L2", initial_cap=len(X3), device_id=0)
    ix.add_batch(X3, labels)
    ranks = ranking(O, X3, labels, Q, "L2")
    for k in (1025, 2500, len(X3)):
        d, l, n, grew = both(ix, lambda: ix.search_batch(Q, k))
        check_oracle(d, l, n, ranks, k)
        want = expected_fallbacks(ranks, k)
        assert want == 0 and grew["fallback_queries"] == want and grew["one_pass_queries"] == 9 - want
    ix.close()
    # 6 000 copies of one row: every query ties 6 000 ways at every k-th place -- beyond the slack unless cap reaches the count
    one = np.repeat(X[:1], 6000, axis=0)
    labels = np.random.default_rng(5).permutation(6000).astype(np.uint64) + np.uint64(100)
    ix = vsa.Index("FLAT", DIM, "L2", initial_cap=6000, device_id=0)
    ix.add_batch(one, labels)
    ranks = ranking(O, one, labels, Q[:5], "L2")
    for k in (1025, 2500, 5000, 6000):
        d, l, n, grew = both(ix, lambda: ix.search_batch(Q[:5], k))
        check_oracle(d, l, n, ranks, k)
        want = expected_fallbacks(ranks, k)
        assert want == (5 if LK.cap_of(k) < 6000 else 0)
        assert grew["fallback_queries"] == want and grew["one_pass_queries"] == 5 - want and grew["chunks"] == 1
    ix.close()


def test_byte_budget_fallback_and_two_chunks(env):
    vsa, O = env
    X, Q = make_data(O, N, DIM, 9, "L2", 6)
    labels = np.arange(N, dtype=np.uint64)
    ix = vsa.Index("FLAT", DIM, "L2", initial_cap=N, device_id=0)
    ix.add_batch(X, labels)
    ranks = ranking(O, X, labels, Q, "L2")
    k = 2500
    fits, ld, chunk_q, chunks = LK.plan(9, N, k, 1 << 30)
    assert fits and chunks == 2                                            # 8 + 1: a chunk is a multiple of 8 once it reaches 8
    ix.set_option("flat-large-k-bytes", ld * 4 - 1)                        # below one query's row of distances
    d, l, n, grew = both(ix, lambda: ix.search_batch(Q, k))
    check_oracle(d, l, n, ranks, k)
    assert grew["fallback_queries"] == 9 and grew["one_pass_queries"] == 0 and grew["chunks"] == 0 and grew["emitted_entries"] == 0
    assert grew["row_passes"] == 3                                         # the paged path: three passes of at most 1024 results
    budget = 5 * (ld * 4 + LK.cap_of(k) * 12) + 100                        # five queries per chunk
    assert LK.plan(9, N, k, budget) == (True, ld, 5, 2)
    ix.set_option("flat-large-k-bytes", budget)
    d, l, n, grew = both(ix, lambda: ix.search_batch(Q, k))
    check_oracle(d, l, n, ranks, k)
    assert grew["chunks"] == 2 and grew["row_passes"] == 2 and grew["one_pass_queries"] == 9 and grew["fallback_queries"] == 0
    ix.close()


def test_wide_rows(env):
    vsa, O = env
    dim = 2500
    X, Q = make_data(O, 1300, dim, 9, "L2", 7)
    labels = np.arange(1300, dtype=np.uint64)
    # 300 rows: k clamps to the count, below the paged path's threshold -- neither large-k path is involved
    ix = vsa.Index("FLAT", dim, "L2", initial_cap=300, device_id=0)
    ix.add_batch(X[:300], labels[:300])
    d, l, n, grew = both(ix, lambda: ix.search_batch(Q, 2500))
    check_oracle(d, l, n, ranking(O, X[:300], labels[:300], Q, "L2"), 300)
    assert grew["queries"] == 0
    ix.close()
    ix = vsa.Index("FLAT", dim, "L2", initial_cap=1300, device_id=0)
    ix.add_batch(X, labels)
    ranks = ranking(O, X, labels, Q, "L2")
    for k in (1100, 2500):
        d, l, n, grew = both(ix, lambda: ix.search_batch(Q, k))
        check_oracle(d, l, n, ranks, k)
        assert grew["one_pass_queries"] == 9 and grew["fallback_queries"] == 0
    ix.close()
