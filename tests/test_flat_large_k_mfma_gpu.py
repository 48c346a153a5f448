"""Option flat-large-k-mfma through the C ABI: FLAT searches with k > 1024 under flat-large-k = 1 with a chunk's dense distances
from the vector kernel (option 0) and from the matrix cores (option 1, flat_dense_mfma_kernel in csrc/flat_large_k.hip).  No
tolerance: distances, labels and out_n are byte-identical under both and the CPU oracle's ranking; vk_flat_large_k_mfma_stats
says exactly which chunks ran where, and stands still under 0.  (Data and oracle helpers: tests/test_flat_large_k_gpu.py's.)"""
import ctypes as C
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
OPT, FIELDS = "flat-large-k-mfma", ("launches", "queries", "rows", "declined")
N, DIM, NQ, K = 3000, 100, 8, 1500
GONE = (0, 1234, N - 1)   # rows removed behind the bulk add: the first, one in the middle, the last
LIVE, RANKS = N - len(GONE), {}


def world(vsa, O, space, dtype="f32", **kw):
    """an index of LIVE rows under flat-large-k = 1, 8 queries, the oracle's ranking of every row per query, the live labels"""
    X, Q = G.make_data(O, N, DIM, NQ, space, 7)
    labels = np.arange(N, dtype=np.uint64) * np.uint64(3) + np.uint64(10)
    ix = vsa.Index("FLAT", DIM, space, initial_cap=N, device_id=0, dtype=dtype, **kw)
    ix.add_batch(X, labels)
    assert all(ix.remove(int(labels[g])) == 0 for g in GONE) and ix.get_option(OPT) == 0            # ships off
    keep = np.ones(N, bool)
    keep[list(GONE)] = False
    ix.set_option("flat-large-k", 1)
    if (space, dtype) not in RANKS:                                                     # (the reference: once per space and row format)
        RANKS[space, dtype] = G.ranking(O, X[keep], labels[keep], Q, space, dtype == "bf16")
    return ix, Q, RANKS[space, dtype], labels[keep]


def both(ix, search):
    """search() under option 0 and 1: equal bytes, no counter moves under 0; returns the answer and the movement under 1"""
    outs, moved = [], []
    for v in (0, 1):
        ix.set_option(OPT, v)
        s0 = ix.large_k_mfma_stats()
        outs.append([np.ascontiguousarray(x) for x in search()])
        s1 = ix.large_k_mfma_stats()
        moved.append({f: getattr(s1, f) - getattr(s0, f) for f in FIELDS})
    ix.set_option(OPT, 0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs)) and moved[0] == dict.fromkeys(FIELDS, 0)
    return (*outs[1], moved[1])


@pytest.mark.parametrize("dsort", (0, 1))
@pytest.mark.parametrize("space,dtype,bitmap", [("COSINE", "f32", True), ("COSINE", "bf16", False), ("IP", "f32", False), ("IP", "bf16", True)])
def test_both_options_give_the_oracles_bytes(env, space, dtype, bitmap, dsort):
    vsa, O = env
    ix, Q, ranks, labels = world(vsa, O, space, dtype)
    ix.set_option("flat-large-k-device-sort", dsort)
    allowed, kw = None, {}
    if bitmap:   # a host bitmap that ends below the largest label
        nbits = int(labels[-1]) - 90
        allowed = labels[(np.random.default_rng(3).random(LIVE) < 0.7) & (labels < nbits)]
        kw = dict(allow=O.allow_bitmap(allowed, nbits), allow_nbits=nbits)
    d, l, n, moved = both(ix, lambda: ix.search_batch(Q, K, **kw))
    G.check_oracle(d, l, n, ranks, K, allowed)
    assert moved == dict(launches=1, queries=NQ, rows=LIVE, declined=0)
    ix.close()


@pytest.mark.parametrize("why", ["L2", "three queries", "a short last chunk"])
def test_chunks_that_stay_on_the_vector_kernel(env, why):
    vsa, O = env
    ix, Q, ranks, labels = world(vsa, O, "L2" if why == "L2" else "COSINE")
    nq, taken = 3 if why == "three queries" else NQ, why == "a short last chunk"
    if taken:   # the budget pays for five queries: chunks of 5 and 3
        ix.set_option("flat-large-k-bytes", 5 * (((LIVE + 63) & ~63) * 4 + LK.cap_of(K) * 12) + 100)
    d, l, n, moved = both(ix, lambda: ix.search_batch(Q[:nq], K))
    G.check_oracle(d, l, n, ranks[:nq], K)
    assert moved == dict(launches=int(taken), queries=5 * taken, rows=LIVE * taken, declined=1)
    ix.close()


def test_two_logical_shards_and_a_bad_struct_size(env):
    vsa, O = env
    ix, Q, ranks, labels = world(vsa, O, "COSINE", shard_devices=[0, 0])
    ix.set_option(OPT, 1)
    assert ix.get_option(OPT) == 1                                                      # forwarded like the other large-k options
    d, l, n, moved = both(ix, lambda: ix.search_batch(Q, K))
    G.check_oracle(d, l, n, ranks, K)
    assert moved == dict(launches=2, queries=2 * NQ, rows=LIVE, declined=0)               # every shard launches for itself: the sums
    s = vsa.FlatLargeKMfmaStats()
    s.struct_size = C.sizeof(s) - 8
    assert vsa.lib().vk_index_large_k_mfma_stats(ix._h, C.byref(s)) == vsa.VK_ERR_INVALID
    ix.close()
