"""Option prefilter-shared-mfma through the C ABI: pre-filter batches with a shared list's distances from K8m against the same
calls on K8b.  No tolerance: under 0 and 1 the outputs are byte for byte the same and the CPU oracle's heap over the known keys
in list order; vk_prefilter_mfma_stats says exactly what ran, and stands still under 0."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
OPT, FIELDS = "prefilter-shared-mfma", ("launches", "queries", "entries", "declined")
N, DIM, NQ, K = 3000, 100, 37, 10


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


class World:
    """an index, its rows as stored by label, 40 queries, and a shared list: 1400 labels, 60 unknown, one removed, two repeated"""

    def __init__(self, vsa, oracle, kind, metric, dtype, n, dim):
        rng = np.random.default_rng([len(kind), len(metric), len(dtype), dim])
        kw = dict(m=8, ef_construction=40) if "HNSW" in kind else {}
        if kind.startswith("SHARDED"):
            kw["shard_devices"] = [0, 0, 0, 0]
        self.oracle, self.metric = oracle, metric
        self.g = vsa.Index("HNSW" if "HNSW" in kind else "FLAT", dim, metric, initial_cap=n, dtype=dtype, **kw)
        unit = lambda m: np.stack([oracle.normalize(v)[0] for v in rng.standard_normal((m, dim)).astype(np.float32)])
        x, labels = unit(n), np.arange(n, dtype=np.uint64) * 3 + 10
        self.g.add_batch(x, labels)
        if dtype == "bf16":   # round to nearest even, as the index stores them
            u = x.view(np.uint32).astype(np.uint64)
            x = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
        self.live, self.Q = dict(zip(labels.tolist(), x)), unit(40)
        keys = rng.choice(labels, size=min(1338, n // 2), replace=False)
        assert self.g.remove(int(keys[7])) == 0
        del self.live[int(keys[7])]
        self.keys = np.concatenate([keys, np.arange(10 ** 9, 10 ** 9 + 60, dtype=np.uint64), keys[:2]]).astype(np.uint64)
        self.known = sum(int(l) in self.live for l in self.keys.tolist())

    def both(self, call, Q, keys_of):
        """the call under option 0 and 1: equal bytes, the oracle's answer, no counter moves under 0; returns the movement under 1"""
        outs, moved = [], []
        for v in (0, 1):
            self.g.set_option(OPT, v)
            s0 = self.g.prefilter_mfma_stats()
            outs.append(call())
            s1 = self.g.prefilter_mfma_stats()
            moved.append({f: getattr(s1, f) - getattr(s0, f) for f in FIELDS})
        self.g.set_option(OPT, 0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs)) and moved[0] == dict.fromkeys(FIELDS, 0)
        D, L, Nn = outs[1]
        for q in range(Q.shape[0]):
            lab = [l for l in keys_of(q).tolist() if l in self.live]
            od, ol = self.oracle.prefilter_topk(self.metric, Q[q], np.stack([self.live[l] for l in lab]), np.array(lab, np.uint64), K)
            n = int(Nn[q])
            assert L[q, :n].tolist() == ol.tolist() and D[q, :n].view(np.uint32).tolist() == od.view(np.uint32).tolist(), q
        return moved[1]


def world(vsa, oracle, kind, metric, dtype, n=N, dim=DIM):
    return _world(vsa, oracle, kind, metric, dtype, n, dim)   # (one index per kind for the whole module)


@lru_cache(maxsize=None)
def _world(*args):
    return World(*args)


@pytest.mark.parametrize("kind,metric,dtype,n,dim,resolve,shards",
                         [(k, m, d, N, DIM, 0, 1) for k in ("FLAT", "HNSW") for m in ("COSINE", "IP") for d in ("f32", "bf16")] +
                         [("FLAT", "COSINE", "f32", 600, 768, 0, 1),
                          ("HNSW", "COSINE", "f32", N, DIM, 1, 1),             # prefilter_device_stage_keys drives the launch
                          ("SHARDED FLAT", "COSINE", "f32", N, DIM, 0, 4)])    # each of the four shards holds keys of the list
def test_both_options_give_the_oracles_bytes(vsa, oracle, kind, metric, dtype, n, dim, resolve, shards):
    w = world(vsa, oracle, kind, metric, dtype, n, dim)
    w.g.set_option("prefilter-device-resolve", resolve)
    r0 = w.g.prefilter_stats().device_resolved_keys
    moved = w.both(lambda: w.g.search_labels_batch(w.Q[:NQ], K, w.keys), w.Q[:NQ], lambda q: w.keys)
    assert (w.g.prefilter_stats().device_resolved_keys > r0) == bool(resolve)
    w.g.set_option("prefilter-device-resolve", 0)
    assert moved == dict(launches=shards, queries=shards * NQ, entries=w.known, declined=0)


@pytest.mark.parametrize("why", ["four queries", "L2", "per-query lists"])
def test_launches_that_stay_on_k8b(vsa, oracle, why):
    w = world(vsa, oracle, "FLAT", "L2" if why == "L2" else "COSINE", "f32")
    nq = 4 if why == "four queries" else NQ
    lb = np.arange(nq + 1, dtype=np.uint64) * 30 if why == "per-query lists" else None
    keys = w.keys[:nq * 30] if lb is not None else w.keys
    moved = w.both(lambda: w.g.search_labels_batch(w.Q[:nq], K, keys, lb), w.Q[:nq], lambda q: keys if lb is None else keys[30 * q:30 * q + 30])
    assert moved == dict(launches=0, queries=0, entries=0, declined=0 if lb is not None else 1)


def test_the_handle_path_launches_once_per_run(vsa, oracle):
    w = world(vsa, oracle, "FLAT", "COSINE", "f32")
    known = np.array(sorted(w.live), np.uint64)
    fa, fb = w.g.make_filter(3 * N + 100, labels=known[:900]), w.g.make_filter(3 * N + 100, labels=known[500:2100])
    moved = w.both(lambda: w.g.search_filter_exact_batch(w.Q, K, [fa] * 20 + [fb] * 20), w.Q, lambda q: known[:900] if q < 20 else known[500:2100])
    assert moved == dict(launches=2, queries=40, entries=900 + 1600, declined=0)


def test_a_bad_struct_size_is_refused(vsa, oracle):
    s = vsa.PrefilterMfmaStats()
    s.struct_size = C.sizeof(s) - 8
    assert vsa.lib().vk_index_prefilter_mfma_stats(world(vsa, oracle, "FLAT", "COSINE", "f32").g._h, C.byref(s)) == vsa.VK_ERR_INVALID
