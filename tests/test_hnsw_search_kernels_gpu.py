"""The HNSW search kernels (csrc/hnsw_search.hip, K5 + K6) on graphs, launch arguments and scratch memory the test chooses,
through tests/helpers/hnsw_search_probe.hip -- a small library that includes that translation unit, so the product's nine
entry points and its launcher run.  The cases, their graphs and the model that says what each reaches are in
tests/helpers/hnsw_search_cases.py (pinned on the CPU by tests/test_hnsw_search_model_cpu.py).

Reference of every case: oracle.HNSW.from_arrays(the same arrays).search(q, k, ef, allow, stats=True).  Every comparison is
exact: out_n, labels, distance BITS, the (+inf, kNoLabel) tail up to k, stats[0] / stats[1] = the oracle's evaluations / hops
summed over the queries the launch answered, stats[3] = their number, stats[2] = the model's count of dropped frontier
entries (0 wherever the frontier cannot overflow), totals = stats[0:2], redo_out = exactly the queries the model says outgrow
the frontier or the table (the rest of it still the fill pattern), the output rows of abandoned queries still the pattern after
the first launch and exact after the second, queue = the number of work items.  Every case runs from three fill patterns of
the scratch memory -- 0, 0xFFFFFFFF (the kernels' own "no id") and 0xEEEEEEEE -- with identical answers.

The LDS visited sets (modes 3 and 5) decide on chip which ids spill into the table in memory, and lanes race for slots, so the
model cannot count the spills.  Every case is built so that the verdict is certain all the same (lds_verdict, asserted on
the CPU too): NOT given up when the list lengths of the expanded nodes add up to at most 3/4 of the spill table (q_hbm + size
cannot pass it) or when no id of the visited set can fail to find room on chip (bucket occupancy restated in numpy); given up
when more ids are visited than the set and 3/4 of the table hold together."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.helpers import hnsw_search_cases as HC

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "helpers"
CSRC = ROOT / "valkey-search_amd" / "csrc"
LIB = HERE / "libhnswsearchprobe.so"
INF_BITS = 0x7F800000


@functools.lru_cache(maxsize=None)
def probe():
    src = HERE / "hnsw_search_probe.hip"
    newest = max(p.stat().st_mtime for p in (src, CSRC / "hnsw_search.hip", CSRC / "kernels.hpp", CSRC / "device_common.hpp"))
    if not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
                               "-shared", "-fPIC", "-I", str(CSRC), str(src), "-o", str(LIB)])
    lib = C.CDLL(str(LIB))
    lib.hs_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hs_probe.restype = C.c_int
    return lib


class Out:
    pass


def run(g, dev, Q, q_stride, first, second=None, pattern=0xEEEEEEEE, expect_rc=0):
    """one probe call; first / second: launch() dicts.  Returns one Out per launch."""
    keep = []

    def ptr(a):
        if a is None:
            return None
        keep.append(a)
        return a.ctypes.data

    def tab(entries):
        if entries is None:
            return None
        t = np.array([0 if e is None else ptr(e) for e in entries], np.uint64)
        return ptr(t)

    nq = Q.shape[0]
    qp = np.full((nq, q_stride), np.array([0x7FC00000], np.uint32).view(np.float32)[0], np.float32)
    qp[:, :16 * dev["chunks"]] = 0
    qp[:, :g.dim] = Q
    G = HC.HsGraph(rows=ptr(dev["rows"]), labels=ptr(g.labels), links0=ptr(g.l0), levels=ptr(g.levels), upper_slot=ptr(dev["upper_slot"]),
                   upper_pool=ptr(dev["upper_pool"]), queries=ptr(qp), row_stride=dev["row_stride"], chunks=dev["chunks"], l0_stride=g.l0.shape[1],
                   up_stride=g.M + 1, n_slots=dev["n_slots"], entry_point=g.entry_point, max_level=g.max_level, n_nodes=g.n, q_stride=q_stride,
                   nq=nq)
    Ls, outs = [], []
    for d in (first, second):
        if d is None:
            Ls.append(None)
            continue
        o = Out()
        o.dist = np.zeros((nq, d["k"]), np.float32)
        o.label = np.zeros((nq, d["k"]), np.uint64)
        o.n = np.zeros(nq, np.uint32)
        o.stats, o.totals, o.redo = np.zeros(5, np.uint64), np.zeros(2, np.uint64), np.zeros(nq + 1, np.uint32)
        L = HC.HsLaunch(pattern=pattern, out_dist=ptr(o.dist), out_label=ptr(o.label), out_n=ptr(o.n), stats=ptr(o.stats), totals=ptr(o.totals),
                        redo=ptr(o.redo))
        for key, v in d.items():
            if key in ("allow_tab", "mask_tab"):
                setattr(L, key, tab(v))
            elif key in ("allow_bits", "allow_nbits_tab", "live_bits", "mask_bits", "cancel_q"):
                setattr(L, key, ptr(v))
            else:
                setattr(L, key, int(v))
        o.L = L
        Ls.append(L)
        outs.append(o)
    rc = probe().hs_probe(C.addressof(G), C.addressof(Ls[0]), C.addressof(Ls[1]) if Ls[1] is not None else None)
    if rc >= 2:      # a launch that had to be cancelled, or a HIP error: nothing more is launched on this device
        pytest.exit("hnsw_search_probe: " + ("a launch did not end and had to be cancelled" if rc == 2 else
                                             f"HIP error seen at hnsw_search_probe.hip:{rc}"), returncode=3)
    assert rc == expect_rc, "the probe refused its arguments" if rc else "the probe accepted what it must refuse"
    return outs


@functools.lru_cache(maxsize=None)
def prepared(name):
    """everything of a case that does not depend on the fill pattern, computed once: device arrays, launch descriptions,
    the oracle's answers and the model's verdict per query"""
    c = HC.BY_NAME[name]
    g = c.graph()
    dev = g.device_arrays(c.bf16, c.row_stride)
    Q = c.queries(g)
    F = c.filters(g)
    a, b = c.launches(g)
    oks = [HC.allowed_nodes(g, *(f or (None, None))) for f in F]
    for d in (a, b):
        if d is None:
            continue
        if c.via == "live_bits":
            d["live_bits"] = HC.node_bitmap(~g.deleted)
        elif c.allow is None:
            pass
        elif c.via == "allow_bits":
            d["allow_bits"], d["allow_nbits"] = F[0]
        elif c.via == "mask_bits":
            d["mask_bits"] = HC.node_bitmap(oks[0])
        elif c.via == "allow_tab":
            d["allow_tab"] = [None if f is None else f[0] for f in F]
            d["allow_nbits_tab"] = np.array([0 if f is None else f[1] for f in F], np.uint64)
        elif c.via == "mask_tab":
            d["mask_tab"] = [None if f is None and not g.deleted.any() else HC.node_bitmap(ok) for f, ok in zip(F, oks)]
    if c.via in ("allow_bits", "mask_bits") and c.allow is not None:
        assert all(np.array_equal(f[0], F[0][0]) and f[1] == F[0][1] for f in F), "one filter for the whole batch"
    o = g.oracle()
    ref = []
    for q, f in zip(Q, F):
        d, l, ev, hp = o.search(q, c.k, ef=c.ef, allow=None if f is None else f[0], allow_nbits=None if f is None else f[1], stats=True)
        ref.append((d, l, ev, hp))
    models = c.first_models(g)
    if c.ref_from_model:      # (a frontier that drops entries searches differently from the reference: the model is the statement)
        ref = [(m["dist"], m["labels"], m["evals"], m["hops"]) for m in models]
    return c, g, dev, Q, a, b, ref, models


def check_rows(c, g, out, ref, which, pattern, kernel_ids=False):
    """the answered queries `which` against the oracle; every other row still the pattern"""
    pat_d = np.uint32(pattern)
    pat_l = np.uint64(pattern) << np.uint64(32) | np.uint64(pattern)
    id_of = {int(l): i for i, l in enumerate(g.labels)}
    for q in range(len(ref)):
        if q not in which:
            assert (out.dist[q].view(np.uint32) == pat_d).all() and (out.label[q] == pat_l).all() and out.n[q] == pat_d, (c.name, q)
            continue
        d, l, _, _ = ref[q]
        if kernel_ids:
            l = np.array([id_of[int(x)] for x in l], np.uint64)
        n = d.size
        assert out.n[q] == n, (c.name, q, out.n[q], n)
        assert out.label[q, :n].tolist() == l.tolist(), (c.name, q)
        assert out.dist[q, :n].view(np.uint32).tolist() == d.view(np.uint32).tolist(), (c.name, q)
        assert (out.dist[q, n:].view(np.uint32) == INF_BITS).all() and (out.label[q, n:] == np.uint64(HC.NO_LABEL)).all(), (c.name, q)


@pytest.mark.parametrize("name", [c.name for c in HC.CASES])
def test_case(name):
    c, g, dev, Q, a, b, ref, models = prepared(name)
    nq = c.nq
    lds_set = a["vis_hash_log2"] != 0 and a["vis_mode"] in (3, 5)
    results = []
    for pattern in HC.PATTERNS:
        outs = run(g, dev, Q, c.q_stride or 16 * dev["chunks"], a, b, pattern)
        o1 = outs[0]
        # which kernel ran
        kern, wpb = HC.kernel_of(a, nq)
        assert kern == c.kernel and o1.L.waves_per_block == wpb and o1.L.latency == int(nq <= 1024), (kern, wpb, o1.L.waves_per_block)
        assert o1.L.lds_bytes == HC.expected_lds_bytes(a, g, dev["chunks"], nq) <= 160 * 1024      # (tells the visited modes apart)
        if a["blocks"]:
            assert o1.L.blocks_used == a["blocks"]
        # who was given up
        n_redo = int(o1.redo[0]) if a["with_redo_out"] else 0
        if a["with_redo_out"]:
            given_up = set(o1.redo[1:1 + n_redo].tolist())
            assert len(given_up) == n_redo and (o1.redo[1 + n_redo:] == np.uint32(pattern)).all()
            if lds_set:     # (the model cannot say which ids spill; tests/helpers/hnsw_search_cases.py lds_verdict can say what follows)
                verdict = [HC.lds_verdict(a, g, m) for m in models]
                assert None not in verdict, (name, verdict)
                assert given_up == {q for q, v in enumerate(verdict) if v}, (name, sorted(given_up))
            else:
                assert given_up == {q for q, m in enumerate(models) if m["abandoned"]}, (name, sorted(given_up))
        else:
            given_up = set()
            assert (o1.redo == np.uint32(pattern)).all()
        answered = set(range(nq)) - given_up
        check_rows(c, g, o1, ref, answered, pattern, kernel_ids=bool(a["out_ids"]))
        assert int(o1.stats[0]) == sum(ref[q][2] for q in answered) and int(o1.stats[1]) == sum(ref[q][3] for q in answered), name
        assert int(o1.stats[3]) == len(answered) and int(o1.stats[4]) == 0
        assert int(o1.stats[2]) == sum(m["over"] for m in models)
        assert o1.totals.tolist() == o1.stats[:2].tolist()
        assert o1.L.queue == nq
        if b is not None:
            o2 = outs[1]
            check_rows(c, g, o2, ref, set(range(nq)), pattern)
            assert int(o2.stats[0]) == sum(r[2] for r in ref) and int(o2.stats[1]) == sum(r[3] for r in ref)
            assert int(o2.stats[3]) == nq and int(o2.stats[4]) == n_redo and int(o2.stats[2]) == int(o1.stats[2])
            assert o2.totals.tolist() == o2.stats[:2].tolist() and o2.L.queue == n_redo
            assert o2.redo.tolist() == o1.redo.tolist()
        last = outs[-1]
        results.append((last.dist.tobytes(), last.label.tobytes(), last.n.tobytes(), last.stats.tobytes()))
    assert results[0] == results[1] == results[2]


def test_everything_filtered_out_is_abandoned_and_then_answered_empty():
    c, g, dev, Q, a, b, ref, models = prepared("gpool2-second-L2")
    for pattern in HC.PATTERNS:
        o1, o2 = run(g, dev, Q, 16, a, b, pattern)
        assert int(o1.redo[0]) == c.nq and (o2.n == 0).all()
        assert (o2.dist.view(np.uint32) == INF_BITS).all() and (o2.label == np.uint64(HC.NO_LABEL)).all()


def test_ties_between_duplicate_rows_under_different_labels():
    """ef >= n and k = the number of reachable nodes: every reachable node ends in the list whatever the order ties are met in,
    so the (distance, label) output is still exact"""
    base = HC.random_digraph(200, 16, seed=14)
    g = base.copy()
    g.rows[100:] = g.rows[:100]                            # every row twice, under two labels
    q = HC.make_queries(3, 16, 5)
    reach = HC.model(base, q[0], 1, 200)["visited"]
    assert reach > 150
    dev = g.device_arrays()
    o = g.oracle()
    for kw in (dict(), dict(vis_hash_log2=12, vis_mode=3), dict(vis_hash_log2=12, vis_mode=2)):
        a = HC.launch(g, 256, reach, **kw)
        for pattern in HC.PATTERNS:
            out, = run(g, dev, q, 16, a, None, pattern)
            for i in range(3):
                d, l = o.search(q[i], reach, ef=256)
                assert out.n[i] == reach and d.size == reach
                assert out.label[i].tolist() == l.tolist() and out.dist[i].view(np.uint32).tolist() == d.view(np.uint32).tolist()


def test_cancel_raised_before_the_launch_and_per_query():
    c, g, dev, Q, a, b, ref, models = prepared("plain-L2-ef64")
    for pattern in HC.PATTERNS:
        out, = run(g, dev, Q, 16, dict(a, cancel=1), None, pattern)
        assert (out.n == 0).all() and (out.dist.view(np.uint32) == INF_BITS).all() and (out.label == np.uint64(HC.NO_LABEL)).all()
        assert out.stats.tolist() == [0, 0, 0, 0, 0] and out.L.queue == c.nq
        cq = np.array([1, 0, 0, 1, 0, 1], np.uint32)
        out, = run(g, dev, Q, 16, dict(a, cancel_q=cq), None, pattern)
        live = [q for q in range(c.nq) if not cq[q]]
        for q in range(c.nq):
            if cq[q]:
                assert out.n[q] == 0 and (out.dist[q].view(np.uint32) == INF_BITS).all() and (out.label[q] == np.uint64(HC.NO_LABEL)).all()
        for q in live:
            d, l, _, _ = ref[q]
            assert out.n[q] == d.size and out.label[q, :d.size].tolist() == l.tolist()
            assert out.dist[q, :d.size].view(np.uint32).tolist() == d.view(np.uint32).tolist()
        assert int(out.stats[3]) == len(live) and int(out.stats[0]) == sum(ref[q][2] for q in live)


def test_probe_refuses_what_the_kernels_trust():
    c, g, dev, Q, a, b, ref, models = prepared("plain-L2-ef64")
    refuse = lambda gg, dd, first, second=None, QQ=Q: run(gg, dd, QQ, 16 * dd["chunks"], first, second, expect_rc=1)
    bad = g.copy()
    bad.l0[5, 1] = g.n                                       # an id outside the graph
    refuse(bad, dev, a)
    bad = g.copy()
    bad.l0[5, 0] = bad.l0.shape[1]                           # a count past the row
    refuse(bad, dev, a)
    bad = g.copy()
    bad.entry_point = g.n
    refuse(bad, dev, a)
    bad = g.copy()
    lvl0 = int(np.nonzero(g.levels == 0)[0][0])
    key = (g.entry_point, g.max_level)
    bad.upper[key] = np.append(bad.upper[key][:-1], np.uint32(lvl0))     # a node named at a level it has no list for
    refuse(bad, bad.device_arrays(), a)
    refuse(g, dev, dict(a, k=0))
    refuse(g, dev, dict(a, k=65))                                        # k > ef
    refuse(g, dev, dict(a, e=2))                                         # not hnsw_slots_per_lane(ef)
    refuse(g, dev, dict(a, cand_cap=64))                                 # an LDS frontier below 2 * ef, nothing selective
    refuse(g, dev, dict(a, nbr_cap=0))
    refuse(g, dev, dict(a, vis_hash_log2=12))                            # a hash set without redo_out
    refuse(g, dev, dict(a, vis_hash_log2=4, vis_mode=2, with_redo_out=1))
    refuse(g, dev, dict(a, vis_hash_log2=12, with_redo_out=1, gpool_level=1, cand_cap=640))
    refuse(g, dev, dict(a, gpool_level=1, cand_cap=200))                 # not a multiple of 128
    refuse(g, dev, dict(a, gpool_level=1, cand_cap=128))                 # below n_nodes without redo_out
    refuse(g, dev, dict(a, gpool_level=2, cand_cap=4096))                # not a multiple of 8192
    refuse(g, dev, dict(a, gpool_level=1, cand_cap=128, with_redo_out=1), dict(a, vis_hash_log2=12, with_redo_out=1))   # hash + redo_in
    big = HC.oracle_built(150, 16 * 192, 8, "L2", 20 + 16 * 192)
    refuse(big, big.device_arrays(), HC.launch(big, 16000, 10), QQ=HC.make_queries(2, big.dim, 0))   # more than 160 KB of LDS
