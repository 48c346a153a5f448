"""Every launcher of the device HNSW build (csrc/hnsw_build.hip, K9) on its own, and the chain select -> group -> relink ->
gather once from fixed candidate lists, through tests/helpers/hnsw_build_probe.hip -- a small library that includes that
translation unit, so the product's kernels run.  No beam search and no host threads: the inputs are the test's, the
reference is a few lines of numpy per step, and every comparison is exact -- ids, counts, float BITS, and the whole links0
table (the models write exactly the words the kernels may write, so a word that must stay as it was is compared too).

Distances are oracle.distance(metric, a, b) on the f32 values of the rows (bf16 rows widened by << 16); the product's
distance is pinned bit for bit to it elsewhere.  The "lattice" data class has small-integer rows, so every dot product and
squared distance is exact in f32: there the model also runs in float64 and must decide identically before anything is
launched -- a high-precision reference in which exact ties occur (duplicate rows, equidistant candidates).

    select(cands, M)   n = min(cand_n, cand_ld); n < M: keep all in order; otherwise walk the candidates in the given order,
                       keep c unless some kept r has dist(r, c) < d(c), stop at M  (hnswalg.h getNeighborsByHeuristic2)
    group              pairs (sel_id[p][t], sel_dist[p][t], first + p), t < sel_n[p], stable-sorted by (node, order key of the
                       distance).  The key is the sort's own: sign bit set -> all bits inverted, else the sign bit set.  -0
                       sorts before +0; a NaN with the sign bit clear sorts after +inf, one with the sign bit set before -inf.
                       Entries past counts / off[T] / pairs are unspecified and not compared.
    relink(maxM0)      cnt + nadd <= maxM0: append in order.  Otherwise the old list with dist(e, s) plus the first
                       min(nadd, 256 - cnt) additions with their given distances, ordered by (relink key, id, position)
                       (csrc/hnsw_relink_order.hpp: -0 = +0, every NaN last), then the heuristic with cap maxM0.
                       Ties go to the SMALLER id, where hnswlib's heap pops the larger one first: this is the kernel's
                       documented order, not the reference's.
    gather / widen     plain indexing; 0xEEEEEEEE (the probe's fill) where nothing may be written.

Shapes: dimensions 13 / 144 / 768 = row strides of 1, 9 (one batch of 8 + a tail) and 48 chunks; f32 and bf16; IP and L2;
random, lattice and clustered rows.  The group launcher takes its pair count n_new * m from {2, 63, 127, 128, 129, 1023,
1024, 1025, 8191, 300000}: the odd counts are no multiple of m in {2, 16, 96}, so m also takes 1, 3, 25 and 31 there."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "helpers"
CSRC = ROOT / "valkey-search_amd" / "csrc"
LIB = HERE / "libhnswbuildprobe.so"

EE = 0xEEEEEEEE
KCAP = 256                                    # hnsw_relink_kernel: candidates per node
DIMS = [13, 144, 768]
CONFIGS = [(dim, dt, metric, cls) for dim in DIMS for dt in ("f32", "bf16") for metric in ("IP", "L2")
           for cls in ("random", "lattice", "clustered")]


def build_probe():
    src = HERE / "hnsw_build_probe.hip"
    newest = max(p.stat().st_mtime for p in (src, CSRC / "hnsw_build.hip", CSRC / "hnsw_relink_order.hpp", CSRC / "kernels.hpp",
                                             CSRC / "device_common.hpp"))
    if not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", "-I", str(CSRC), str(src),
                               "-o", str(LIB)])
    return LIB


def ptr(a):
    return a.ctypes.data


class Probe:
    def __init__(self):
        lib = C.CDLL(str(build_probe()))
        vp, u32, i = C.c_void_p, C.c_uint32, C.c_int
        lib.hb_probe_select.argtypes = [vp, u32, u32, i, i, vp, u32, u32, vp, vp, vp, u32, u32, u32, vp, vp, vp]
        lib.hb_probe_group.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp]
        lib.hb_probe_relink.argtypes = [vp, u32, u32, i, i, vp, u32, u32, vp, vp, vp, vp, u32, u32]
        lib.hb_probe_gather.argtypes = [vp, u32, u32, u32, u32, vp, u32, u32, vp]
        lib.hb_probe_widen.argtypes = [vp, u32, u32, u32, u32, u32, vp]
        lib.hb_probe_chain.argtypes = [vp, u32, u32, i, i, vp, u32, u32, u32, vp, vp, vp, u32, u32, u32, vp, vp, vp]
        for f in ("select", "group", "relink", "gather", "widen", "chain"):
            getattr(lib, "hb_probe_" + f).restype = C.c_int
        self.lib = lib

    @staticmethod
    def ok(rc, what):
        assert rc == 0, f"{what}: HIP error seen at hnsw_build_probe.hip:{rc}" if rc > 1 else f"{what} refused its arguments"

    def select(self, R, links, M, cid, cd, cn, first, expect_rc=0):
        n_new, ld = cid.shape
        links = links.copy()
        sid = np.zeros((n_new, M), np.uint32)
        sd = np.zeros((n_new, M), np.float32)
        sn = np.zeros(n_new, np.uint32)
        rc = self.lib.hb_probe_select(ptr(R.dev), R.n, R.stride, R.bf16, R.l2, ptr(links), links.shape[1], M, ptr(cid), ptr(cd), ptr(cn), ld,
                                      n_new, first, ptr(sid), ptr(sd), ptr(sn))
        if expect_rc:
            assert rc == expect_rc
            return None
        self.ok(rc, "hb_probe_select")
        return links, sid, sd, sn

    def group(self, sid, sd, sn, first):
        n_new, m = sid.shape
        n = n_new * m
        counts, node, off = np.zeros(2, np.uint32), np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32)
        add_p, add_d = np.zeros(n, np.uint32), np.zeros(n, np.float32)
        self.ok(self.lib.hb_probe_group(ptr(sid), ptr(sd), ptr(sn), n_new, m, first, ptr(counts), ptr(node), ptr(off), ptr(add_p), ptr(add_d)),
                "hb_probe_group")
        return counts, node, off, add_p, add_d

    def relink(self, R, links, maxM0, node, off, add_p, add_d, bound, expect_rc=0):
        links = links.copy()
        rc = self.lib.hb_probe_relink(ptr(R.dev), R.n, R.stride, R.bf16, R.l2, ptr(links), links.shape[1], maxM0, ptr(node), ptr(off),
                                      ptr(add_p), ptr(add_d), node.size, bound)
        if expect_rc:
            assert rc == expect_rc
            return None
        self.ok(rc, "hb_probe_relink")
        return links

    def gather(self, links, first, n_new, node, touched):
        dst = np.zeros((n_new + node.size, links.shape[1]), np.uint32)
        self.ok(self.lib.hb_probe_gather(ptr(links), links.shape[0], links.shape[1], first, n_new, ptr(node), node.size, touched, ptr(dst)),
                "hb_probe_gather")
        return dst

    def widen(self, rows16, first, n, pad):
        out = np.zeros((n + pad, rows16.shape[1]), np.uint32)
        self.ok(self.lib.hb_probe_widen(ptr(rows16), rows16.shape[0], rows16.shape[1], first, n, pad, ptr(out)), "hb_probe_widen")
        return out

    def chain(self, R, links, M, maxM0, cid, cd, cn, first):
        n_new, ld = cid.shape
        links = links.copy()
        counts, node = np.zeros(2, np.uint32), np.zeros(n_new * M, np.uint32)
        lists = np.zeros((n_new + n_new * M, links.shape[1]), np.uint32)
        self.ok(self.lib.hb_probe_chain(ptr(R.dev), R.n, R.stride, R.bf16, R.l2, ptr(links), links.shape[1], M, maxM0, ptr(cid), ptr(cd),
                                        ptr(cn), ld, n_new, first, ptr(counts), ptr(node), ptr(lists)), "hb_probe_chain")
        return links, counts, node, lists


@pytest.fixture(scope="module")
def probe():
    return Probe()


# ---- rows and distances --------------------------------------------------------------------------------------------------
class Rows:
    """a row table: .f = the f32 values the kernels see, .dev = what is uploaded (zero padded to the stride); R(i, j) = the
    oracle's distance of rows i and j (both metrics are symmetric in their arguments, bit for bit), computed once"""

    def __init__(self, oracle, vals, dt, metric):
        vals = np.ascontiguousarray(vals, np.float32)
        self.n, self.dim = vals.shape
        self.stride = (self.dim + 15) // 16 * 16
        self.bf16, self.l2, self.metric = int(dt == "bf16"), int(metric == "L2"), metric
        if self.bf16:
            u16 = (vals.view(np.uint32) >> 16).astype(np.uint16)
            self.f = np.ascontiguousarray((u16.astype(np.uint32) << 16).view(np.float32))
            self.dev = np.zeros((self.n, self.stride), np.uint16)
            self.dev[:, :self.dim] = u16
        else:
            self.f = vals
            self.dev = np.zeros((self.n, self.stride), np.float32)
            self.dev[:, :self.dim] = vals
        self.oracle = oracle
        self._fn, self._space, self._isa = oracle.LIB.vko_distance, oracle.SPACE[metric], oracle.ISA["skylake"]
        self._p = [C.cast(self.f.ctypes.data + r * self.dim * 4, oracle._f32p) for r in range(self.n)]
        self.cache = {}
        # the direct call below is oracle.distance without its per-call conversions
        for i, j in ((0, self.n - 1), (self.n // 2, 1)):
            assert np.float32(self(i, j)).view(np.uint32) == oracle.distance(metric, self.f[i], self.f[j]).view(np.uint32) or np.isnan(self(i, j))

    def __call__(self, i, j):
        key = (i, j) if i <= j else (j, i)
        v = self.cache.get(key)
        if v is None:
            v = self.cache[key] = np.float32(self._fn(self._space, self._isa, self._p[key[0]], self._p[key[1]], self.dim))
        return v


class Exact64:
    """the same distances in float64, for lattice rows (exact there)"""

    def __init__(self, R):
        self.R, self.f = R, R.f.astype(np.float64)
        self.cache = {}

    def __call__(self, i, j):
        key = (i, j) if i <= j else (j, i)
        v = self.cache.get(key)
        if v is None:
            a, b = self.f[key[0]], self.f[key[1]]
            v = self.cache[key] = float(((a - b) ** 2).sum()) if self.R.l2 else 1.0 - float(a @ b)
        return v

    def agrees(self):
        for (i, j), v in self.cache.items():
            assert float(self.R(i, j)) == v, (i, j, v)          # the f32 distance IS the exact one


def make_values(cls, n, dim, rng):
    if cls == "random":
        return rng.standard_normal((n, dim)).astype(np.float32)
    if cls == "lattice":                                        # |x| <= 3: 768 * 36 < 2^24, every sum exact; rows repeat
        v = rng.integers(-3, 4, (n, dim)).astype(np.float32)
        v[:, 2:] *= (rng.random((n, dim - 2)) < 8.0 / dim)      # few non-zero coordinates: many equidistant pairs
        dup = rng.choice(n, n // 8, replace=False)
        v[dup] = v[rng.choice(n, n // 8)]
        return v
    centres = rng.standard_normal((5, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    return (centres[rng.integers(0, 5, n)] + 0.1 / np.sqrt(dim) * rng.standard_normal((n, dim))).astype(np.float32)


def seed_of(*parts):
    return [p if isinstance(p, int) else sum(ord(c) << (8 * k) for k, c in enumerate(str(p)[:4])) for p in parts]


def random_links(rng, n_rows, l0s, max_cnt, ids_below):
    """dirty rows (no word is zero by accident), counts 0..max_cnt, flag bits in the high half of word 0 on some rows"""
    links = rng.integers(1, 1 << 32, (n_rows, l0s), dtype=np.uint64).astype(np.uint32)
    for r in range(n_rows):
        cnt = int(rng.integers(0, max_cnt + 1))
        flags = (0, 0x00010000, 0xA5A50000, 0xFFFF0000)[int(rng.integers(0, 4))]
        links[r, 0] = flags | cnt
        links[r, 1:1 + cnt] = rng.choice(ids_below, cnt, replace=False)
    return links


# ---- the models ------------------------------------------------------------------------------------------------------------
def heuristic(D, cands, cap, stats=None):
    """cands: (id, distance to the base) in walking order"""
    kept = []
    for c, dq in cands:
        if len(kept) == cap:
            break
        bad = any(D(r, c) < dq for r in kept)
        if stats is not None and kept:
            stats[0] += 1
            stats[1] += bad
        if not bad:
            kept.append(c)
    return kept


def select_model(D, links, M, cid, cd, cn, first, stats=None):
    """-> links after the launch, sel_id / sel_n, and per point the indices of the kept candidates"""
    links = links.copy()
    n_new, ld = cid.shape
    sel, picks = [], []
    for p in range(n_new):
        n = min(int(cn[p]), ld)
        ids = [int(x) for x in cid[p, :n]]
        if n < M:
            kept = ids
        else:
            kept = heuristic(D, list(zip(ids, cd[p, :n])), M, stats)
        row = links[first + p]
        row[1:1 + len(kept)] = kept
        row[0] = (row[0] & np.uint32(0xFFFF0000)) | np.uint32(len(kept))
        sel.append(kept)
        picks.append([ids.index(k) for k in kept] if len(set(ids)) == len(ids) else None)
    return links, sel, picks


def sort_key(d):
    u = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def relink_key(d):
    u = np.ascontiguousarray(d, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    k = np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[(u & 0x7FFFFFFF) > 0x7F800000] = 0xFFFFFFFF
    return k


def group_model(sid, sd, sn, first):
    """-> counts, node [T], off [T + 1], add_p [pairs], add_d bits [pairs]"""
    n_new, m = sid.shape
    valid = (np.arange(m)[None, :] < sn[:, None]).ravel()
    node = sid.ravel()[valid].astype(np.uint64)
    d = sd.ravel()[valid]
    p = (np.uint32(first) + np.repeat(np.arange(n_new, dtype=np.uint32), m))[valid]
    order = np.argsort((node << np.uint64(32)) | sort_key(d).astype(np.uint64), kind="stable")
    node = node[order].astype(np.uint32)
    heads = np.flatnonzero(np.r_[True, node[1:] != node[:-1]]) if node.size else np.zeros(0, np.int64)
    off = np.r_[heads, node.size].astype(np.uint32)
    return np.array([heads.size, node.size], np.uint32), node[heads], off, p[order], d[order].view(np.uint32)


def relink_model(D, links, maxM0, node, off, add_p, add_d, stats=None):
    """-> links after the launch, and per touched node the set of ids it may hold afterwards"""
    links = links.copy()
    allowed = []
    for t, s in enumerate(int(x) for x in node):
        row = links[s]
        w0 = int(row[0])
        cnt = w0 & 0xFFFF
        adds = [int(x) for x in add_p[off[t]:off[t + 1]]]
        ad = add_d[off[t]:off[t + 1]]
        old = [int(x) for x in row[1:1 + cnt]]
        if cnt + len(adds) <= maxM0:
            new = old + adds
            row[1 + cnt:1 + len(new)] = adds
        else:
            nadd = min(len(adds), KCAP - cnt)
            ids = old + adds[:nadd]
            d = np.array([D(e, s) for e in old] + list(ad[:nadd]), np.float32)
            order = sorted(range(len(ids)), key=lambda i, k=relink_key(d): (int(k[i]), ids[i], i))
            new = heuristic(D, [(ids[i], d[i]) for i in order], maxM0, stats)
            row[1:1 + len(new)] = new
        row[0] = (w0 & 0xFFFF0000) | len(new)
        allowed.append(set(old) | set(adds))
    return links, allowed


def same_table(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (what, "rows", bad[:8].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


# ---- select ----------------------------------------------------------------------------------------------------------------
SEL_EXIST, SEL_NEW = 560, 37
SEL_MS = [2, 16, 17, 33, 96]


def select_inputs(R, rng, M, ld, n_new, first, D=None):
    """candidates of each new point: distinct existing nodes, ascending by (distance, id), cand_n through its edge values"""
    D = D or R
    cn_cycle = [0, 1, M - 1, M, M + 1, ld, ld + 7]
    cid = np.full((n_new, ld), 0xEEEEEEEEEEEEEEEE, np.uint64)      # beyond min(cand_n, ld): never read
    cd = np.full((n_new, ld), np.nan, np.float32)
    cn = np.zeros(n_new, np.uint32)
    for p in range(n_new):
        cn[p] = cn_cycle[(p + M) % len(cn_cycle)] if n_new > 1 else ld
        n = min(int(cn[p]), ld)
        pool = rng.choice(first, n, replace=False) if n < 64 else np.arange(first)     # long lists: the true nearest
        dd = [(float(D(first + p, int(c))), int(c)) for c in pool]
        dd.sort()
        cid[p, :n] = [c for _, c in dd[:n]]
        cd[p, :n] = [d for d, _ in dd[:n]]
    return cid, cd, cn


@pytest.mark.parametrize("dim,dt,metric,cls", CONFIGS)
def test_select(probe, oracle, dim, dt, metric, cls):
    rng = np.random.default_rng(seed_of(1, dim, dt, metric, cls))
    R = Rows(oracle, make_values(cls, SEL_EXIST + SEL_NEW, dim, rng), dt, metric)
    first = SEL_EXIST
    stats, filled = [0, 0], 0
    for M in SEL_MS:
        l0s = M + 3
        for ld, n_new in ((M, 4), (100, SEL_NEW), (512, 5), (M, 1)):
            links = random_links(rng, R.n, l0s, M, first)
            cid, cd, cn = select_inputs(R, rng, M, ld, n_new, first)
            want_links, sel, picks = select_model(R, links, M, cid, cd, cn, first, stats)
            if cls == "lattice":                             # float64 decides the same, before anything is launched
                D64 = Exact64(R)
                cd64 = np.array([[D64(first + p, int(c)) if t < min(cn[p], ld) else 0.0 for t, c in enumerate(cid[p])] for p in range(n_new)])
                _, sel64, _ = select_model(D64, links, M, cid, cd64, cn, first)
                assert sel64 == sel
                D64.agrees()
            filled += sum(len(s) == M and min(int(cn[p]), ld) > M for p, s in enumerate(sel))
            got_links, sid, sd, sn = probe.select(R, links, M, cid, cd, cn, first)
            what = (dim, dt, metric, cls, M, ld, n_new)
            assert sn.tolist() == [len(s) for s in sel], what
            for p, kept in enumerate(sel):
                assert sid[p, :len(kept)].tolist() == kept, (what, p)
                assert (sid[p, len(kept):] == EE).all() and (sd[p, len(kept):].view(np.uint32) == EE).all(), (what, p)
                if picks[p] is not None:
                    assert sd[p, :len(kept)].view(np.uint32).tolist() == cd[p, picks[p]].view(np.uint32).tolist(), (what, p)
            same_table(got_links, want_links, what)          # the new rows, flag bits kept; every other row untouched
    if cls == "clustered":
        assert stats[1] * 4 >= stats[0] > 0, stats          # the heuristic rejects at least a quarter of what it looks at
    if cls == "random":
        assert filled > 0                                    # some points fill M from a longer list


def test_select_refuses_what_the_kernel_trusts(probe, oracle):
    rng = np.random.default_rng(5)
    R = Rows(oracle, make_values("random", 40, 13, rng), "f32", "L2")
    links = random_links(rng, R.n, 20, 4, 30)
    cid, cd, cn = select_inputs(R, rng, 4, 8, 3, 30)
    bad = cid.copy()
    bad[1, 2] = R.n
    probe.select(R, links, 4, bad, cd, cn, 30, expect_rc=1)                       # id >= n_rows
    probe.select(R, links, 4, cid, cd, cn, 38, expect_rc=1)                       # first + n_new beyond the table
    probe.select(R, np.ascontiguousarray(links[:, :4]), 4, cid, cd, cn, 30, expect_rc=1)   # M + 1 > l0_stride
    wide = np.zeros((3, 193), np.uint64)
    probe.select(R, random_links(rng, R.n, 200, 4, 30), 193, wide, wide.astype(np.float32), cn, 30, expect_rc=1)   # max_keep > 192
    R.stride = 24
    probe.select(R, links, 4, cid, cd, cn, 30, expect_rc=1)                       # stride no multiple of 16


# ---- group -----------------------------------------------------------------------------------------------------------------
GROUP_SHAPES = [(1, 2), (21, 3), (127, 1), (8, 16), (43, 3), (33, 31), (64, 16), (512, 2), (41, 25), (8191, 1), (16, 96), (3125, 96)]


def group_inputs(n_new, m, rng, all_empty=False):
    n = n_new * m
    pool = rng.integers(0, 0xFFFFFFFF, max(1, n // 6), dtype=np.uint64).astype(np.uint32)     # all four bytes; 0xFFFFFFFF itself is
    pool[:min(4, pool.size)] = [0, 0xFF, 0xFFFFFFFE, 0x01000000][:min(4, pool.size)]       # left out: with an all-ones key = the invalid mark
    sid = rng.choice(pool, (n_new, m))
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x3F800000, 0xBF800000,
                        0x00000001, 0x80000001], np.uint32).view(np.float32)
    sd = rng.standard_normal((n_new, m)).astype(np.float32)
    runs = rng.random((n_new, m))
    sd[runs < 0.35] = rng.choice(special, int((runs < 0.35).sum()))           # equal (node, distance) across different p: stability
    sd[(runs >= 0.35) & (runs < 0.5)] = np.float32(-2.5)
    sn = rng.choice(np.array([0, m, m, max(0, m - 1), m // 2], np.uint32), n_new).astype(np.uint32)
    if all_empty:
        sn[:] = 0
    sid[np.arange(m)[None, :] >= sn[:, None]] = EE                                # what select leaves there
    return np.ascontiguousarray(sid, np.uint32), sd, sn


def check_group(probe, sid, sd, sn, first, what):
    counts, node, off, add_p, add_d = probe.group(sid, sd, sn, first)
    w_counts, w_node, w_off, w_p, w_bits = group_model(sid, sd, sn, first)
    assert counts.tolist() == w_counts.tolist(), what
    T, pairs = int(w_counts[0]), int(w_counts[1])
    if pairs == 0:
        assert off[0] == 0, what
        return
    assert np.array_equal(node[:T], w_node), what
    assert np.array_equal(off[:T + 1], w_off), what
    assert np.array_equal(add_p[:pairs], w_p), what
    assert np.array_equal(add_d[:pairs].view(np.uint32), w_bits), what


@pytest.mark.parametrize("n_new,m", GROUP_SHAPES)
def test_group(probe, n_new, m):
    rng = np.random.default_rng([2, n_new, m])
    sid, sd, sn = group_inputs(n_new, m, rng)
    if n_new > 1:
        sn[0], sn[-1] = m, 0                              # a full list first, an empty one last
    assert sn.max() == m and (n_new == 1 or (sn.min() == 0 and sn.sum() < n_new * m))
    if n_new * m > 256 * 1024:
        assert (n_new * m + 1023) // 1024 > 256          # the block sums of the scan: more than one per thread
    check_group(probe, sid, sd, sn, 0xFFFF0000 if n_new < 60000 else 7, (n_new, m))
    full = np.full(n_new, m, np.uint32)                   # every pair valid: the last pair is the last key
    check_group(probe, sid if (sid != EE).all() else np.where(sid == EE, np.uint32(3), sid), sd, full, 1, (n_new, m, "full"))


@pytest.mark.parametrize("n_new,m", [(1, 2), (64, 16), (41, 25)])
def test_group_with_nothing_selected(probe, n_new, m):
    sid, sd, sn = group_inputs(n_new, m, np.random.default_rng([3, n_new, m]), all_empty=True)
    counts, node, off, add_p, add_d = probe.group(sid, sd, sn, 5)
    assert counts.tolist() == [0, 0] and off[0] == 0


# ---- relink ----------------------------------------------------------------------------------------------------------------
RL_ROWS = 400


def relink_combos(maxM0):
    c = [(0, 1), (0, maxM0), (0, maxM0 + 1), (maxM0 - 1, 1), (maxM0 - 1, 2), (maxM0, 1), (maxM0, maxM0)]
    if maxM0 >= 32:
        c.append((32, 300))                               # truncated to 256 - 32 additions
    if maxM0 >= 192:
        c.append((192, 100))                              # truncated to 64
    return c


def relink_inputs(R, rng, maxM0, n_touched, D=None):
    """touched nodes cycling through the (cnt, nadd) combinations; additions ascending by (distance, id) as group leaves them"""
    D = D or R
    l0s = maxM0 + 2
    links = random_links(rng, R.n, l0s, maxM0, R.n)
    combos = relink_combos(maxM0)
    node = rng.choice(R.n, n_touched, replace=False).astype(np.uint32)
    off, add_p, add_d = [0], [], []
    for t, s in enumerate(int(x) for x in node):
        cnt, nadd = combos[(t + n_touched) % len(combos)]
        others = np.setdiff1d(np.arange(R.n), [s])
        pick = rng.choice(others, cnt + nadd, replace=False)
        links[s, 0] = (links[s, 0] & np.uint32(0xFFFF0000)) | np.uint32(cnt)
        links[s, 1:1 + cnt] = pick[:cnt]
        dd = sorted((float(D(int(p), s)), int(p)) for p in pick[cnt:])
        add_p += [p for _, p in dd]
        add_d += [d for d, _ in dd]
        off.append(len(add_p))
    off = np.array(off, np.uint32)
    full = (links[node, 0] & 0xFFFF) + np.diff(off) > maxM0
    for path in (full, ~full):                            # the tombstone bit on a node of either path, whatever the draw was
        if path.any():
            links[node[np.flatnonzero(path)[0]], 0] |= np.uint32(0x00010000)
    return links, node, np.array(off, np.uint32), np.array(add_p, np.uint32), np.array(add_d, np.float32)


@pytest.mark.parametrize("dim,dt,metric,cls", CONFIGS)
def test_relink(probe, oracle, dim, dt, metric, cls):
    rng = np.random.default_rng(seed_of(4, dim, dt, metric, cls))
    R = Rows(oracle, make_values(cls, RL_ROWS, dim, rng), dt, metric)
    stats = [0, 0]
    # (maxM0, touched nodes, 0 = the host knows the number | the bound the grid covers with device-side counts)
    for maxM0, n_touched, bound in ((4, 41, 0), (4, 5, 5 * 16), (4, 1, 0), (32, 41, 41 * 16), (32, 4, 0), (32, 1, 16), (192, 41, 0),
                                    (192, 5, 5 * 16)):
        links, node, off, add_p, add_d = relink_inputs(R, rng, maxM0, n_touched)
        want, _ = relink_model(R, links, maxM0, node, off, add_p, add_d, stats)
        if cls == "lattice":
            D64 = Exact64(R)
            ad64 = np.array([D64(int(p), int(node[np.searchsorted(off, i, side="right") - 1])) for i, p in enumerate(add_p)])
            assert np.array_equal(ad64.astype(np.float32), add_d) and np.array_equal(ad64, add_d.astype(np.float64))
            want64, _ = relink_model_f64(D64, links, maxM0, node, off, add_p, ad64)
            assert np.array_equal(want64, want)
            D64.agrees()
        got = probe.relink(R, links, maxM0, node, off, add_p, add_d, bound)
        same_table(got, want, (dim, dt, metric, cls, maxM0, n_touched, bound))
    if cls == "clustered":
        assert stats[1] * 4 >= stats[0] > 0, stats


def relink_model_f64(D64, links, maxM0, node, off, add_p, ad64):
    """relink_model with float64 distances: the order key of an exact f64 value is the value itself (no NaN, no -0 on lattice rows)"""
    links = links.copy()
    for t, s in enumerate(int(x) for x in node):
        row = links[s]
        w0 = int(row[0])
        cnt = w0 & 0xFFFF
        adds = [int(x) for x in add_p[off[t]:off[t + 1]]]
        old = [int(x) for x in row[1:1 + cnt]]
        if cnt + len(adds) <= maxM0:
            new = old + adds
            row[1 + cnt:1 + len(new)] = adds
        else:
            nadd = min(len(adds), KCAP - cnt)
            ids = old + adds[:nadd]
            d = [D64(e, s) for e in old] + [float(x) for x in ad64[off[t]:off[t] + nadd]]
            order = sorted(range(len(ids)), key=lambda i: (d[i], ids[i], i))
            new = heuristic(D64, [(ids[i], d[i]) for i in order], maxM0)
            row[1:1 + len(new)] = new
        row[0] = (w0 & 0xFFFF0000) | len(new)
    return links, None


def test_relink_marks_both_paths_with_tombstones(oracle):
    """host only: relink_inputs sets the tombstone bit on a node of the append path and on one of the heuristic path"""
    rng = np.random.default_rng(6)
    R = Rows(oracle, make_values("random", RL_ROWS, 13, rng), "f32", "L2")
    for maxM0 in (4, 32, 192):
        links, node, off, add_p, add_d = relink_inputs(R, rng, maxM0, 41)
        tomb = ((links[node, 0] >> 16) & 1).astype(bool)
        full = np.array([(links[s, 0] & 0xFFFF) + (off[t + 1] - off[t]) > maxM0 for t, s in enumerate(node)])
        assert (tomb & full).any() and (tomb & ~full).any(), maxM0
        assert {(int(links[s, 0] & 0xFFFF), int(off[t + 1] - off[t])) for t, s in enumerate(node)} == set(relink_combos(maxM0))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_relink_nan_and_duplicates(probe, oracle, metric, dt):
    """Distances that are not numbers (a NaN element in an old neighbour's row, a NaN add_d, inf - inf between two rows that
    hold +inf under L2) and the same (id, distance) twice among the additions: the ranks of the counting sort stay a
    permutation (csrc/hnsw_relink_order.hpp), so every id written is one of the node's candidates, and the lists are the
    model's: NaN candidates last in (id, position) order, never dominated and never dominating."""
    rng = np.random.default_rng(seed_of(7, metric, dt))
    vals = make_values("clustered", 120, 13, rng)
    NANROW, INF_A, INF_B = 100, 101, 102
    vals[NANROW, 5] = np.nan
    vals[INF_A, 3] = np.inf
    vals[INF_B, 3] = np.inf
    R = Rows(oracle, vals, dt, metric)
    assert np.isnan(R(NANROW, 0)) and (metric != "L2" or (np.isnan(R(INF_A, INF_B)) and np.isinf(R(INF_A, 0))))
    for maxM0 in (4, 32):
        l0s = maxM0 + 2
        links = random_links(rng, R.n, l0s, maxM0, 100)
        node, off, add_p, add_d = [], [0], [], []

        def touch(s, old, adds, dists=None):
            links[s, 0] = (links[s, 0] & np.uint32(0xFFFF0000)) | np.uint32(len(old))
            links[s, 1:1 + len(old)] = old
            d = [R(p, s) for p in adds] if dists is None else dists
            node.append(s)
            add_p.extend(adds)
            add_d.extend(d)
            off.append(len(add_p))

        base = [int(x) for x in rng.choice(np.arange(20, 100), maxM0 - 1, replace=False)]
        nan32 = np.float32(np.nan)
        touch(0, base + [NANROW], [103, 104])                                       # an old neighbour at NaN distance
        touch(1, base + [5], [103, 104, 105], [R(103, 1), nan32, nan32])            # additions with NaN add_d
        touch(2, [NANROW] * 1 + base, [NANROW, 106], [nan32, R(106, 2)])            # NaN twice under one id: position decides
        touch(INF_A, base + [INF_B], [107, 108])                                    # L2: inf - inf = NaN; IP: an infinite distance
        touch(3, base + [INF_A], [INF_B, 109])                                      # two infinite distances: the id decides
        touch(4, base + [6], [110, 110], [R(110, 4)] * 2)                           # the same (id, distance) twice, full list
        touch(7, base[:maxM0 - 2], [111, 111], [R(111, 7)] * 2)                     # ... and on the append path
        touch(8, [NANROW, INF_A] + base[:maxM0 - 2], [112, 112, NANROW], [R(112, 8)] * 2 + [nan32])
        touch(9, [], [113] * (maxM0 + 1), [np.float32(0.5)] * (maxM0 + 1))          # nothing but one pair
        touch(10, [], list(range(20, 21 + maxM0)), [nan32] * (maxM0 + 1))           # nothing but NaN
        node, off = np.array(node, np.uint32), np.array(off, np.uint32)
        add_p, add_d = np.array(add_p, np.uint32), np.array(add_d, np.float32)
        want, allowed = relink_model(R, links, maxM0, node, off, add_p, add_d)
        for bound in (0, 64):
            got = probe.relink(R, links, maxM0, node, off, add_p, add_d, bound)
            for t, s in enumerate(node):
                cnt = int(got[s, 0] & 0xFFFF)
                assert cnt <= maxM0 and set(got[s, 1:1 + cnt].tolist()) <= allowed[t], (metric, dt, maxM0, t, got[s].tolist())
            same_table(got, want, (metric, dt, maxM0, bound))


def test_relink_refuses_what_the_kernel_trusts(probe, oracle):
    rng = np.random.default_rng(8)
    R = Rows(oracle, make_values("random", 60, 13, rng), "f32", "IP")
    links, node, off, add_p, add_d = relink_inputs(R, rng, 4, 5)

    def refused(links=links, maxM0=4, node=node, off=off, add_p=add_p):
        probe.relink(R, links, maxM0, node, off, add_p, add_d, 0, expect_rc=1)

    bad = links.copy()
    bad[int(node[1]), 1] = R.n
    bad[int(node[1]), 0] |= 1
    refused(links=bad)                                                       # a list entry >= n_rows
    bad = links.copy()
    bad[7, 0] = 5
    refused(links=bad)                                                       # cnt > max_keep
    refused(node=np.r_[node[:4], np.uint32(R.n)].astype(np.uint32))          # node >= n_rows
    refused(add_p=np.r_[add_p[:-1], np.uint32(R.n)].astype(np.uint32))       # addition >= n_rows
    o = off.copy()
    o[2], o[3] = off[3], off[2]
    refused(off=o)                                                           # off not ascending
    refused(links=random_links(rng, R.n, 200, 4, R.n), maxM0=193)            # max_keep > 192
    probe.relink(R, links, 4, node, off, add_p, add_d, 3, expect_rc=1)       # a bound below the number of touched nodes


# ---- gather_lists / widen_rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows,l0s,n_new,n_node,touched", [(400, 33, 37, 50, 41), (400, 33, 1, 4, 0), (400, 17, 5, 5, 5),
                                                             (3100, 193, 37, 3000, 2990)])    # the last: more words than threads
def test_gather_lists(probe, n_rows, l0s, n_new, n_node, touched):
    rng = np.random.default_rng([9, n_rows, l0s, n_new])
    links = rng.integers(0, 1 << 32, (n_rows, l0s), dtype=np.uint64).astype(np.uint32)
    first = n_rows - n_new - 3
    node = rng.choice(n_rows, n_node, replace=False).astype(np.uint32)
    if (n_new + touched) * l0s > 2048 * 256:
        assert n_rows == 3100
    dst = probe.gather(links, first, n_new, node, touched)
    want = np.full_like(dst, EE)
    want[:n_new] = links[first:first + n_new]
    want[n_new:n_new + touched] = links[node[:touched]]
    same_table(dst, want, (n_rows, l0s, n_new, touched))


@pytest.mark.parametrize("n_rows,stride,first,n", [(400, 16, 363, 37), (400, 144, 0, 1), (400, 768, 399, 1), (400, 16, 5, 0),
                                                   (900, 768, 60, 800)])                      # the last: more words than threads
def test_widen_rows(probe, n_rows, stride, first, n):
    rng = np.random.default_rng([10, n_rows, stride, first, n])
    rows = rng.integers(0, 1 << 16, (n_rows, stride), dtype=np.uint32).astype(np.uint16)       # every bit pattern, NaNs included
    out = probe.widen(rows, first, n, 2)
    want = np.full_like(out, EE)
    want[:n] = rows[first:first + n].astype(np.uint32) << 16
    same_table(out, want, (n_rows, stride, first, n))


# ---- the chain -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,dt,metric,cls", [(144, "f32", "IP", "clustered"), (144, "bf16", "L2", "clustered"), (13, "f32", "IP", "lattice"),
                                               (768, "bf16", "L2", "random")])
def test_chain(probe, oracle, dim, dt, metric, cls):
    """select, group, relink (maxM0, device-side counts, bound n_new * M) and gather as HnswIndex::device_batch enqueues them:
    ~400 nodes with random valid lists and tombstones, 37 new points, candidates = the exact 100 nearest, M = 16"""
    rng = np.random.default_rng(seed_of(11, dim, dt, metric, cls))
    n_exist, n_new, M, maxM0, efc = 400, 37, 16, 32, 100
    R = Rows(oracle, make_values(cls, n_exist + n_new, dim, rng), dt, metric)
    first, l0s = n_exist, maxM0 + 1
    links = random_links(rng, R.n, l0s, maxM0, n_exist)
    cid, cd, cn = select_inputs_full(R, efc, n_new, first)
    stats = [0, 0]
    l1, sel, picks = select_model(R, links, M, cid, cd, cn, first, stats)
    sid = np.full((n_new, M), EE, np.uint32)
    sd = np.zeros((n_new, M), np.float32)
    for p, kept in enumerate(sel):
        sid[p, :len(kept)] = kept
        sd[p, :len(kept)] = cd[p, picks[p]]
    sn = np.array([len(s) for s in sel], np.uint32)
    w_counts, w_node, w_off, w_p, w_bits = group_model(sid, sd, sn, first)
    want, _ = relink_model(R, l1, maxM0, w_node, w_off, w_p, w_bits.view(np.float32), stats)
    full = sum(int(links[s, 0] & 0xFFFF) + int(w_off[t + 1] - w_off[t]) > maxM0 for t, s in enumerate(w_node))
    assert w_counts[0] >= 20 and 0 < full < w_counts[0], (w_counts.tolist(), full)     # many touched nodes, some on either path
    got, counts, node, lists = probe.chain(R, links, M, maxM0, cid, cd, cn, first)
    what = (dim, dt, metric, cls)
    assert counts.tolist() == w_counts.tolist(), what
    T = int(w_counts[0])
    assert np.array_equal(node[:T], w_node), what
    same_table(got, want, what)
    w_lists = np.full_like(lists, EE)
    w_lists[:n_new] = want[first:first + n_new]
    w_lists[n_new:n_new + T] = want[w_node]
    same_table(lists, w_lists, what)


def select_inputs_full(R, efc, n_new, first):
    """the exact efc nearest existing nodes of every new point, ascending by (distance, id)"""
    cid = np.zeros((n_new, efc), np.uint64)
    cd = np.zeros((n_new, efc), np.float32)
    for p in range(n_new):
        dd = sorted((float(R(first + p, c)), c) for c in range(first))[:efc]
        cid[p] = [c for _, c in dd]
        cd[p] = [d for d, _ in dd]
    return cid, cd, np.full(n_new, efc, np.uint32)
