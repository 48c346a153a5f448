"""Graphs, a model and the case list of tests/test_hnsw_search_kernels_gpu.py (the HNSW search kernels behind
tests/helpers/hnsw_search_probe.hip) -- everything that needs no GPU, so tests/test_hnsw_search_model_cpu.py can pin it.

Graph makers (deterministic, 16 dimensions unless a case is about rows): oracle_built, random_digraph, with_repeats,
with_tombstones.  Rows and queries are random normal floats; the CPU test asserts that no two nodes are equidistant from any
query, so no answer depends on how ties are broken and the reference of every case is simply
oracle.HNSW.from_arrays(...).search(q, k, ef, allow, stats=True).

model(): a heapq restatement of searchKnn (greedy descent + searchBaseLayerST) that is pinned to the oracle and only used to
say what a case REACHES -- peak frontier, visited count, prunes, repeated ids met -- and, with a frontier capacity or a hash
table size, which queries the kernels must give up (their frontier is pruned lazily, when it is full: the model does the same)."""
import ctypes as C
import functools
import heapq

import numpy as np

from oracle import oracle as O

FLT_MAX = np.float32(3.402823466e+38)
NONE = 0xFFFFFFFF
NO_LABEL = 0xFFFFFFFFFFFFFFFF
DELETED = 0x10000
PATTERNS = (0x00000000, 0xFFFFFFFF, 0xEEEEEEEE)
LDS_LIST = 255


class Graph:
    def __init__(self, rows, labels, l0, upper, max_level, entry_point, space, M):
        self.rows = np.ascontiguousarray(rows, np.float32)
        self.labels = np.ascontiguousarray(labels, np.uint64)
        self.l0 = np.ascontiguousarray(l0, np.uint32)
        self.upper = {key: np.asarray(v, np.uint32) for key, v in upper.items()}
        self.max_level, self.entry_point, self.space, self.M = int(max_level), int(entry_point), space, M
        self.n, self.dim = self.rows.shape
        self.levels = np.zeros(self.n, np.int32)
        for (i, lv) in self.upper:
            self.levels[i] = max(self.levels[i], lv)
        self._o = self._flat = None

    def copy(self):
        return Graph(self.rows.copy(), self.labels.copy(), self.l0.copy(), dict(self.upper), self.max_level, self.entry_point,
                     self.space, self.M)

    deleted = property(lambda s: (s.l0[:, 0] & DELETED) != 0)

    def oracle(self):
        if self._o is None:
            self._o = O.HNSW.from_arrays(self.rows, self.labels, self.l0, self.upper, self.max_level, self.entry_point,
                                         self.space, self.M)
        return self._o

    def distances(self, q):
        """The oracle's distance from q to every node, [n] (one brute-force search over the rows, labelled by id)."""
        if self._flat is None:
            self._flat = O.Flat(self.dim, self.space, max_elements=self.n)
            self._flat.add_many(self.rows, labels=np.arange(self.n, dtype=np.uint64))
        od, ol = self._flat.search(q, self.n)
        assert od.size == self.n
        d = np.empty(self.n, np.float32)
        d[ol.astype(np.int64)] = od
        return d

    def device_arrays(self, bf16=False, row_stride=None, slack_bits=0x7FC00000):
        """rows padded to the stride (zeros inside the chunks, NaN bits in the slack behind them), the slot table, the pool"""
        chunks = (self.dim + 15) // 16
        stride = row_stride or 16 * chunks
        r = np.zeros((self.n, stride), np.float32)
        r[:, 16 * chunks:] = np.array([slack_bits], np.uint32).view(np.float32)[0]
        r[:, :self.dim] = self.rows
        if bf16:
            r = np.ascontiguousarray(r.view(np.uint32) >> 16).astype(np.uint16)
        slot = np.full(self.n, NONE, np.uint32)
        n_slots = int(self.levels.sum())
        pool = np.zeros((max(n_slots, 1), self.M + 1), np.uint32)
        at = 0
        for i in np.nonzero(self.levels)[0]:
            slot[i] = at
            for lv in range(1, self.levels[i] + 1):
                ids = self.upper[(int(i), lv)]
                pool[at, 0] = ids.size
                pool[at, 1:1 + ids.size] = ids
                at += 1
        return dict(rows=r, chunks=chunks, row_stride=stride, upper_slot=slot, upper_pool=pool, n_slots=n_slots)


def to_bf16(x):
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def make_rows(n, dim, seed, bf16=False):
    x = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    return to_bf16(x) if bf16 else x


def make_queries(nq, dim, seed):
    return np.random.default_rng(10_000 + seed).standard_normal((nq, dim)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def oracle_built(n, dim=16, M=8, space="L2", seed=1, bf16=False, label_base=0):
    o = O.HNSW(dim, space, max_elements=n, M=M, ef_construction=40, seed=100 + seed)
    o.add_many(make_rows(n, dim, seed, bf16), labels=np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(label_base))
    g = o.export_graph()
    l0 = g["l0"].copy()
    l0[:, 0] |= g["deleted"].astype(np.uint32) << 16
    return Graph(g["rows"], g["labels"], l0, g["upper"], g["max_level"], g["entry_point"], space, M)


@functools.lru_cache(maxsize=None)
def random_digraph(n, M, space="L2", seed=2, dim=16, fan=None, hub=()):
    """Level-0 lists of random length 0 .. 2M (both ends present) with random ids; a few nodes on levels 1 .. 3 with random
    upper lists (up to M long: more than 16, two rounds of the descent, from M = 64).  `fan`: list length of every node
    instead; `hub`: ids that the level-0 list of every node with upper levels names first (the layer-0 search starts at one of them)."""
    rng = np.random.default_rng(seed)
    l0 = np.zeros((n, 2 * M + 1), np.uint32)
    cnt = rng.integers(0, 2 * M + 1, n) if fan is None else np.full(n, fan)
    if n > 3 and fan is None:
        cnt[1], cnt[2] = 0, 2 * M
    for i in range(n):
        l0[i, 0] = cnt[i]
        l0[i, 1:1 + cnt[i]] = rng.integers(0, n, cnt[i])
    n_up = [0, min(n // 4, max(2 * M // 3, 6)), min(n // 8, 6), min(n // 16, 2)]
    levels = np.zeros(n, np.int32)
    order = rng.permutation(n)
    for lv in (1, 2, 3):
        levels[order[:n_up[lv]]] = lv
    max_level = int(levels.max())
    ep = int(order[0])
    upper = {}
    for i in np.nonzero(levels)[0]:
        for lv in range(1, levels[i] + 1):
            peers = np.nonzero(levels >= lv)[0]
            m = int(rng.integers(0, min(M, peers.size) + 1))
            if i == ep:
                m = min(M, peers.size)
            upper[(int(i), lv)] = rng.choice(peers, m, replace=False).astype(np.uint32)
    if len(hub):
        h = np.asarray(hub, np.uint32)[:2 * M]
        for i in np.nonzero(levels)[0]:
            l0[i, 0] = max(int(l0[i, 0]), h.size)
            l0[i, 1:1 + h.size] = h
    rows = make_rows(n, dim, seed)
    if n > 4000:     # thousands of f32 distances within a few binades collide: norms over many binades keep them distinct
        rows = rows * np.exp(rng.uniform(0, 12, n)).astype(np.float32)[:, None]
    return Graph(rows, np.arange(n, dtype=np.uint64) * np.uint64(5) + np.uint64(7), l0, upper, max_level, ep, space, M)


def with_repeats(g, q):
    """Repeated ids where a search for q meets them first: in the list of the FIRST node the layer-0 search expands (all of
    its neighbours are new then) position 9 repeats position 3 -- the same round of 64 lanes -- and, from M = 64, position 70
    repeats it again -- the next round; the second expanded node names the entry of the search (visited long before) twice
    and itself once (a self-loop at level 0); the entry point's top-level list names the entry point (one at an upper level)."""
    m = model(g, q, 1, g.n)
    g = g.copy()
    first, second = m["expanded"][0], m["expanded"][1]
    l = g.l0[first]
    need = 71 if g.M >= 64 else 10
    if (l[0] & 0xFFFF) < need:
        fill = np.random.default_rng(5).permutation(g.n)[:need].astype(np.uint32)
        l[1 + (l[0] & 0xFFFF):1 + need] = fill[(l[0] & 0xFFFF):need]
        l[0] = (l[0] & ~np.uint32(0xFFFF)) | np.uint32(need)
    l[1 + 9] = l[1 + 3]
    if g.M >= 64:
        l[1 + 70] = l[1 + 3]
    if second not in l[1:1 + need].tolist():
        l[1] = second                                    # (keeps the second node reachable)
    s = g.l0[second]
    c = int(s[0] & 0xFFFF)
    if c < 3:
        s[0] = (s[0] & ~np.uint32(0xFFFF)) | np.uint32(3)
    s[1], s[2], s[3] = first, second, first
    if g.max_level > 0:
        top = g.upper[(g.entry_point, g.max_level)].copy()
        if top.size:
            top[top.size // 2] = g.entry_point
            g.upper[(g.entry_point, g.max_level)] = top
    return g


def with_tombstones(g, share, entry_too=True, seed=3):
    g = g.copy()
    dead = np.random.default_rng(seed).random(g.n) < share
    dead[g.entry_point] = entry_too
    g.l0[dead, 0] |= np.uint32(DELETED)
    return g


def allowed_nodes(g, allow=None, nbits=None):
    """[n] bool: live and allowed by a label bitmap (what mask_bits / live_bits state per internal id)"""
    ok = ~g.deleted
    if allow is not None:
        nbits = allow.size * 64 if nbits is None else nbits
        lab = g.labels
        inb = lab < np.uint64(nbits)
        w = np.zeros(g.n, np.uint64)
        w[inb] = (allow[(lab[inb] >> np.uint64(6)).astype(np.int64)] >> (lab[inb] & np.uint64(63))) & np.uint64(1)
        ok &= w != 0
    return ok


def node_bitmap(ok):
    bits = np.zeros((ok.size + 63) // 64, np.uint64)
    idx = np.nonzero(ok)[0].astype(np.uint64)
    np.bitwise_or.at(bits, (idx >> np.uint64(6)).astype(np.int64), np.uint64(1) << (idx & np.uint64(63)))
    return bits


def model(g, q, k, ef, ok=None, cap=None, give_up=False, hash_log2=0, dist=None):
    """searchKnn on graph g.  ok: [n] bool (live and allowed), None = all live.  cap: frontier capacity with the kernels' lazy
    prune (None: the reference's unbounded candidate_set); give_up: a query whose frontier stays full after the prune is
    abandoned (else the entry is dropped and counted).  hash_log2: a query is abandoned at the hop whose list could take
    the visited table past 3/4."""
    d = g.distances(q) if dist is None else dist
    ok = ~g.deleted if ok is None else ok
    cur, curd = g.entry_point, d[g.entry_point]
    self_upper = False
    for level in range(g.max_level, 0, -1):
        changed = True
        while changed:
            changed = False
            for cid in g.upper[(cur, level)].tolist():      # (the list of the node the pass started from, hnswalg.h:1674-1694)
                self_upper |= cid == cur
                if d[cid] < curd:
                    curd, cur, changed = d[cid], cid, True
    res = dict(abandoned=False, over=0, prunes=0, peak=1, evals=0, hops=0, expanded=[], repeat_same=0, repeat_cross=0,
               repeat_old=0, self_loops=0, self_upper=self_upper, far_new=False, full=False, rem_small=False, rem_mid=False,
               list_sum=0, entry_ok=bool(ok[cur]), entry_deleted=bool(g.deleted[cur]), visited=1, entry=cur)
    top, cand, visited = [], [], {cur}
    if ok[cur]:
        lb = d[cur]
        heapq.heappush(top, (-d[cur], cur))
        res["evals"] += 1
        heapq.heappush(cand, (d[cur], cur))
    else:
        lb = FLT_MAX
        heapq.heappush(cand, (FLT_MAX, cur))
    while cand:
        cd, c = cand[0]
        if cd > lb and len(top) == ef:
            break
        heapq.heappop(cand)
        res["hops"] += 1
        res["expanded"].append(c)
        lst = g.l0[c, 1:1 + (g.l0[c, 0] & 0xFFFF)].tolist()
        res["list_sum"] += len(lst)
        if hash_log2 and len(visited) + len(lst) > (3 << hash_log2) // 4:
            res["abandoned"] = True
            break
        new, seen_here = [], {}
        for pos, nid in enumerate(lst):
            res["self_loops"] += nid == c
            if nid in visited:
                if nid in seen_here:
                    res["repeat_same" if seen_here[nid] // 64 == pos // 64 else "repeat_cross"] += 1
                elif nid != c:
                    res["repeat_old"] += 1
                continue
            visited.add(nid)
            seen_here[nid] = pos
            new.append(nid)
            res["far_new"] |= pos >= 64
        res["evals"] += len(new)
        res["rem_small"] |= 1 <= len(new) % 16 <= 4           # (the last distance round: four quads per row, or two)
        res["rem_mid"] |= 5 <= len(new) % 16 <= 8
        for nid in new:
            if not (len(top) < ef or lb > d[nid]):
                continue
            if cap is not None and len(cand) == cap:
                if len(top) == ef:
                    cand = [e for e in cand if not e[0] > lb]
                    heapq.heapify(cand)
                    res["prunes"] += 1
                if len(cand) == cap:
                    if give_up:
                        res["abandoned"] = True
                        break
                    res["over"] += 1
            if cap is None or len(cand) < cap:
                heapq.heappush(cand, (d[nid], nid))
                res["peak"] = max(res["peak"], len(cand))
            if ok[nid]:
                heapq.heappush(top, (-d[nid], nid))
                if len(top) > ef:
                    heapq.heappop(top)
            if top:
                lb = -top[0][0]
            res["full"] |= len(top) == ef
        if res["abandoned"]:
            break
    res["visited"] = len(visited)
    res["visited_ids"] = np.fromiter(visited, np.int64, len(visited))
    out = sorted((float(-nd), int(g.labels[i]), i) for nd, i in top)[:k]
    res["dist"] = np.array([e[0] for e in out], np.float32)
    res["labels"] = np.array([e[1] for e in out], np.uint64)
    res["ids"] = np.array([e[2] for e in out], np.uint64)
    return res


# ---- launch descriptions (mirrors of the probe's structs) --------------------------------------------------------------
class HsGraph(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rows", "labels", "links0", "levels", "upper_slot", "upper_pool", "queries")] + \
               [(n, C.c_uint32) for n in ("row_stride", "chunks", "l0_stride", "up_stride", "n_slots", "entry_point")] + \
               [("max_level", C.c_int32)] + [(n, C.c_uint32) for n in ("n_nodes", "q_stride", "nq")]


class HsLaunch(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("l2", "bf16", "e")] + \
               [(n, C.c_uint32) for n in ("ef", "k", "blocks", "cand_cap", "gpool_level", "vis_hash_log2", "vis_mode", "nbr_cap",
                                          "check_deleted", "out_ids", "with_redo_out", "with_totals", "pattern", "cancel")] + \
               [("allow_nbits", C.c_uint64)] + \
               [(n, C.c_void_p) for n in ("allow_bits", "allow_tab", "allow_nbits_tab", "live_bits", "mask_bits", "mask_tab", "cancel_q",
                                          "out_dist", "out_label", "out_n", "stats", "totals", "redo")] + \
               [(n, C.c_uint32) for n in ("queue", "waves_per_block", "lds_bytes", "latency", "blocks_used")]


def slots_per_lane(ef, gpool=0):
    """hnsw_slots_per_lane, with the LDS list where hnsw_list_in_lds says so"""
    if ef > 1024 or (ef > 512 and gpool):
        return LDS_LIST
    return 1 if ef <= 64 else 2 if ef <= 128 else 4 if ef <= 256 else 8 if ef <= 512 else 16


def launch(g, ef, k, **kw):
    """A launch description with the arguments hnsw_index.cc would choose, overridden by kw"""
    gpool = kw.get("gpool_level", 0)
    d = dict(l2=int(g.space == "L2"), bf16=0, e=slots_per_lane(ef, gpool), ef=ef, k=k, blocks=0, gpool_level=gpool, vis_hash_log2=0,
             vis_mode=0, nbr_cap=(2 * g.M + 63) & ~63, check_deleted=int(g.deleted.any()), out_ids=0, with_redo_out=0, with_totals=1,
             cancel=0, allow_bits=None, allow_nbits=0, allow_tab=None, allow_nbits_tab=None, live_bits=None, mask_bits=None,
             mask_tab=None, cancel_q=None)
    d["cand_cap"] = {0: max(2 * ef, 64), 1: min(65536, (max(2 * ef, g.n) + 127) & ~127), 2: (g.n + 8191) & ~8191}[gpool]
    if kw.get("vis_hash_log2"):
        d["cand_cap"] = (ef + max(64, ef // 4) + 3) & ~3
        d["with_redo_out"] = 1
    d.update(kw)
    return d


# ---- the cases ---------------------------------------------------------------------------------------------------------
class Case:
    """graph: () -> Graph.  first / second: keyword arguments of launch() (second: the chained launch, or None).  allow:
    (graph, q index) -> (bitmap, nbits) or None; via: how the filter reaches the kernel (allow_bits, allow_tab, mask_bits,
    mask_tab; tombstones alone: none or live_bits).  path: (text, predicate over the per-query models of the FIRST launch) --
    what the case is there to reach, asserted on the CPU.  kernel: the entry point the first launch must take."""

    def __init__(self, name, graph, nq, ef, k, kernel, path, first=None, second=None, allow=None, via="allow_bits", bf16=False,
                 row_stride=None, q_stride=None, qseed=0, use_model=True, make_q=None, ref_from_model=False):
        self.name, self.graph, self.nq, self.ef, self.k, self.kernel, self.path = name, graph, nq, ef, k, kernel, path
        self.first, self.second, self.allow, self.via, self.bf16 = first or {}, second, allow, via, bf16
        self.row_stride, self.q_stride, self.qseed, self.use_model = row_stride, q_stride, qseed, use_model
        self.make_q, self.ref_from_model = make_q, ref_from_model

    def queries(self, g):
        """random queries, without the few from which two nodes are exactly equidistant (a tie in f32 turns up about once
        in a thousand queries over a few hundred nodes)"""
        if getattr(self, "_q", None) is None:
            cand = self.make_q(g, self.nq) if self.make_q else candidate_queries(self.nq, g.dim, self.qseed)
            keep = [q for q in cand if np.unique(g.distances(q).view(np.uint32)).size == g.n]
            assert len(keep) >= self.nq
            self._q = np.stack(keep[:self.nq])
        return self._q

    def launches(self, g):
        a = launch(g, self.ef, self.k, bf16=int(self.bf16), **self.first)
        b = None if self.second is None else launch(g, self.ef, self.k, bf16=int(self.bf16), **self.second)
        return a, b

    def filters(self, g):
        one = self.via in ("allow_bits", "mask_bits")         # (one filter for the whole batch)
        Q = self.queries(g)
        return [self.allow(g, 0 if one else i, Q[0 if one else i]) if self.allow else None for i in range(self.nq)]

    def first_models(self, g):
        """the model of every query under the FIRST launch's frontier capacity and table size"""
        a, _ = self.launches(g)
        hashed = a["vis_hash_log2"] != 0
        cap = None if a["gpool_level"] == 2 else a["cand_cap"]
        give_up = bool(a["with_redo_out"]) and (a["gpool_level"] == 1 or hashed)
        log2 = a["vis_hash_log2"] if hashed and a["vis_mode"] in (0, 1, 2) else 0
        Q, F = self.queries(g), self.filters(g)
        return [model(g, Q[i], self.k, self.ef, allowed_nodes(g, *(F[i] or (None, None))), cap, give_up, log2) for i in range(self.nq)]


def candidate_queries(nq, dim, seed):
    """what Case.queries draws from (a few spares for the ones that meet a tie)"""
    return make_queries(nq + 8 + nq // 16, dim, seed)


def lds_set_capacity(mode):
    return 1024 * 6 if mode == 3 else 2048 * 8


def lds_verdict(a, g, m):
    """modes 3 / 5: False = the query is certainly NOT given up by the spill table's 3/4 rule, True = certainly given up, None =
    neither can be shown.  q_hbm + size never exceeds the sum of the list lengths of the expanded nodes; more visited ids than
    the on-chip set and 3/4 of the table hold together cannot be kept."""
    thr = (3 << a["vis_hash_log2"]) // 4
    if m["abandoned"]:
        return True                                            # (the LDS frontier filled up: the model's own verdict)
    if m["list_sum"] <= thr:
        return False
    if m["visited"] > lds_set_capacity(a["vis_mode"]) + thr + 2 * g.M:
        return True
    return None


def expected_lds_bytes(a, g, chunks, nq):
    """hnsw_lds_bytes: the per-wave carve of hnsw_search_body times the waves per block"""
    lds_list = a["e"] == LDS_LIST
    pool = {0: a["cand_cap"] * 2, 1: a["cand_cap"] // 128 * 2, 2: a["cand_cap"] // 8192 * 2}[a["gpool_level"]]
    vis = 0
    if a["vis_hash_log2"]:
        vis = {0: 0, 1: 0, 2: (1 << a["vis_hash_log2"]) // 32, 3: 1024 * 3, 5: 2048 * 4}[a["vis_mode"]]
    per_wave_f4 = chunks * 4 + ((2 * a["ef"] if lds_list else 0) + pool + a["nbr_cap"] * 2 + vis + 3) // 4
    return per_wave_f4 * 16 * kernel_of(a, nq)[1]


def kernel_of(a, nq):
    """the __global__ entry point hnsw_pick chooses, and the waves per block it is launched with (hnsw_search.hip)"""
    e, lds_list = a["e"], a["e"] == LDS_LIST
    latency = nq <= 1024
    if a["vis_hash_log2"]:
        name = {0: "hash", 1: "hash", 2: "bucket", 3: "ldsvis", 5: "ldsvis_big"}[a["vis_mode"]]
        return name, 1 if lds_list else 4
    wpb = 1 if lds_list or latency else 4
    if a["gpool_level"] == 2:
        return "gpool2", wpb
    if a["gpool_level"] == 1:
        return ("gpool_latency" if latency and e <= 4 else "gpool"), wpb
    return ("latency" if latency and e <= 4 else "plain"), wpb


def _some(key, pred=bool):
    return lambda ms: any(pred(m[key]) for m in ms)


def _none_allowed(g, i, q=None):
    return np.zeros((int(g.labels.max()) + 64) // 64, np.uint64), int(g.labels.max()) + 1


def _third(g, i, q=None):
    """labels of every third node plus the neighbourhood of nothing in particular: about a third of the graph"""
    nb = int(g.labels.max()) + 1
    return O.allow_bitmap(g.labels[(np.arange(g.n) + i) % 3 == 0], nb), nb


def _third_short(g, i, q=None):
    bits, nb = _third(g, i)
    return bits, nb // 2                                    # allow_nbits below the largest label: the rest is not allowed


def _tab(g, i, q=None):
    return None if i % 3 == 1 else _third_short(g, i) if i % 3 == 2 else _third(g, i)


def _not_entry(g, i, q=None):
    """everything but the node the layer-0 search of THIS query starts from (where the descent ends)"""
    nb = int(g.labels.max()) + 1
    return O.allow_bitmap(g.labels[np.arange(g.n) != model(g, q, 1, 1)["entry"]], nb), nb


@functools.lru_cache(maxsize=None)
def _entries_tombstoned():
    """the 600-node graph with a tenth of its nodes tombstoned -- and the layer-0 entry of every query the cases can draw"""
    g = with_tombstones(oracle_built(600, 16, 8, "L2", 4), 0.1, entry_too=False)
    for q in candidate_queries(4, 16, 0):
        g.l0[model(g, q, 1, 1)["entry"], 0] |= np.uint32(DELETED)
    return g


@functools.lru_cache(maxsize=None)
def _alternating(dead=False):
    """the 600-node graph plus one node X far from everything with NO level-0 neighbours, named by the entry point's top list
    and present on every upper level: a query next to X descends to it and its layer-0 search ends at once"""
    b = oracle_built(600, 16, 8, "L2", 4)
    assert b.max_level >= 1
    X = b.n
    rows = np.vstack([b.rows, np.full((1, 16), 40, np.float32)])
    labels = np.append(b.labels, np.uint64(3 * X))
    l0 = np.vstack([b.l0, np.zeros((1, b.l0.shape[1]), np.uint32)])
    upper = dict(b.upper)
    top = upper[(b.entry_point, b.max_level)]
    upper[(b.entry_point, b.max_level)] = np.append(top[:b.M - 1], np.uint32(X))
    for lv in range(1, b.max_level + 1):
        upper[(X, lv)] = np.zeros(0, np.uint32)
    g = Graph(rows, labels, l0, upper, b.max_level, b.entry_point, "L2", b.M)
    if dead:
        g = with_tombstones(g, 0.3)
        g.l0[X, 0] &= ~np.uint32(DELETED)
    return g


def _alternating_queries(g, nq):
    """even: random (a long search), odd: next to X (a search of one node)"""
    C = make_queries(2 * nq + 16, g.dim, 3)
    distinct = lambda q: np.unique(g.distances(q).view(np.uint32)).size == g.n
    longs = [q for q in C[:nq + 8] if distinct(q)]
    shorts = [q for q in (g.rows[g.n - 1] + 0.01 * C[nq + 8:]) if distinct(q)]
    return np.stack([(longs if i % 2 == 0 else shorts)[i // 2] for i in range(nq)])


def _special_ids(n):
    """ids whose LDS key would read as an empty slot: the low bits of the second bijection all ones (14 for the small set --
    its (c, d) = (1, 1) key is then 0xFFFF --, 13 for the big one)"""
    ids = np.arange(n, dtype=np.uint64)
    H1 = (ids * np.uint64(0x85EBCA6B) + np.uint64(0x5BD1E9)) & np.uint64(0xFFFFFF)
    return np.nonzero((H1 & np.uint64(0x3FFF)) == np.uint64(0x3FFF))[0], np.nonzero((H1 & np.uint64(0x1FFF)) == np.uint64(0x1FFF))[0]


@functools.lru_cache(maxsize=None)
def _special_graph():
    small, big = _special_ids(33000)
    return random_digraph(33000, 16, seed=13, hub=tuple(int(x) for x in np.unique(np.concatenate([small, big]))))


G_PLAIN = lambda sp="L2", bf=False: (lambda: oracle_built(2500, 16, 8, sp, 1, bf))
G_SMALL = lambda sp="L2", bf=False: (lambda: oracle_built(600, 16, 8, sp, 4, bf))
G_TINY = lambda sp="L2": (lambda: oracle_built(300, 16, 8, sp, 6))
G_DEAD = lambda sp="L2": (lambda: with_tombstones(oracle_built(600, 16, 8, sp, 4), 0.3))
FULL = ("some result list reaches ef", _some("full"))
ANY = ("answers", lambda ms: True)


@functools.lru_cache(maxsize=None)
def _repeats(M, space="L2"):
    g = random_digraph(300, M, space, seed=8)
    return with_repeats(g, make_queries(1, 16, 0)[0])


@functools.lru_cache(maxsize=None)
def _big_labels():
    g = oracle_built(600, 16, 8, "L2", 4).copy()
    g.labels[::2] += np.uint64(1 << 41)
    return g


def _cases():
    cs = []
    add = lambda *a, **kw: cs.append(Case(*a, **kw))
    # 1. every entry point, by name ------------------------------------------------------------------------------------
    for sp in ("L2", "IP"):
        for ef in (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2000):
            e = slots_per_lane(ef)
            add(f"plain-{sp}-ef{ef}", G_PLAIN(sp), 6, ef, min(ef, 10), "latency" if e <= 4 else "plain", FULL)
        for ef in (10, 100, 200):
            add(f"throughput-{sp}-ef{ef}", G_TINY(sp), 1025, ef, min(ef, 10), "plain", FULL)
        for mode in (0, 1, 2, 3, 5):
            for ef in (40, 100, 200, 400, 600):
                if mode == 5 and ef > 512:
                    continue
                lg = 14 if mode >= 3 else 12     # (modes 3 / 5: the lists of a search add up to less than 3/4 of the spill table)
                add(f"hash{mode}-{sp}-ef{ef}", G_SMALL(sp), 8, ef, 10, kernel_of(dict(e=1, vis_hash_log2=lg, vis_mode=mode), 8)[0],
                    ("nothing abandoned", lambda ms: not any(m["abandoned"] for m in ms)), first=dict(vis_hash_log2=lg, vis_mode=mode))
        for ef, kern in ((32, "gpool_latency"), (200, "gpool_latency"), (300, "gpool"), (600, "gpool"), (1000, "gpool")):
            add(f"gpool1-{sp}-ef{ef}", G_DEAD(sp), 6, ef, 10, kern, ANY, first=dict(gpool_level=1))
        add(f"gpool1-throughput-{sp}", G_DEAD(sp), 1025, 20, 10, "gpool", FULL, first=dict(gpool_level=1))
        add(f"gpool2-second-{sp}", G_DEAD(sp), 6, 50, 10, "gpool_latency", ("every frontier outgrows 128", lambda ms: all(m["abandoned"] for m in ms)),
            first=dict(gpool_level=1, cand_cap=128, with_redo_out=1), second=dict(gpool_level=2), allow=_none_allowed)
    for ef in (64, 257, 1025):
        add(f"plain-bf16-ef{ef}", G_PLAIN("L2", True), 6, ef, 10, "latency" if ef <= 256 else "plain", FULL, bf16=True)
    add("hash3-bf16", G_SMALL("IP", True), 8, 100, 10, "ldsvis", ANY, first=dict(vis_hash_log2=14, vis_mode=3), bf16=True)
    add("gpool1-bf16", G_SMALL("L2", True), 6, 50, 10, "gpool_latency", ANY, first=dict(gpool_level=1), allow=_third, bf16=True)
    # 2. one wave slot, many queries ------------------------------------------------------------------------------------
    # queries alternate between a long search (most of the graph) and one that ends at its first node: a visited set, a
    # spill table or segment minima left over from the long one change the next one's work
    def many(nq):
        return ("long searches (over 480 of 601 nodes visited) alternate with searches of one node",
                lambda ms: all(m["abandoned"] or m["visited"] > 480 for m in ms[0::2]) and all(m["visited"] == 1 for m in ms[1::2]))
    alt, alt_dead = (lambda: _alternating()), (lambda: _alternating(True))
    for nq in (1, 3, 4, 5, 40):
        kw = dict(make_q=_alternating_queries)
        add(f"oneblock-bitmap-nq{nq}", alt, nq, 500, 10, "plain", many(nq), first=dict(blocks=1), **kw)
        for mode in (0, 1, 2, 3, 5):
            lg = 14 if mode >= 3 else 11
            add(f"oneblock-hash{mode}-nq{nq}", alt, nq, 500, 10, kernel_of(dict(e=1, vis_hash_log2=lg, vis_mode=mode), nq)[0], many(nq),
                first=dict(blocks=1, vis_hash_log2=lg, vis_mode=mode), **kw)
        add(f"oneblock-gpool1-nq{nq}", alt_dead, nq, 500, 10, "gpool", many(nq), first=dict(blocks=1, gpool_level=1), **kw)
        add(f"oneblock-gpool2-nq{nq}", alt_dead, nq, 500, 10, "hash", many(nq), first=dict(blocks=1, vis_hash_log2=4),
            second=dict(blocks=1, gpool_level=2), **kw)
        add(f"oneblock-ldslist-nq{nq}", alt, nq, 1100, 10, "plain", many(nq), first=dict(blocks=1), **kw)
    # ... and with a spill table in use: six searches that outgrow the on-chip set on the four wave slots of one block
    for mode, n, ef, lg in ((3, 12000, 150, 15), (5, 24000, 480, 16)):
        add(f"oneblock-spill-hash{mode}", lambda n=n: random_digraph(n, 64, seed=11), 6, ef, 10, "ldsvis" if mode == 3 else "ldsvis_big",
            ("more visited ids than the on-chip set holds, two queries on one wave",
             lambda ms, mode=mode: all(m["visited"] > lds_set_capacity(mode) + 128 for m in ms)),
            first=dict(blocks=1, vis_hash_log2=lg, vis_mode=mode), make_q=lambda g, nq: make_queries(40, g.dim, 0))
    # 3. hand-made graphs -----------------------------------------------------------------------------------------------
    for M in (3, 16, 64, 96):
        far = ("a list longer than 64 with an unvisited id beyond position 64", _some("far_new")) if M >= 64 else ANY
        add(f"digraph-M{M}-bitmap", lambda M=M: random_digraph(400, M), 6, 50, 10, "latency", far)
        add(f"digraph-M{M}-ldsvis", lambda M=M: random_digraph(400, M), 6, 50, 10, "ldsvis", far, first=dict(vis_hash_log2=15, vis_mode=3))
        add(f"digraph-M{M}-IP-gpool", lambda M=M: with_tombstones(random_digraph(400, M, "IP"), 0.2), 6, 300, 10, "gpool", far,
            first=dict(gpool_level=1))
    for M in (16, 64):
        rep = ("a repeated id in one round of 64%s, a repeat of a visited id, a self-loop at level 0 and above" % (" and across rounds" if M == 64 else ""),
               lambda ms, M=M: ms[0]["repeat_same"] >= 1 and (M < 64 or ms[0]["repeat_cross"] >= 1) and ms[0]["repeat_old"] >= 1
               and ms[0]["self_loops"] >= 1 and ms[0]["self_upper"])
        add(f"repeats-M{M}-bitmap", lambda M=M: _repeats(M), 4, 300, 300, "plain", rep)
        for mode in (0, 1, 2, 3, 5):
            lg = 16 if mode >= 3 else 12
            add(f"repeats-M{M}-hash{mode}", lambda M=M: _repeats(M), 4, 300, 300, kernel_of(dict(e=1, vis_hash_log2=lg, vis_mode=mode), 4)[0], rep,
                first=dict(vis_hash_log2=lg, vis_mode=mode))
    one = lambda: Graph(make_rows(1, 16, 9), [42], np.zeros((1, 17), np.uint32), {}, 0, 0, "L2", 8)
    add("single-node", one, 3, 10, 5, "latency", ("one result", lambda ms: all(m["labels"].tolist() == [42] for m in ms)))
    add("fewer-reachable-than-k", lambda: random_digraph(400, 3), 4, 400, 400, "plain",
        ("fewer results than k", lambda ms: all(m["labels"].size < 400 for m in ms)))
    add("entry-tombstoned", _entries_tombstoned, 4, 40, 10, "gpool_latency",
        ("the entry of every layer-0 search is tombstoned", lambda ms: all(m["entry_deleted"] and not m["entry_ok"] for m in ms)), first=dict(gpool_level=1))
    add("entry-filtered", G_SMALL(), 4, 40, 10, "gpool_latency",
        ("the entry of every layer-0 search is filtered out, not tombstoned", lambda ms: all(not m["entry_ok"] and not m["entry_deleted"] for m in ms)),
        first=dict(gpool_level=1), allow=_not_entry, via="allow_tab")
    add("entry-both", _entries_tombstoned, 4, 40, 10, "gpool_latency",
        ("the entry of every layer-0 search is tombstoned and filtered out", lambda ms: all(m["entry_deleted"] and not m["entry_ok"] for m in ms)),
        first=dict(gpool_level=1), allow=_not_entry, via="allow_tab")
    # 4. visited sets at their edges ---------------------------------------------------------------------------------------
    mixed = ("some queries cross 3/4 of the table, others do not", lambda ms: 0 < sum(m["abandoned"] for m in ms) < len(ms))
    for mode in (0, 1, 2):
        add(f"table-small-hash{mode}", G_SMALL(), 24, 10, 10, kernel_of(dict(e=1, vis_hash_log2=7, vis_mode=mode), 24)[0], mixed,
            first=dict(vis_hash_log2=7, vis_mode=mode), second=dict())
    big = lambda n: (lambda: random_digraph(n, 64, seed=11))
    spill = lambda lim: ("more than %d visited ids" % lim, lambda ms: all(m["visited"] > lim for m in ms))
    add("spill-ldsvis-12k", big(12000), 3, 150, 10, "ldsvis", spill(6144 + 24 + 128), first=dict(vis_hash_log2=15, vis_mode=3))
    add("spill-ldsvis-big-24k", big(24000), 3, 480, 10, "ldsvis_big", spill(16384 + 24 + 128), first=dict(vis_hash_log2=16, vis_mode=5))
    # ids whose LDS key would read as "empty", named by the node every layer-0 search starts from
    for mode, which in ((3, 0), (5, 1)):
        add(f"special-keys-hash{mode}", _special_graph, 3, 50, 10, "ldsvis" if mode == 3 else "ldsvis_big",
            ("an id whose key would read as an empty slot is visited",
             lambda ms, which=which: all(np.intersect1d(m["visited_ids"], _special_ids(33000)[which]).size > 0 for m in ms)),
            first=dict(vis_hash_log2=13, vis_mode=mode), make_q=lambda g, nq: make_queries(60, g.dim, 0))
    add("spill-abandoned-12k", big(12000), 3, 150, 10, "ldsvis", spill(6144 + 24 + 128), first=dict(vis_hash_log2=5, vis_mode=3),
        second=dict(gpool_level=2))
    add("spill-abandoned-big-24k", big(24000), 3, 480, 10, "ldsvis_big", spill(16384 + 24 + 128), first=dict(vis_hash_log2=5, vis_mode=5),
        second=dict(gpool_level=2))
    # 5. frontiers --------------------------------------------------------------------------------------------------------
    add("lds-frontier-full", G_SMALL(), 8, 16, 10, "latency", ("the full frontier is pruned and nothing is dropped",
        lambda ms: any(m["prunes"] for m in ms) and not any(m["over"] for m in ms)), first=dict(cand_cap=64), allow=_third)
    # ... and one size smaller: entries that find it full after the prune are dropped and counted (stats[2]); the search
    # then differs from the reference's, so the expected answer is the model's
    add("lds-frontier-drops", G_SMALL(), 8, 16, 10, "latency", ("frontier entries are dropped", lambda ms: sum(m["over"] for m in ms) > 4),
        first=dict(cand_cap=48), allow=_third, ref_from_model=True)
    for cap in (128, 256):
        add(f"gpool1-cap{cap}", G_DEAD(), 40, 28 if cap == 128 else 70, 10, "gpool_latency",
            ("frontiers that peak just below the capacity, exactly at it, and beyond it",
             lambda ms, cap=cap: any(m["abandoned"] for m in ms) and any(not m["abandoned"] and m["peak"] == cap for m in ms)
             and any(cap - 16 <= m["peak"] < cap for m in ms)),
            first=dict(gpool_level=1, cand_cap=cap, with_redo_out=1), second=dict(gpool_level=2), allow=_third, via="allow_tab")
    for n, cap in ((8000, 8192), (12000, 16384)):
        add(f"gpool2-cap{cap}", lambda n=n: random_digraph(n, 16, seed=12), 2, 20, 10, "gpool2",
            ("a frontier of more than 4096 entries", lambda ms: all(m["peak"] > 4096 for m in ms)), first=dict(gpool_level=2), allow=_none_allowed)
    # 6. filters and masks ----------------------------------------------------------------------------------------------
    for via in ("allow_bits", "mask_bits"):
        add(f"filter-{via}", G_DEAD(), 6, 40, 10, "gpool_latency", ANY, first=dict(gpool_level=1), allow=_third, via=via)
        add(f"filter-short-{via}", G_SMALL(), 6, 40, 10, "gpool_latency", ANY, first=dict(gpool_level=1), allow=_third_short, via=via)
        add(f"filter-big-labels-{via}", _big_labels, 6, 40, 10, "gpool_latency", ANY, first=dict(gpool_level=1),
            allow=lambda g, i, q=None: (O.allow_bitmap(g.labels[1::4], 4096), 4096), via=via)
    for via in ("allow_tab", "mask_tab"):
        add(f"filter-{via}", G_DEAD(), 7, 40, 10, "gpool_latency", ANY, first=dict(gpool_level=1), allow=_tab, via=via)
    add("tombstones-live-bits", G_DEAD(), 6, 40, 10, "gpool_latency", ANY, first=dict(gpool_level=1), via="live_bits")
    add("out-ids", G_SMALL(), 6, 40, 10, "latency", ANY, first=dict(out_ids=1))
    # 7. rows ---------------------------------------------------------------------------------------------------------------
    for chunks in (1, 3, 7, 8, 9, 12, 13, 24, 25, 48, 49):
        dim = 40 if chunks == 3 else 16 * chunks
        gr = lambda dim=dim: oracle_built(150, dim, 8, "L2", 20 + dim)
        add(f"rows-c{chunks}-batch8", gr, 4, 300, 10, "plain", ANY)      # (eight slots per lane: the 8-piece kernel at any batch size)
        add(f"rows-c{chunks}-batch12", gr, 4, 30, 10, "hash", ANY, first=dict(vis_hash_log2=10))
        add(f"rows-c{chunks}-batch24", gr, 4, 30, 10, "ldsvis", ANY, first=dict(vis_hash_log2=13, vis_mode=3))
        add(f"rows-c{chunks}-batch48", gr, 4, 30, 10, "latency", ANY)
    for chunks in (96, 144, 192):
        gr = lambda chunks=chunks: with_tombstones(random_digraph(150, 16, "IP", seed=30 + chunks, dim=16 * chunks), 0.1, entry_too=False)
        rem = ("rounds of 1-4 and of 5-8 unvisited neighbours", lambda ms: any(m["rem_small"] for m in ms) and any(m["rem_mid"] for m in ms))
        add(f"rows-c{chunks}-split-latency", lambda chunks=chunks: random_digraph(150, 16, "IP", seed=30 + chunks, dim=16 * chunks), 3, 30, 10,
            "latency", rem)
        add(f"rows-c{chunks}-split-gpool-latency", gr, 3, 30, 10, "gpool_latency", rem, first=dict(gpool_level=1))
    add("row-stride-slack", G_SMALL(), 4, 40, 10, "latency", ANY, row_stride=48)
    add("query-stride-slack", G_SMALL(), 4, 40, 10, "latency", ANY, q_stride=64)
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
