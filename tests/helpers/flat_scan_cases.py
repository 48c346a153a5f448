"""Models, inputs and case lists shared by tests/test_flat_scan_kernels_gpu.py (which runs the cases on the device through
tests/helpers/flat_scan_probe.hip) and tests/test_flat_scan_model_cpu.py (which checks the models and that every case reaches the
path it is meant for).

Nothing here restates a kernel's arithmetic.  Distances are the oracle's bits (Data.table); selection is select_model of
flat_select_cases.py; which partial list a row belongs to is restated from the comments and layouts of csrc/kernels.hpp,
csrc/flat_gemm.hip and csrc/flat_scan.hip:

K4  tile t = rows [128 t, 128 t + 128); contig = 1: partition rp owns t_base + (rp < t_rem) consecutive tiles from
    rp * t_base + min(rp, t_rem); contig = 0: tiles rp, rp + nrp, ...; inside a tile list slot s = wave * 2 + kk owns the rows
    with (row % 128) / 32 == wave and (row % 8) / 4 == kk; list (q, rp, s) lives at ((q * nrp + rp) * 8 + s) * k.
K3  tile t = 16 rows from row_begin; wave g = rp * 4 + wave owns tiles g, g + 4 nrp, ...; e > 1: list (q, g) at
    (q * 4 nrp + g) * k; e == 1: one list per block at (q * nrp + rp) * k over the block's four waves; redo mode: the list index
    is the compact index i and the query is q_index[i]."""
from collections import namedtuple

import numpy as np

import flat_select_cases as FS

NO_LABEL, INF_BITS, FILLS = FS.NO_LABEL, FS.INF_BITS, FS.FILLS
INF_KEY = 0xFF800000
PAD = 5                                # dim = stride - PAD: the rows' zero padding is part of every distance


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16).view(np.float32)


def f32_key(f):
    """kth_bound_kernel: "the same as an order-preserving u32 key": (u & 0x80000000) ? ~u : (u | 0x80000000)"""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


# ---- ownership -------------------------------------------------------------------------------------------------------------
def gemm_tiles(n_rows, nrp, contig):
    """per partition the tiles it owns, in the order it walks them"""
    n_tiles = -(-n_rows // 128)
    if contig:
        t_base, t_rem = divmod(n_tiles, nrp)
        return [list(range(rp * t_base + min(rp, t_rem), rp * t_base + min(rp, t_rem) + t_base + (1 if rp < t_rem else 0))) for rp in range(nrp)]
    return [list(range(rp, n_tiles, nrp)) for rp in range(nrp)]


def gemm_owner(n_rows, nrp, contig, first_tile_only=False):
    """(list of every row = rp * 8 + slot, or -1; how many lists own it), by walking partitions, tiles and slots"""
    owner = np.full(n_rows, -1, np.int64)
    count = np.zeros(n_rows, np.int64)
    for rp, tiles in enumerate(gemm_tiles(n_rows, nrp, contig)):
        for t in (tiles[:1] if first_tile_only else tiles):
            for wave in range(4):
                for kk in range(2):
                    r = np.array([128 * t + 32 * wave + 8 * o + 4 * kk + i for o in range(4) for i in range(4)])
                    r = r[r < n_rows]
                    owner[r] = rp * 8 + wave * 2 + kk
                    count[r] += 1
    return owner, count


def scan_owner(n_alloc, row_begin, row_end, nrp, e):
    """(list of every row of the table, -1 outside the window; how many lists own it), by walking waves and tiles"""
    owner = np.full(n_alloc, -1, np.int64)
    count = np.zeros(n_alloc, np.int64)
    n_tiles = -(-(row_end - row_begin) // 16)
    for g in range(4 * nrp):
        for t in range(g, n_tiles, 4 * nrp):
            r = np.arange(row_begin + 16 * t, min(row_begin + 16 * t + 16, row_end))
            owner[r] = g if e > 1 else g // 4
            count[r] += 1
    return owner, count


# ---- selection per list ----------------------------------------------------------------------------------------------------
def ranking(dist, labels, eligible):
    """the eligible rows in (distance, label) order: select_model over all of them"""
    lab = np.where(eligible, labels, np.uint64(NO_LABEL))
    return FS.select_model(np.ascontiguousarray(dist), lab, dist.size)


def top_per_list(order, owner, n_lists, k):
    """[n_lists][k] rows (-1 = none): of the rows in `order` (ranked), the first k of every list"""
    l = owner[order]
    m = l >= 0
    order, l = order[m], l[m]
    o = np.argsort(l, kind="stable")
    order, l = order[o], l[o]
    start = np.searchsorted(l, np.arange(n_lists))
    pos = np.arange(l.size) - start[l]
    keep = pos < k
    out = np.full((n_lists, k), -1, np.int64)
    out[l[keep], pos[keep]] = order[keep]
    return out


def canon(d_bits, labels):
    """every list ordered by label (a list is a set: the kernels keep no order); real labels are distinct, empty slots equal"""
    o = np.argsort(labels, axis=-1, kind="stable")
    return np.take_along_axis(d_bits, o, -1), np.take_along_axis(labels, o, -1)


def lists_want(dist, labels, eligible, owner, n_lists, k):
    """the model's lists of one query, canonical: (distance bits [n_lists][k], labels [n_lists][k], rows [n_lists][k])"""
    rows = top_per_list(ranking(dist, labels, eligible), owner, n_lists, k)
    have = rows >= 0
    safe = np.where(have, rows, 0)
    d = np.where(have, dist.view(np.uint32)[safe], np.uint32(INF_BITS)).astype(np.uint32)
    l = np.where(have, labels[safe], np.uint64(NO_LABEL)).astype(np.uint64)
    return canon(d, l) + (rows,)


def merged(d_bits, labels, k):
    """all lists of one query merged by select_model: (distance bits, labels) of the answer"""
    d, l = d_bits.reshape(-1), labels.reshape(-1)
    o = FS.select_model(d.view(np.float32), l, k)
    return d[o], l[o]


# ---- data ------------------------------------------------------------------------------------------------------------------
# rows that hold one vector (three times as long as the others: the nearest of the even queries in either space)
GEMM_DUPS = [160 + o for o in (0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18)] + [164, 163 + 128, 163 + 256, 1500, 3000]
SCAN_DUPS = [64 + o for o in range(12)] + [80 + o for o in range(6)] + [96, 97, 112, 64 + 512, 1700, 2900]
_DATA = {}


class Data:
    """rows as the index holds them, padded queries, and table[q][row] = the oracle's distance, computed once"""

    def __init__(self, oracle, space, stride, bf16, n, nq, dups):
        dim = stride - PAD
        rng = np.random.default_rng([stride, int(bf16), n, nq, len(dups)])
        X = (rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(np.float32)
        self.dups = np.array([r for r in dups if r < n], np.int64)
        if self.dups.size:
            X[self.dups] = 3.0 * X[self.dups[0]]
        X = bf16_round(X) if bf16 else X
        near = np.where(np.arange(nq) % 2 == 0, self.dups[0] if self.dups.size else 0, rng.integers(0, n, nq))
        Q = np.zeros((nq, stride), np.float32)
        Q[:, :dim] = X[near] + (0.05 / np.sqrt(dim)) * rng.standard_normal((nq, dim)).astype(np.float32)
        self.space, self.stride, self.dim, self.bf16, self.n, self.nq, self.X, self.Q = space, stride, dim, bool(bf16), n, nq, X, Q
        o = oracle.Flat(dim, space, max_elements=n)
        o.add_many(X, np.arange(n, dtype=np.uint64))
        self.table = np.zeros((nq, n), np.float32)
        for q in range(nq):
            od, ol = o.search(Q[q, :dim], n)
            assert ol.size == n
            self.table[q, ol.astype(np.int64)] = od
            assert (np.diff(FS.order_key(od).astype(np.int64)) >= 0).all()      # (distance, label) order, as promised
        self.table_bits = self.table.view(np.uint32)

    def device_rows(self, n_alloc, slack, slack_kind):
        """[n_alloc + slack][stride] as the device holds them; the rows past n: zeros as in the product ("zeros"), or 1000 times
        the signs of query 0 ("large": finite, and nearer to query 0 than any row of the index)"""
        R = np.zeros((n_alloc + slack, self.stride), np.float32)
        R[:self.n, :self.dim] = self.X
        if slack_kind == "large":
            R[self.n:, :self.dim] = 1000.0 * np.where(self.Q[0, :self.dim] < 0, -1.0, 1.0).astype(np.float32)
        else:
            assert slack_kind == "zeros"
        return (R.view(np.uint32) >> 16).astype(np.uint16) if self.bf16 else R


def dataset(oracle, space, stride, bf16, n, nq, dups):
    key = (space, stride, bool(bf16), n, nq, tuple(dups))
    if key not in _DATA:
        if len(_DATA) > 40:
            _DATA.pop(next(iter(_DATA)))
        _DATA[key] = Data(oracle, space, stride, bf16, n, nq, dups)
    return _DATA[key]


def make_labels(kind, n, n_total, seed):
    """[n_total] labels, the first n the index's.  "small": a permutation of 5 .. n + 4; "spread": distinct over all 64 bits.
    The rows past n carry labels no row of the index has (0 .. 4 in turn; 2^40 + i), all of them allowed by every filter here."""
    rng = np.random.default_rng([n, seed, 77])
    lab = np.zeros(n_total, np.uint64)
    if kind == "small":
        lab[:n] = rng.permutation(n).astype(np.uint64) + np.uint64(5)
        lab[n:] = np.arange(n_total - n, dtype=np.uint64) % np.uint64(5)
    else:
        lab[:n] = FS.spread_labels(rng, n)
        lab[n:] = (np.uint64(1) << np.uint64(40)) + np.arange(n_total - n, dtype=np.uint64)
    return lab


def make_filter(labels, n, fraction, seed):
    """(bitmap, nbits, allowed [n]): nbits = n - 3, so eight labels of the index lie at or beyond it; labels 0 .. 4 allowed"""
    rng = np.random.default_rng([n, seed, int(fraction * 1000)])
    nbits = n - 3
    keep = labels[:n][rng.random(n) < fraction]
    keep = keep[keep < np.uint64(nbits)]
    bits = np.zeros((nbits + 63) // 64, np.uint64)
    for l in np.concatenate([keep, np.arange(5, dtype=np.uint64)]):
        bits[int(l) >> 6] |= np.uint64(1) << np.uint64(int(l) & 63)
    lab = labels[:n].astype(np.int64)
    inside = lab < nbits
    safe = np.where(inside, lab, 0)
    allowed = inside & (((bits[safe >> 6] >> (safe & 63).astype(np.uint64)) & np.uint64(1)) != 0)
    return bits, nbits, allowed


def kth_best(dist, labels, eligible, k):
    """the k-th best eligible distance (f32), +inf when fewer than k rows are eligible"""
    o = ranking(dist, labels, eligible)
    return np.float32(dist[o[k - 1]]) if o.size >= k else np.float32(np.inf)


def gemm_bound(kind, data, labels, allowed, k, nq):
    """init_bound as [2 * nq] words (floats, then keys as kth_bound_kernel documents), or None.
    "true": each query's k-th best allowed distance -- the tightest valid bound; "first1024": the k-th best of the first 1024
    rows -- what the product's pre-pass computes; "mixed": "true" for the even queries, +inf for the odd ones"""
    if kind is None:
        return None
    b = np.full(nq, np.inf, np.float32)
    for q in range(nq):
        if kind == "first1024":
            first = allowed & (np.arange(data.n) < 1024)
            b[q] = kth_best(data.table[q], labels[:data.n], first, k)
        elif kind == "true" or (kind == "mixed" and q % 2 == 0):
            b[q] = kth_best(data.table[q], labels[:data.n], allowed, k)
    return np.concatenate([b.view(np.uint32), f32_key(b)]).astype(np.uint32)


# ---- K4 cases --------------------------------------------------------------------------------------------------------------
GemmCase = namedtuple("GemmCase", "group stride tile_q bf16 n nq k nrp contig lockstep prepass bound filt slack labels cancel flag")
N_MAIN = 128 * 26 - 37               # 26 tiles over 8 partitions: blocks of 4 and 3 tiles, t_rem = 2, the last tile partial
TILE_Q = {64: 32, 128: 32, 192: 32, 1024: 24, 1536: 16}     # what flat_gemm_tile_q must answer (the GPU test asks it)


def gcase(group, stride=64, bf16=0, n=N_MAIN, nq=5, k=5, nrp=8, contig=1, lockstep=0, prepass=0, bound=None, filt=None, slack="large",
          labels="spread", cancel=0, flag=None):
    if filt is not None:
        labels = "small"
    return GemmCase(group, stride, TILE_Q[stride], bf16, n, nq, k, nrp, contig, lockstep, prepass, bound, filt, slack, labels, cancel, flag)


def gemm_cases():
    c = []
    for n in (N_MAIN, 128 * 8, 128 * 8 + 1, 300):
        for contig in (0, 1):
            for k in (5, 64):
                c.append(gcase("shapes", n=n, contig=contig, k=k))
    for contig in (0, 1):
        for k in (10, 11):
            c.append(gcase("shapes", n=128 * 5 - 10, nrp=16, contig=contig, k=k))
    i = 0
    for stride in (64, 128, 192, 1024, 1536):
        tq = TILE_Q[stride]
        for nq in (5, tq, tq + 3):
            for k in (10, 64):
                c.append(gcase("strides", stride=stride, nq=nq, k=k, n=N_MAIN if stride <= 192 else 1999, bf16=i % 2, contig=(i // 2) % 2))
                i += 1
    for nq in (35, 67):
        for lockstep in (0, 1, 2, 64):
            for contig in (0, 1):
                for k in (10, 64):
                    c.append(gcase("lockstep", nq=nq, lockstep=lockstep, contig=contig, k=k))
    for k in (1, 5, 10, 11, 64, 256):
        for bf16 in (0, 1):
            for prepass in (0, 1):
                c.append(gcase("kinds", k=k, bf16=bf16, prepass=prepass, contig=(k + bf16) % 2))
    for bound in (None, "true", "first1024", "mixed"):
        for k in (1, 10, 11, 64):
            for filt in (None, 0.5):
                c.append(gcase("bounds", nq=6, k=k, bound=bound, filt=filt, contig=1 if k in (1, 11) else 0))
    for filt in (0.5, 0.02):
        for k in (5, 10, 64, 256):
            for contig in (0, 1):
                c.append(gcase("filters", k=k, filt=filt, contig=contig, nq=6))
    for k in (10, 64):
        for contig in (0, 1):
            c.append(gcase("filters", k=k, contig=contig, slack="zeros", nq=6))
    for k in (5, 10):
        for contig in (0, 1):
            for nq, lockstep in ((5, 0), (35, 2)):
                c.append(gcase("control", k=k, contig=contig, nq=nq, lockstep=lockstep, cancel=1))
    c.append(gcase("control", k=64, cancel=1))
    c.append(gcase("control", k=11, contig=0, cancel=1))
    for flag in ((5, 4, 0), (0, 1, 8), (9, 1, 8), (5, 5, 0), (3, 1, 8)):
        c.append(gcase("control", k=5, flag=flag))
    return c


def flag_runs(flag):
    """launch_skipped of device_common.hpp, negated: *run_flag == run_if, or with run_hi != 0 run_if <= *run_flag <= run_hi"""
    if flag is None:
        return True
    v, run_if, run_hi = flag
    return run_if <= v <= run_hi if run_hi else v == run_if


# ---- K3 cases --------------------------------------------------------------------------------------------------------------
ScanCase = namedtuple("ScanCase", "group l2 bf16 stride qb e k nq nrp row_begin row_len filt lb redo cancel flag")
N_SCAN = 3300
SCAN_NQ = 16                         # queries of the one data set every K3 case draws from
Q_INDEX = [3, 1, 3, 7, 0, 2, 6, 5]   # a permutation of 0 .. 7 with 3 in place of 4
REDO_FLAG = (1, 8)                   # run_if, run_hi: the word is *nq_dev itself, as FlatIndex::scan_k3 passes it
VARIANTS = ([(qb, 1, k) for qb in (1, 2, 4, 8) for k in (1, 10, 64)] + [(qb, 4, k) for qb in (1, 2) for k in (65, 256)]
            + [(1, 16, 257), (1, 16, 1024)])


def scase(group, qb, e, k, l2=0, bf16=0, stride=64, nq=None, nrp=8, row_begin=0, row_len=3000, filt=None, lb=None, redo=None, cancel=None,
          flag=None):
    return ScanCase(group, l2, bf16, stride, qb, e, k, 2 * qb if nq is None else nq, nrp, row_begin, row_len, filt, lb, redo, cancel, flag)


def scan_cases():
    c = []
    for qb, e, k in VARIANTS:
        for l2 in (0, 1):
            for bf16 in (0, 1):
                c.append(scase("variants", qb, e, k, l2=l2, bf16=bf16, stride=192 if (qb + k) % 2 else 64, row_len=N_SCAN))
    for i, (qb, e, k, nq) in enumerate([(8, 1, 10, 3), (8, 1, 10, 9), (8, 1, 64, 13), (4, 1, 10, 1), (4, 1, 1, 5), (2, 4, 65, 1), (2, 4, 256, 3),
                                        (2, 1, 10, 1)]):
        c.append(scase("nq", qb, e, k, nq=nq, l2=i % 2, bf16=(i // 2) % 2))
    for stride in (64, 192, 576):
        for qb, e, k in ((1, 1, 10), (8, 1, 10)):
            for l2 in (0, 1):
                for bf16 in (0, 1):
                    c.append(scase("strides", qb, e, k, l2=l2, bf16=bf16, stride=stride, row_len=1500))
    for nrp in (8, 16):
        for row_len in (1, 15, 16, 17, 64 * nrp - 1, 64 * nrp + 1, 3000):
            for row_begin in (0, 37):
                for qb, e, k in ((4, 1, 10), (2, 4, 65)):
                    c.append(scase("windows", qb, e, k, nrp=nrp, row_begin=row_begin, row_len=row_len, l2=(row_len + row_begin) % 2))
    for qb, e, k in ((4, 1, 10), (2, 4, 65), (1, 16, 257)):
        for l2 in (0, 1):
            c.append(scase("filters", qb, e, k, l2=l2, bf16=l2, filt=0.5, row_begin=37))
    for k in (100, 1024):
        for l2, bf16 in ((0, 0), (1, 1)):
            for filt in (None, 0.5):
                c.append(scase("paged", 1, 16, k, l2=l2, bf16=bf16, filt=filt, lb=5, nq=4, row_len=N_SCAN))
    for qb, e, k in ((8, 1, 10), (4, 1, 10), (1, 1, 10), (2, 4, 65), (1, 16, 257)):
        for nq_dev in (0, 1, 3, 8):
            c.append(scase("redo", qb, e, k, nq=8, redo=nq_dev, flag="nq_dev", l2=nq_dev % 2))
    for qb, e, k in ((4, 1, 10), (2, 4, 65), (1, 16, 257)):
        c.append(scase("control", qb, e, k, cancel=1))
        c.append(scase("control", qb, e, k, cancel=0))
    for flag in ((5, 4, 0), (0, 1, 8), (9, 1, 8), (5, 5, 0), (3, 1, 8)):
        c.append(scase("control", 4, 1, 10, flag=flag))
        c.append(scase("control", 2, 4, 65, flag=flag))
    return c


def scan_runs(case):
    if case.flag == "nq_dev":
        return flag_runs((case.redo,) + REDO_FLAG)
    return flag_runs(case.flag)


def scan_setup(case, data, labels, allowed):
    """(owner [n], n_lists, eligible [nq][n], lb_dist, lb_label): which rows each query may rank -- inside the window, allowed, and
    with lb strictly beyond (lb_dist[q], lb_label[q]) = entry `lb` of the query's full ranking of the allowed rows"""
    owner, _count = scan_owner(data.n, case.row_begin, case.row_begin + case.row_len, case.nrp, case.e)
    n_lists = case.nrp * (1 if case.e == 1 else 4)
    elig = np.tile((owner >= 0) & allowed, (case.nq, 1))
    lb_d = lb_l = None
    if case.lb is not None:
        lb_d, lb_l = np.zeros(case.nq, np.float32), np.zeros(case.nq, np.uint64)
        for q in range(case.nq):
            o = ranking(data.table[q], labels[:data.n], elig[q])
            lb_d[q], lb_l[q] = data.table[q, o[case.lb]], labels[o[case.lb]]
            elig[q, o[:case.lb + 1]] = False
    return owner, n_lists, elig, lb_d, lb_l
