"""The selection kernels of csrc/flat_scan.hip on their own, through tests/helpers/flat_select_probe.hip -- a small library
that includes that translation unit, so the product's kernels and launchers run: the fused re-rank (flat_rerank_kernel),
the list-mode scan (flat_scan_kernel<.., kIdx = true>), merge_select_kernel, merge_topk_kernel<1|4|16>, K8
(gather_distance_kernel), kth_bound_kernel and fill_empty_kernel.

Every comparison is an equality of bits or of integer counts (one is an inequality of integer counts: the number of rows
the second bound may still re-rank).  Exact distances are the oracle's distance of the same row and query.  Selection is
one numpy statement (tests/helpers/flat_select_cases.py, select_model):

    real entries = label != kNoLabel, ordered by (float value with -0 == +0, label), n = min(k, real)
    out_n == n, out[:n] == those entries in that order with the INPUT's distance bits, out[n:out_ld] == (+inf, kNoLabel)

Every case runs from output and workspace buffers filled with 0x00000000, 0xFFFFFFFF and 0x7F7FFFFF, and every word handed
back is either what the model says or, where the contract says "not written" (a query in ovf_q, a skipped launch, a compact
index >= *nq_dev, the partial lists of a query one block serves), still the pattern.  One buffer is held to less: with the
second bound on, nothing says which rows of a slice the bound drops, so a partial list of an eight-block query is checked to
hold allowed survivors of its own slice with their exact distance bits and (+inf, kNoLabel) in every other slot, and no more;
with the bound off it is the model's list word for word.  The final answer is the model's in both cases.

tests/test_flat_select_model_cpu.py pins the model to Python's sorted and counts that the inputs here reach the paths they are
meant for: the sample's fast and general path of the selection, U = 0xFFFFFFFF, exactly 256 and 257 survivors; the re-rank's
list in registers, walked by one block, walked by eight, and flush() inside a walk.

The second bound.  Scores and margins are the float64 model of tests/test_flat_filter_stages_gpu.py (Case.ref, margins):
score = x . q (L2: x . q - |x|^2 / 2), margin = c2 R^2 + c1 R + c0 at the tile's norm R.  A survivor's score is moved by
u * margin, |u| <= 0.99.  The remaining hundredth of the margin is at least 8e-5 (c0 = c1 = 4e-3, R about 1) and covers what
separates the float64 score from the f32 distance the kernel ranks by: 16 lanes of D / 16 fused multiply-adds and a four-level
tree, at most (D / 16 + 5) 2^-24 sum|x_i q_i| (L2: |x - q|^2 / 2) <= 65 * 6e-8 * 4 = 1.6e-5 at D = 960, plus the rounding of
score, margin and 1 - dot to f32 (2^-24 each, of values near 1).  The pruning case uses u = 0 and c0 = c1 = 2e-4: the whole
margin, 4e-4, covers the same 1.6e-5."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "helpers"
CSRC = ROOT / "valkey-search_amd" / "csrc"
LIB = HERE / "libflatselectprobe.so"
sys.path.insert(0, str(HERE))
import flat_select_cases as FS  # noqa: E402

NO_LABEL, INF_BITS, FILLS = FS.NO_LABEL, FS.INF_BITS, FS.FILLS
u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p


def build_probe():
    src = HERE / "flat_select_probe.hip"
    newest = max(p.stat().st_mtime for p in (src, CSRC / "flat_scan.hip", CSRC / "kernels.hpp", CSRC / "device_common.hpp"))
    if not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", "-I", str(CSRC), str(src),
                               "-o", str(LIB)])
    return LIB


class MergeIO(C.Structure):
    _fields_ = ([("in_dist", vp), ("in_label", vp), ("in_entries", u64), ("part_stride", u64), ("q_stride", u64)]
                + [(n, u32) for n in ("parts", "per_part", "nq", "k", "e", "out_ld")] + [("ovf_q", vp), ("q_index", vp)]
                + [(n, u32) for n in ("nq_dev", "use_flag", "flag_value", "run_if", "run_hi", "direct_topk1", "fill")]
                + [(n, vp) for n in ("out_dist", "out_label", "out_n", "redo_cnt", "redo_list")])


class RerankIO(C.Structure):
    _fields_ = ([(n, vp) for n in ("rows", "labels", "queries", "list_begin", "list_row", "list_val", "qcoef", "tile_norm", "allow_bits")]
                + [("allow_nbits", u64), ("ovf_q", vp)]
                + [(n, u32) for n in ("n_rows", "stride", "bf16", "l2", "nq", "k", "out_ld", "cand_cap", "n_tiles", "prune", "fused", "fill")]
                + [(n, vp) for n in ("out_dist", "out_label", "out_n", "reranked", "done_cnt", "redo_cnt", "redo_list", "part_dist", "part_label",
                                     "qchunk")])


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def rc_text(name, rc):
    return "%s refused its arguments" % name if rc == 1 else "%s: HIP error seen at flat_select_probe.hip:%d" % (name, rc)


class Out:
    pass


class Probe:
    def __init__(self):
        lib = C.CDLL(str(build_probe()))
        lib.fs_probe_merge.argtypes = [C.POINTER(MergeIO)]
        lib.fs_probe_rerank.argtypes = [C.POINTER(RerankIO)]
        lib.fs_probe_per_q.argtypes = [u32]
        lib.fs_probe_per_q.restype = u32
        lib.fs_probe_gather.argtypes = [vp, u32, u32, u32, u32, vp, vp, u32, u32, u32, vp]
        lib.fs_probe_kth_bound.argtypes = [vp, vp, u32, u32, u32, vp]
        lib.fs_probe_fill_empty.argtypes = [u32, u32, u32, u32, vp, vp, vp]
        for f in (lib.fs_probe_merge, lib.fs_probe_rerank, lib.fs_probe_gather, lib.fs_probe_kth_bound, lib.fs_probe_fill_empty):
            f.restype = C.c_int
        self.lib = lib

    def merge(self, in_d, in_l, parts, per_part, part_stride, q_stride, nq, k, e, out_ld, fill, *, direct=False, ovf=None, q_index=None,
              nq_dev=0, flag=None, expect_rc=0):
        ld = max(out_ld, k)
        o = Out()
        o.dist = np.zeros((nq, ld), np.uint32)
        o.label = np.zeros((nq, ld), np.uint64)
        o.n = np.zeros(nq, np.uint32)
        o.redo_cnt = np.zeros(1, np.uint32)
        o.redo_list = np.zeros(nq, np.uint32)
        use_flag, flag_value, run_if, run_hi = (0, 0, 0, 0) if flag is None else (1, *flag)
        io = MergeIO(ptr(in_d), ptr(in_l), in_d.size, part_stride, q_stride, parts, per_part, nq, k, e, out_ld, ptr(ovf), ptr(q_index), nq_dev,
                     use_flag, flag_value, run_if, run_hi, 1 if direct else 0, fill, ptr(o.dist), ptr(o.label), ptr(o.n), ptr(o.redo_cnt),
                     ptr(o.redo_list))
        rc = self.lib.fs_probe_merge(C.byref(io))
        assert rc == expect_rc, rc_text("fs_probe_merge", rc)
        return o

    def rerank(self, data, lists, vals, *, k, out_ld, cap, fused, prune, fill, qcoef=None, tile_norm=None, allow=None, nbits=0, ovf=None):
        nq = len(lists)
        per_q = self.lib.fs_probe_per_q(k)
        ld = max(out_ld, k)
        begin = np.zeros(nq + 1, np.uint32)
        begin[1:] = np.cumsum([l.size for l in lists])
        rows = np.ascontiguousarray(np.concatenate(lists), np.uint32) if begin[nq] else np.zeros(1, np.uint32)
        val = np.ascontiguousarray(np.concatenate(vals), np.float32) if begin[nq] else np.zeros(1, np.float32)
        n_tiles = (data.n + 127) // 128
        qcoef = np.zeros((nq, 4), np.float32) if qcoef is None else np.ascontiguousarray(qcoef, np.float32)
        tile_norm = np.zeros(n_tiles, np.uint32) if tile_norm is None else np.ascontiguousarray(tile_norm, np.float32).view(np.uint32)
        assert tile_norm.size == n_tiles and qcoef.shape == (nq, 4)
        o = Out()
        o.dist = np.zeros((nq, ld), np.uint32)
        o.label = np.zeros((nq, ld), np.uint64)
        o.n, o.reranked, o.done, o.redo_list = (np.zeros(nq, np.uint32) for _ in range(4))
        o.redo_cnt = np.zeros(1, np.uint32)
        o.part_d = np.zeros((nq, per_q), np.uint32)
        o.part_l = np.zeros((nq, per_q), np.uint64)
        o.qchunk = np.zeros((nq, FS.SPILL_PER_QUERY), np.uint32)
        io = RerankIO(ptr(data.dev_rows), ptr(data.labels), ptr(data.Q[:nq]), ptr(begin), ptr(rows), ptr(val), ptr(qcoef), ptr(tile_norm), ptr(allow),
                      nbits, ptr(ovf), data.n, data.D, int(data.bf16), int(data.l2), nq, k, out_ld, cap, n_tiles, int(prune), int(fused), fill,
                      ptr(o.dist), ptr(o.label), ptr(o.n), ptr(o.reranked), ptr(o.done), ptr(o.redo_cnt), ptr(o.redo_list), ptr(o.part_d),
                      ptr(o.part_l), ptr(o.qchunk))
        rc = self.lib.fs_probe_rerank(C.byref(io))
        assert rc == 0, rc_text("fs_probe_rerank", rc)
        return o


@pytest.fixture(scope="module")
def probe():
    return Probe()


def fill64(fill):
    return np.uint64(fill | (fill << 32))


def expected_rows(dist, label, k, ld):
    """the model's output row: (distance bits [ld], labels [ld], n)"""
    o = FS.select_model(dist, label, k)
    d = np.full(ld, INF_BITS, np.uint32)
    l = np.full(ld, NO_LABEL, np.uint64)
    d[:o.size] = dist[o].view(np.uint32)
    l[:o.size] = label[o]
    return d, l, o.size


def compare_outputs(o, want, written, fill, what):
    """want: per output query (dist bits, labels, n) or None; written[q] False: the row still holds the pattern"""
    nq, ld = o.dist.shape
    for q in range(nq):
        if written[q]:
            wd, wl, wn = want[q]
            assert int(o.n[q]) == wn, "%s: out_n[%d] = %d, the model has %d" % (what, q, int(o.n[q]), wn)
            bad = np.flatnonzero((o.dist[q] != wd) | (o.label[q] != wl))
            assert bad.size == 0, "%s: query %d, place %d: (%#x, %#x), the model has (%#x, %#x)" % (
                what, q, bad[0], o.dist[q][bad[0]], o.label[q][bad[0]], wd[bad[0]], wl[bad[0]])
        else:
            assert int(o.n[q]) == fill and (o.dist[q] == fill).all() and (o.label[q] == fill64(fill)).all(), \
                "%s: query %d is not this launch's to write, and a word of its output changed" % (what, q)


# ---- the merges ------------------------------------------------------------------------------------------------------------
GAP_DIST, GAP_LABEL = np.float32(-3e38), np.uint64(7)     # what lies between the lists: it would win every selection


def lay_out(queries, parts, per_part, part_stride, q_stride):
    """entry e of query q = (part e // per_part, i = e % per_part) at part * part_stride + q * q_stride + i"""
    nq = len(queries)
    size = (parts - 1) * part_stride + (nq - 1) * q_stride + per_part if nq else 1
    in_d = np.full(size, GAP_DIST, np.float32)
    in_l = np.full(size, GAP_LABEL, np.uint64)
    e = np.arange(parts * per_part)
    at = (e // per_part) * part_stride + e % per_part
    for q, (_name, d, lab) in enumerate(queries):
        in_d[at + q * q_stride] = d
        in_l[at + q * q_stride] = lab
    return in_d, in_l


_WANT = {}


def merge_want(total, k, seed, placements, ld):
    key = (total, k, seed, placements)
    if key not in _WANT:
        qs = FS.merge_queries(total, k, seed, placements)
        _WANT[key] = (qs, [FS.select_model(d, lab, k) for _n, d, lab in qs])
        if len(_WANT) > 64:
            _WANT.pop(next(iter(_WANT)))
    qs, orders = _WANT[key]
    want = []
    for (_n, d, lab), o in zip(qs, orders):
        wd = np.full(ld, INF_BITS, np.uint32)
        wl = np.full(ld, NO_LABEL, np.uint64)
        wd[:o.size] = d[o].view(np.uint32)
        wl[:o.size] = lab[o]
        want.append((wd, wl, o.size))
    return qs, want


def general_layout(total, nq):
    """lists further apart than they are long; in four parts where the total divides"""
    if total % 4 == 0:
        per = total // 4
        return 4, per, nq * (per + 3) + 11, per + 3
    return 1, total, 0, total + 5


@pytest.mark.parametrize("total", FS.SELECT_TOTALS)
def test_merge_by_selection(probe, total):
    """launch_merge_topk with e = 1 and at most 4096 entries (merge_select_kernel), and merge_topk_kernel<1> on the same input"""
    for k in FS.SELECT_KS:
        for out_ld in (k, k + 3, 128):
            qs, want = merge_want(total, k, 0, True, max(out_ld, k))
            nq = len(qs)
            for layout in ("one_part", "general"):
                parts, per_part, part_stride, q_stride = (1, total, 0, total) if layout == "one_part" else general_layout(total, nq)
                in_d, in_l = lay_out(qs, parts, per_part, part_stride, q_stride)
                for fill in FILLS:
                    for direct in (False, True):
                        o = probe.merge(in_d, in_l, parts, per_part, part_stride, q_stride, nq, k, 1, out_ld, fill, direct=direct)
                        what = "total %d k %d out_ld %d %s fill %#x %s [%s]" % (total, k, out_ld, layout, fill, "merge_topk<1>" if direct else "select",
                                                                                 " ".join(n for n, _d, _l in qs))
                        compare_outputs(o, want, [True] * nq, fill, what)
                        assert int(o.redo_cnt[0]) == 0 and (o.redo_list == fill).all(), what


@pytest.mark.parametrize("parts", [2, 8])
def test_merge_shard_layout(probe, parts):
    """the layout of vk_merge_topk_device: per_part = k, part_stride = nq k, the lists of a shard's queries back to back"""
    for k in FS.SELECT_KS:
        total = parts * k
        for out_ld in (k, k + 3, 128):
            qs, want = merge_want(total, k, 1, True, max(out_ld, k))
            nq = len(qs)
            in_d, in_l = lay_out(qs, parts, k, nq * k, k)
            assert in_d.size == parts * nq * k
            for fill in FILLS:
                for direct in (False, True):
                    o = probe.merge(in_d, in_l, parts, k, nq * k, k, nq, k, 1, out_ld, fill, direct=direct)
                    compare_outputs(o, want, [True] * nq, fill, "shards %d k %d out_ld %d fill %#x direct %d" % (parts, k, out_ld, fill, direct))


INSERT_CASES = [(1, 10), (1, 64), (4, 65), (4, 256), (16, 257), (16, 1024)]


@pytest.mark.parametrize("e,k", INSERT_CASES)
def test_merge_by_insertion(probe, e, k):
    """merge_topk_kernel<1> behind the launcher (more than 4096 entries), <4> and <16>"""
    shapes = [(parts, per) for parts in (1, 3, 8) for per in (k, 1023, 1024, 1025, 2500)]
    if e == 1:
        shapes = [(p, per) for p, per in shapes if p * per > FS.SEL_MAX] + [(1, 4097), (1, 5000), (2, 2500)]
    for i, (parts, per_part) in enumerate(shapes):
        total = parts * per_part
        out_ld = (k, k + 3, max(128, k + 64))[i % 3]
        qs, want = merge_want(total, k, 2, False, max(out_ld, k))
        nq = len(qs)
        q_stride = per_part + (5 if i % 2 else 0)
        part_stride = nq * q_stride + (3 if i % 2 else 0)
        in_d, in_l = lay_out(qs, parts, per_part, part_stride, q_stride)
        for fill in FILLS:
            o = probe.merge(in_d, in_l, parts, per_part, part_stride, q_stride, nq, k, e, out_ld, fill)
            compare_outputs(o, want, [True] * nq, fill, "e %d k %d parts %d per_part %d out_ld %d fill %#x" % (e, k, parts, per_part, out_ld, fill))


# (e, k, total): the selection, merge_topk_kernel<1> behind the launcher, <4>
CONTROL_SHAPES = [(1, 10, 1024), (1, 10, 4100), (4, 100, 1024)]


@pytest.mark.parametrize("e,k,total", CONTROL_SHAPES)
def test_merge_control_paths(probe, e, k, total):
    nq = 9
    ld = k + 3
    qs, want = merge_want(total, k, 3, total <= FS.SEL_MAX, ld)
    qs, want = (qs * 2)[:nq], (want * 2)[:nq]
    assert len(qs) == nq
    in_d, in_l = lay_out(qs, 1, total, 0, total)
    directs = (False, True) if e == 1 and total <= FS.SEL_MAX else (False,)
    for fill in FILLS:
        for direct in directs:
            args = (in_d, in_l, 1, total, 0, total, nq, k, e, ld, fill)
            what = "e %d k %d total %d fill %#x direct %d: " % (e, k, total, fill, direct)
            # queries the filter handed over: listed once each, counted, their outputs untouched
            ovf = np.array([0, 1, 0, 0, 7, 0, 1, 0, 1], np.uint32)
            o = probe.merge(*args, direct=direct, ovf=ovf)
            compare_outputs(o, want, ovf == 0, fill, what + "ovf_q")
            n_ovf = int((ovf != 0).sum())
            assert int(o.redo_cnt[0]) == n_ovf, what + "redo_cnt"
            assert sorted(o.redo_list[:n_ovf].tolist()) == np.flatnonzero(ovf).tolist() and (o.redo_list[n_ovf:] == fill).all(), what + "redo_list"
            # redo mode: lists at the compact index, outputs at q_index, nothing behind *nq_dev
            q_index = np.array([4, 8, 0, 6, 2, 1, 3, 5, 7], np.uint32)
            for nq_dev in (0, 4, 9):
                o = probe.merge(*args, direct=direct, q_index=q_index, nq_dev=nq_dev)
                w2, written = [None] * nq, [False] * nq
                for i in range(nq_dev):
                    w2[q_index[i]], written[q_index[i]] = want[i], True
                compare_outputs(o, w2, written, fill, what + "redo mode, %d queries" % nq_dev)
            # ... with a handed-over query among them (ovf_q is indexed by the query, not by the compact index)
            ovf = np.zeros(nq, np.uint32)
            ovf[[8, 2]] = 1
            o = probe.merge(*args, direct=direct, q_index=q_index, nq_dev=4, ovf=ovf)
            w2, written = [None] * nq, [False] * nq
            for i in (0, 2, 3):
                w2[q_index[i]], written[q_index[i]] = want[i], True
            compare_outputs(o, w2, written, fill, what + "redo mode with ovf_q")
            assert int(o.redo_cnt[0]) == 1 and int(o.redo_list[0]) == 8 and (o.redo_list[1:] == fill).all(), what + "redo mode with ovf_q"
            # the device-side conditional launch: (word, run_if, run_hi); run_hi == 0 is the equality form
            for flag, runs in (((5, 4, 0), False), ((0, 1, 0), False), ((3, 4, 9), False), ((10, 4, 9), False), ((5, 5, 0), True),
                               ((4, 4, 9), True), ((9, 4, 9), True)):
                o = probe.merge(*args, direct=direct, flag=flag, ovf=np.ones(nq, np.uint32) if not runs else None)
                compare_outputs(o, want, [runs] * nq, fill, what + "run_flag %r" % (flag,))
                assert int(o.redo_cnt[0]) == 0 and (o.redo_list == fill).all(), what + "run_flag %r: the redo list" % (flag,)
        # no query at all; and an input of no entries is refused
        o = probe.merge(in_d, in_l, 1, total, 0, total, 0, k, e, ld, fill)
        assert o.dist.size == 0 and int(o.redo_cnt[0]) == 0
        probe.merge(in_d, in_l, 0, total, 0, total, nq, k, e, ld, fill, expect_rc=1)
        probe.merge(in_d, in_l, 1, 0, 0, total, nq, k, e, ld, fill, expect_rc=1)


# ---- the re-rank -----------------------------------------------------------------------------------------------------------
def bf16_value(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32) << 16).view(np.float32)


N_DUP = 40
_DATA = {}


class Data:
    """rows (the values the index holds), labels, queries, and per query the oracle's distance of every row, computed once"""

    def __init__(self, oracle, D, bf16, l2, n, nq):
        rng = np.random.default_rng([D, int(bf16), int(l2), n])
        X = (rng.standard_normal((n, D)) / np.sqrt(D)).astype(np.float32)
        self.dup = np.sort(rng.choice(n, N_DUP, replace=False))          # one vector under N_DUP labels, all over the index
        X[self.dup] = X[self.dup[0]]
        self.X = bf16_value(X) if bf16 else X
        self.dev_rows = (self.X.view(np.uint32) >> 16).astype(np.uint16) if bf16 else self.X
        # labels: a permutation of 5 .. n + 4; nbits = n + 4 puts one label AT nbits (never allowed) and one at nbits - 1 --
        # both on copies of the duplicated vector, so both rows are among the nearest of the queries next to it
        lab = rng.permutation(n).astype(np.uint64) + np.uint64(5)
        self.nbits = n + 4
        for want, row in ((self.nbits, self.dup[1]), (self.nbits - 1, self.dup[2])):
            other = int(np.flatnonzero(lab == np.uint64(want))[0])
            lab[other], lab[row] = lab[row], lab[other]
        self.labels = lab
        # queries: even ones next to the duplicated vector (ties at the k-th distance), odd ones next to some row
        near = np.where(np.arange(nq) % 2 == 0, self.dup[0], rng.integers(0, n, nq))
        self.Q = np.ascontiguousarray(self.X[near] + (0.05 / np.sqrt(D)) * rng.standard_normal((nq, D)), np.float32)
        self.D, self.bf16, self.l2, self.n, self.nq = D, bf16, l2, n, nq
        metric = "L2" if l2 else "IP"
        self.table = np.zeros((nq, n), np.float32)
        for q in range(nq):
            od, ol = oracle.prefilter_topk(metric, self.Q[q], self.X, np.arange(n, dtype=np.uint64), n)
            assert ol.size == n
            self.table[q, ol.astype(np.int64)] = od
            for r in (0, int(self.dup[3]), n - 1):                          # ... which is the oracle's distance function, row by row
                assert self.table[q, r].view(np.uint32) == oracle.distance(metric, self.X[r], self.Q[q]).view(np.uint32)
        Xd, Qd = self.X.astype(np.float64), self.Q.astype(np.float64)
        n2 = (Xd * Xd).sum(1)
        self.S = (Xd @ Qd.T - (0.5 * n2[:, None] if l2 else 0.0)).T              # [nq][n] exact scores, accumulator space (Case.ref)
        norm = np.sqrt(n2)
        pad = np.concatenate([norm, np.zeros((-n) % 128)]).reshape(-1, 128).max(1)
        self.tile_norm = np.nextafter((pad * (1 + 1e-6)).astype(np.float32), np.float32(np.inf))   # >= every norm of the tile
        assert (self.tile_norm.astype(np.float64)[np.arange(n) >> 7] >= norm).all()

    def allowed(self, allow):
        """per row: does the bitmap (by label) let it through -- allow_bit() of device_common.hpp"""
        if allow is None:
            return np.ones(self.n, bool)
        lab = self.labels.astype(np.int64)
        ok = lab < self.nbits
        bit = (allow[np.minimum(lab, self.nbits - 1) >> 6] >> (np.minimum(lab, self.nbits - 1) & 63).astype(np.uint64)) & np.uint64(1)
        return ok & (bit != 0)

    def want(self, q, rows, allow_rows, k, ld):
        lab = np.where(allow_rows[rows], self.labels[rows], np.uint64(NO_LABEL))
        return expected_rows(np.ascontiguousarray(self.table[q, rows]), lab, k, ld)

    def margin(self, coef, rows, tile_norm=None):
        """the float64 model of filter_margin (tests/test_flat_filter_stages_gpu.py, margins) at the rows' tile norms"""
        R = (self.tile_norm if tile_norm is None else tile_norm).astype(np.float64)[rows >> 7]
        c = np.asarray(coef, np.float64)
        with np.errstate(all="ignore"):
            return (c[0] * R * R if self.l2 else 0.0) + c[1] * R + c[2]


def dataset(oracle, D, bf16, l2, n, nq):
    key = (D, bf16, l2, n, nq)
    if key not in _DATA:
        _DATA[key] = Data(oracle, D, bf16, l2, n, nq)
        if len(_DATA) > 3:
            _DATA.pop(next(iter(_DATA)))
    return _DATA[key]


def make_lists(data, counts, rng):
    """per query a list of `count` distinct row slots; the copies of the duplicated vector spread evenly through it"""
    lists = []
    for q, c in enumerate(counts):
        rows = rng.permutation(data.n)[:c].astype(np.uint32)
        if c >= 2 * N_DUP:
            rest = rows[~np.isin(rows, data.dup)][:c - N_DUP]
            at = np.linspace(0, c - 1, N_DUP).astype(np.int64)
            rows = np.empty(c, np.uint32)
            rows[at] = data.dup
            rows[np.setdiff1d(np.arange(c), at)] = rest
        elif c >= 4:                                   # a short list: a few of the copies, next to each other
            rows[:min(c, 6)] = data.dup[:min(c, 6)]
            rows = rows[np.sort(np.unique(rows, return_index=True)[1])]
            extra = np.setdiff1d(np.arange(data.n), rows)[:c - rows.size].astype(np.uint32)
            rows = np.concatenate([rows, extra])
        assert rows.size == c and np.unique(rows).size == c
        lists.append(rows)
    return lists


COEF, COEF_SMALL = (1e-3, 4e-3, 4e-3, 0.0), (1e-4, 2e-4, 2e-4, 0.0)


def scores(data, lists, mode, rng, top_rows=None, coef=COEF, tile_norm=None):
    """the survivors' approximate scores: the exact score moved inside the margin"""
    vals = []
    for q, rows in enumerate(lists):
        s, m = data.S[q, rows], data.margin(coef, rows.astype(np.int64), tile_norm)
        if mode == "exact":
            u = np.zeros(rows.size)
        elif mode == "adversarial":                    # the answer's rows look as bad as they may, all others as good
            u = np.where(np.isin(rows, top_rows[q]), -0.99, 0.99)
        else:
            u = rng.uniform(-0.99, 0.99, rows.size)
        with np.errstate(all="ignore"):
            v = (s + u * np.where(np.isfinite(m), m, 0.0)).astype(np.float32)
        if mode == "nan":
            v[rng.random(rows.size) < 0.3] = np.float32(np.nan)
        vals.append(v)
    return vals


def part_slices(n, fused, e):
    """which list entries feed which partial list: [n_lists] index arrays"""
    i = np.arange(n)
    if fused:      # a contiguous slice per wave, four waves per block: part p = entries [4 p per, (4 p + 4) per)
        per = -(-n // 32) if n else 1
        owner = i // (4 * per)
        return [i[owner == p] for p in range(8)]
    tile_wave = (i // 16) % 32                         # list mode: tile t goes to wave t % 32 of the query's eight blocks
    if e == 1:
        return [i[tile_wave // 4 == p] for p in range(8)]
    return [i[tile_wave == w] for w in range(32)]


def check_rerank(data, o, lists, allow_rows, *, k, out_ld, cap, fused, prune, fill, ovf, what):
    nq, ld = len(lists), max(out_ld, k)
    ovf = np.zeros(nq, np.uint32) if ovf is None else ovf
    want = [data.want(q, lists[q].astype(np.int64), allow_rows, k, ld) for q in range(nq)]
    compare_outputs(o, want, ovf == 0, fill, what)
    n_ovf = int((ovf != 0).sum())
    assert int(o.redo_cnt[0]) == n_ovf, what + ": redo_cnt"
    assert sorted(o.redo_list[:n_ovf].tolist()) == np.flatnonzero(ovf).tolist() and (o.redo_list[n_ovf:] == fill).all(), what + ": redo list"
    e = 1 if k <= 64 else 4 if k <= 256 else 16
    n_lists = 8 if e == 1 else 32
    pd, pl = o.part_d.reshape(nq, n_lists, k), o.part_l.reshape(nq, n_lists, k)
    for q in range(nq):
        n = lists[q].size
        path = FS.rerank_path(n, cap, prune)[0]
        if fused:
            assert int(o.done[q]) == (8 if path == "blocks" and not ovf[q] else 0), "%s: done_cnt[%d] = %d (%s)" % (what, q, int(o.done[q]), path)
            if not prune and not ovf[q]:
                assert int(o.reranked[q]) == n, "%s: reranked[%d] = %d of %d" % (what, q, int(o.reranked[q]), n)
            assert int(o.reranked[q]) <= (0 if ovf[q] else n)
        else:
            assert int(o.done[q]) == 0 and int(o.reranked[q]) == 0, what + ": a fused kernel's word changed"
        if fused and (path != "blocks" or ovf[q]):     # one block, or none: no partial list is written
            assert (pd[q] == fill).all() and (pl[q] == fill64(fill)).all(), "%s: query %d, a partial list was written" % (what, q)
            continue
        rows = lists[q].astype(np.int64)
        for p, sl in enumerate(part_slices(0 if ovf[q] else n, fused, e)):
            wd, wl, wn = data.want(q, rows[sl], allow_rows, k, k)
            got_real = pl[q, p] != np.uint64(NO_LABEL)
            assert (pd[q, p][~got_real] == INF_BITS).all(), "%s: query %d list %d: an empty slot is not (+inf, kNoLabel)" % (what, q, p)
            go = np.argsort(pl[q, p][got_real])
            if not prune:
                wo = np.argsort(wl[:wn])
                assert (pl[q, p][got_real][go] == wl[:wn][wo]).all() if int(got_real.sum()) == wn else False, \
                    "%s: query %d list %d holds %d entries, the model %d, or other labels" % (what, q, p, int(got_real.sum()), wn)
                assert (pd[q, p][got_real][go] == wd[:wn][wo]).all(), "%s: query %d list %d: distance bits" % (what, q, p)
            else:   # pruned by the second bound: every entry is an allowed survivor of the slice with its exact distance
                lab_of = {int(data.labels[r]): data.table[q, r].view(np.uint32) for r in rows[sl][allow_rows[rows[sl]]]}
                for d_bits, lab in zip(pd[q, p][got_real].tolist(), pl[q, p][got_real].tolist()):
                    assert lab in lab_of and int(lab_of[lab]) == d_bits, "%s: query %d list %d: (%#x, %d) is no survivor of its slice" % (what, q, p, d_bits, lab)


def make_allow(data, lists, rng, kind):
    if kind is None:
        return None
    bits = np.zeros((data.nbits + 63) // 64 + 1, np.uint64)
    if kind == "none":
        return bits
    ok = rng.random(data.n) < 0.7
    ok[data.dup[2]] = True                             # the label at nbits - 1 is let through; the one at nbits cannot be
    for q, rows in enumerate(lists):                   # ... and each query loses its nearest survivor, and its third
        if rows.size:
            o = np.lexsort((data.labels[rows], data.table[q, rows]))
            for t in (0, 2):
                if t < o.size and rows[o[t]] != data.dup[2]:
                    ok[rows[o[t]]] = False
    lab = data.labels[ok & (data.labels < np.uint64(data.nbits))]
    np.bitwise_or.at(bits, (lab >> np.uint64(6)).astype(np.int64), np.uint64(1) << (lab & np.uint64(63)))
    got = data.allowed(bits)
    assert (got == (ok & (data.labels < np.uint64(data.nbits)))).all() and not got[data.dup[1]] and got[data.dup[2]]
    return bits


def mixed_counts(k, nq_min=16):
    c = FS.rerank_counts(k)
    return c + [300] * max(0, nq_min - len(c))


def top_rows_of(data, lists, allow_rows, k):
    out = []
    for q, rows in enumerate(lists):
        r = rows.astype(np.int64)
        lab = np.where(allow_rows[r], data.labels[r], np.uint64(NO_LABEL))
        out.append(rows[FS.select_model(np.ascontiguousarray(data.table[q, r]), lab, k)])
    return out


# (D, bf16, l2): 64 -> round16's tail loop only, 192 -> 8-loop + tail, 768 -> 48-loop, 832 -> 48 + tail, 960 -> 48 + 8 + tail;
# 384 -> list mode's 24-loop.  The long lists (eight blocks) at D = 64 and 192 only: few bytes per row.
RERANK_CONFIGS = [(64, False, False), (64, True, True), (64, False, True), (64, True, False), (192, False, True), (192, True, False),
                  (384, True, False), (384, False, True), (768, False, False), (768, True, True), (832, False, True), (832, True, False),
                  (960, True, False), (960, False, True)]


@pytest.mark.parametrize("D,bf16,l2", RERANK_CONFIGS, ids=lambda v: str(int(v)))
def test_rerank_mixed_lists(probe, oracle, D, bf16, l2):
    """lists of every length class side by side in one launch; fused with and without the second bound, and un-fused"""
    big = D <= 192
    n = 2304 if big else 640
    rng = np.random.default_rng([D, int(bf16), int(l2), 7])
    for k in (1, 10, 64, 100, 300):
        if k > 64 and D not in (64, 384, 768):
            continue
        counts = [c for c in mixed_counts(k) if c <= n and (big or c <= 600)]
        counts = counts + [300] * (16 - len(counts))
        nq = len(counts)
        data = dataset(oracle, D, bf16, l2, n, 24)
        assert nq <= 24
        lists = make_lists(data, counts, rng)
        ovf = np.zeros(nq, np.uint32)
        ovf[[3, nq - 2]] = 1                           # a short list and a long one handed over
        for allow_kind in (None, "some", "none"):
            allow = make_allow(data, lists, rng, allow_kind)
            allow_rows = data.allowed(allow)
            nbits = 0 if allow is None else data.nbits
            tops = top_rows_of(data, lists, allow_rows, k)
            runs = [(False, False, None)]
            if k <= 64:
                runs += [(True, False, None), (True, True, "random"), (True, True, "adversarial")]
                if allow_kind is None:
                    runs += [(True, True, "nan")]
            if allow_kind is not None and k not in (10, 100):
                runs = runs[:2]
            for fused, prune, mode in runs:
                tn = data.tile_norm.copy()
                if mode == "nan":                      # tiles outside f16: their norm is +inf, "no information"
                    tn[::3] = np.float32(np.inf)
                # the second bound reasons about the list's rows as candidates for the answer: the filter lists allowed rows only
                # (flat_filter.hip applies the bitmap before it appends), so with the bound on the lists are what it would leave
                run_lists = [r[allow_rows[r]] for r in lists] if prune and allow is not None else lists
                vals = scores(data, run_lists, mode or "exact", rng, tops, COEF, tn)
                for out_ld, use_ovf in ((k, False), (k + 3, True)):
                    for fill in FILLS:
                        o = probe.rerank(data, run_lists, vals, k=k, out_ld=out_ld, cap=4096, fused=fused, prune=prune, fill=fill,
                                         qcoef=np.tile(np.array(COEF, np.float32), (nq, 1)), tile_norm=tn, allow=allow, nbits=nbits,
                                         ovf=ovf if use_ovf else None)
                        what = "D %d bf16 %d l2 %d k %d allow %s fused %d prune %d scores %s out_ld %d fill %#x" % (
                            D, bf16, l2, k, allow_kind, fused, prune, mode, out_ld, fill)
                        check_rerank(data, o, run_lists, allow_rows, k=k, out_ld=out_ld, cap=4096, fused=fused, prune=prune, fill=fill,
                                     ovf=ovf if use_ovf else None, what=what)


@pytest.mark.parametrize("bf16,l2", [(False, False), (True, True)])
def test_rerank_every_fill(probe, oracle, bf16, l2):
    """one launch of each kind from each of the three patterns: the same words come back"""
    k, D = 10, 64
    data = dataset(oracle, D, bf16, l2, 2304, 24)
    rng = np.random.default_rng(11)
    lists = make_lists(data, mixed_counts(k), rng)
    nq = len(lists)
    allow_rows = data.allowed(None)
    vals = scores(data, lists, "random", rng)
    ovf = np.zeros(nq, np.uint32)
    ovf[5] = 1
    for fused, prune in ((True, True), (True, False), (False, False)):
        outs = []
        for fill in FILLS:
            o = probe.rerank(data, lists, vals, k=k, out_ld=k + 3, cap=4096, fused=fused, prune=prune, fill=fill,
                             qcoef=np.tile(np.array(COEF, np.float32), (nq, 1)), tile_norm=data.tile_norm, ovf=ovf)
            check_rerank(data, o, lists, allow_rows, k=k, out_ld=k + 3, cap=4096, fused=fused, prune=prune, fill=fill, ovf=ovf,
                         what="fill %#x fused %d prune %d" % (fill, fused, prune))
            outs.append(o)
        keep = ovf == 0
        for o in outs[1:]:
            assert (o.dist[keep] == outs[0].dist[keep]).all() and (o.label[keep] == outs[0].label[keep]).all() and (o.n[keep] == outs[0].n[keep]).all()
            assert (o.done == outs[0].done).all()


@pytest.mark.parametrize("l2", [False, True])
def test_rerank_small_private_list(probe, oracle, l2):
    """cand_cap = 256: the list in registers up to 256, walked by one block through spill chunks behind it, and by eight blocks
    across the edge of a chunk; chunk numbers not contiguous and interleaved between the queries"""
    k, D, cap = 10, 64, FS.RERANK_SMALL_CAP
    data = dataset(oracle, D, False, l2, 4480, 24)
    rng = np.random.default_rng(12)
    counts = FS.RERANK_SMALL_CAP_COUNTS + [0, 9, 300, 2048, 2049, 1000, 4352, 257, 256]
    lists = make_lists(data, counts, rng)
    nq = len(lists)
    allow_rows = data.allowed(None)
    tops = top_rows_of(data, lists, allow_rows, k)
    coef = np.tile(np.array(COEF, np.float32), (nq, 1))
    for fused, prune, mode in ((True, False, "exact"), (True, True, "random"), (True, True, "adversarial"), (True, True, "nan"),
                               (False, False, "exact"), (True, True, "random")):
        tn = data.tile_norm.copy()
        if mode == "nan":
            tn[1::2] = np.float32(np.inf)
        vals = scores(data, lists, mode, rng, tops, COEF, tn)
        for fill in FILLS:
            o = probe.rerank(data, lists, vals, k=k, out_ld=k, cap=cap, fused=fused, prune=prune, fill=fill, qcoef=coef, tile_norm=tn)
            # the chunk table the probe made: a query's chunks are not consecutive numbers, and the queries' chunks interleave
            taken = sorted((int(c) - 2, q) for q in range(nq) for c in o.qchunk[q] if c)
            assert len(taken) == sum(-(-max(0, c - cap) // FS.SPILL_CHUNK) for c in counts)
            assert all(b[0] - a[0] >= 2 for a, b in zip(taken, taken[1:])) and any(a[1] != b[1] for a, b in zip(taken, taken[1:]))
            check_rerank(data, o, lists, allow_rows, k=k, out_ld=k, cap=cap, fused=fused, prune=prune, fill=fill, ovf=None,
                         what="cap 256 l2 %d fused %d prune %d scores %s fill %#x" % (l2, fused, prune, mode, fill))


def test_rerank_long_list_flushes_inside_the_walk(probe, oracle):
    """20 000 survivors at D = 64: each of the 32 waves keeps 625 entries, more than its 512 waiting slots, so flush() runs inside
    the walk.  Without the second bound every step keeps 64; with it (most scores NaN = kept, the far rows pruned) a step keeps
    an uneven number and flush() has entries to move to the front."""
    k, D, cap, n_long = 10, 64, FS.RERANK_SMALL_CAP, FS.RERANK_LONG
    data = dataset(oracle, D, False, False, 20480, 16)
    rng = np.random.default_rng(13)
    counts = [n_long, 5, 0, 700, 64, 2049, 17, 1, 300, 16, 513, 65, 10, 11, 9, 63]
    lists = make_lists(data, counts, rng)
    nq = len(lists)
    assert FS.rerank_path(n_long, cap, False) == ("blocks", True)
    allow_rows = data.allowed(None)
    coef = np.tile(np.array(COEF, np.float32), (nq, 1))
    for prune in (False, True):
        vals = scores(data, lists, "random", rng)
        if prune:
            far = data.S[0, lists[0]] < np.quantile(data.S[0, lists[0]], 0.1)      # the far tenth keeps its score, the rest: no information
            vals[0][~far] = np.float32(np.nan)
        for fill in FILLS:
            o = probe.rerank(data, lists, vals, k=k, out_ld=k + 3, cap=cap, fused=True, prune=prune, fill=fill, qcoef=coef, tile_norm=data.tile_norm)
            check_rerank(data, o, lists, allow_rows, k=k, out_ld=k + 3, cap=cap, fused=True, prune=prune, fill=fill, ovf=None,
                         what="long list prune %d fill %#x" % (prune, fill))
            if prune:
                assert FS.RERANK_SLOTS - 64 < int(o.reranked[0]) // 32 and int(o.reranked[0]) < n_long, "the case means to prune some and keep most"


@pytest.mark.parametrize("bf16,l2", [(False, False), (False, True), (True, False)])
def test_second_bound_prunes(probe, oracle, bf16, l2):
    """With well-separated scores and small margins the bound must prune: reranked[q] <= the survivors whose hi reaches
    b - 2^-10 max(1, |b|), b = the k-th largest lo among the first min(n, 2048, cand_cap) survivors (kBoundBits = 20 leaves
    the threshold short of the k-th largest key by less than 2^-11 relative, the kernel adds 2^-21 max(1, |b|))."""
    D = 64
    data = dataset(oracle, D, bf16, l2, 4480, 24)
    rng = np.random.default_rng(14)
    for k, cap in ((10, 4096), (1, 4096), (64, 4096), (10, 256)):
        counts = [c for c in mixed_counts(k) if c] + [4353, 3000]
        lists = make_lists(data, counts, rng)
        nq = len(lists)
        vals = scores(data, lists, "exact", rng, coef=COEF_SMALL)
        may = []                                       # per query: how many rows the bound may leave; None: fewer than k to bound by
        for rows, val in zip(lists, vals):
            n, m = rows.size, data.margin(COEF_SMALL, rows.astype(np.int64))
            v = val.astype(np.float64)
            n_sel = min(n, 2048, cap)
            if n_sel < k:
                may.append(None)
                continue
            b = np.sort((v - m)[:n_sel])[n_sel - k]
            may.append(int(((v + m) >= b - 2.0 ** -10 * max(1.0, abs(b))).sum()))
        assert sum(m is not None and m < rows.size for m, rows in zip(may, lists)) >= 5, "the case means to have something to prune"
        for fill in FILLS:
            o = probe.rerank(data, lists, vals, k=k, out_ld=k, cap=cap, fused=True, prune=True, fill=fill,
                             qcoef=np.tile(np.array(COEF_SMALL, np.float32), (nq, 1)), tile_norm=data.tile_norm)
            check_rerank(data, o, lists, data.allowed(None), k=k, out_ld=k, cap=cap, fused=True, prune=True, fill=fill, ovf=None,
                         what="pruning k %d cap %d fill %#x" % (k, cap, fill))
            for q, rows in enumerate(lists):
                if may[q] is None:
                    assert int(o.reranked[q]) == rows.size
                    continue
                assert k <= int(o.reranked[q]) <= may[q], "k %d cap %d fill %#x query %d: %d rows re-ranked, the bound leaves %d of %d" % (
                    k, cap, fill, q, int(o.reranked[q]), may[q], rows.size)


# ---- K8 and the small kernels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,bf16,l2", [(64, False, False), (64, True, True), (192, False, True), (768, True, False)], ids=lambda v: str(int(v)))
def test_gather_distance(probe, oracle, D, bf16, l2):
    data = dataset(oracle, D, bf16, l2, 2304 if D <= 192 else 640, 24)
    rng = np.random.default_rng(15)
    sizes = [1, 15, 16, 17, 64, 1000] + ([2048 * 4 * 16 + 17] if D == 64 else [])
    for i, n in enumerate(sizes):
        q = i % data.nq
        idx = rng.integers(0, data.n, n).astype(np.uint32)
        idx[-1] = data.n - 1
        want = data.table[q, idx].view(np.uint32)
        for fill in FILLS:
            out = np.zeros(n + 64, np.uint32)
            rc = probe.lib.fs_probe_gather(ptr(data.dev_rows), data.n, D, int(bf16), int(l2), ptr(data.Q[q]), ptr(idx), n, out.size, fill, ptr(out))
            assert rc == 0, rc_text("fs_probe_gather", rc)
            bad = np.flatnonzero(out[:n] != want)
            assert bad.size == 0, "n %d fill %#x: out[%d] = %#x, the oracle's distance is %#x" % (n, fill, bad[0], out[bad[0]], want[bad[0]])
            assert (out[n:] == fill).all(), "n %d fill %#x: a word behind the list was written" % (n, fill)
    for fill in FILLS:
        out = np.zeros(8, np.uint32)
        assert probe.lib.fs_probe_gather(ptr(data.dev_rows), data.n, D, int(bf16), int(l2), ptr(data.Q[0]), ptr(np.zeros(1, np.uint32)), 0, 8, fill, ptr(out)) == 0
        assert (out == fill).all()


@pytest.mark.parametrize("nq", [1, 256, 257])
def test_kth_bound(probe, nq):
    rng = np.random.default_rng(nq)
    for k in (1, 10):
        special = np.array([-np.inf, -2.5, -1e-40, -0.0, 0.0, 1e-40, 3.0, 3.4e38, np.inf], np.float32)
        d = rng.standard_normal((nq, k)).astype(np.float32)
        d[:, k - 1] = special[np.arange(nq) % special.size]
        n = np.where(np.arange(nq) % 5 == 2, rng.integers(0, k, nq), k + (np.arange(nq) % 2)).astype(np.uint32)     # < k, == k, > k
        for fill in FILLS:
            out = np.zeros(2 * nq + 8, np.uint32)
            rc = probe.lib.fs_probe_kth_bound(ptr(d), ptr(n), k, nq, fill, ptr(out))
            assert rc == 0, rc_text("fs_probe_kth_bound", rc)
            b = np.where(n >= k, d[:, k - 1].view(np.uint32), np.uint32(INF_BITS)).astype(np.uint32)
            key = np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
            assert (out[:nq] == b).all() and (out[nq:2 * nq] == key).all() and (out[2 * nq:] == fill).all()
            # the key word orders like the float (-0 below +0: the K4 bound compares keys, and -0 is the smaller key)
            f = b.view(np.float32)[np.argsort(key, kind="stable")]
            assert (f[1:] >= f[:-1]).all()


@pytest.mark.parametrize("nq,k", [(1, 1), (7, 37), (257, 3), (4100, 65)])
def test_fill_empty(probe, nq, k):
    assert (nq * k) % 256 != 0 or nq * k > 1024 * 256
    for with_n in (1, 0):
        for fill in FILLS:
            d = np.zeros(nq * k + 8, np.uint32)
            l = np.zeros(nq * k + 8, np.uint64)
            n = np.zeros(nq + 8, np.uint32)
            rc = probe.lib.fs_probe_fill_empty(nq, k, with_n, fill, ptr(d), ptr(l), ptr(n))
            assert rc == 0, rc_text("fs_probe_fill_empty", rc)
            assert (d[:nq * k] == INF_BITS).all() and (l[:nq * k] == np.uint64(NO_LABEL)).all()
            assert (d[nq * k:] == fill).all() and (l[nq * k:] == fill64(fill)).all()
            assert (n[:nq] == (0 if with_n else fill)).all() and (n[nq:] == fill).all()
