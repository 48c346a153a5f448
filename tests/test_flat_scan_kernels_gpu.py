"""The two kernels behind every exact FLAT answer on their own, through tests/helpers/flat_scan_probe.hip -- a small library that
includes csrc/flat_scan.hip and csrc/flat_gemm.hip themselves, built with the product's compiler flags, so the product's kernels
and launchers run: flat_scan_kernel in its plain mode (K3: every query block, every slots-per-lane variant, the paged scan, the
redo mode) and flat_gemm_kernel / flat_gemm_prepass_kernel (K4), with the partition count, the tile walk, the lockstep window,
the pre-pass bound, cancel and run_flag chosen by the test instead of derived from an index.

Every comparison is an equality of bits, of sets of (distance bits, label) pairs, or of integers.  Distances are the oracle's
(oracle.Flat over the same rows; bf16 rows: over the rounded rows), selection is select_model, and which list owns a row is the
model of tests/helpers/flat_scan_cases.py; tests/test_flat_scan_model_cpu.py checks that model and that the inputs here reach
the paths they are meant for.  Every case runs from output and workspace buffers filled with 0x00000000, 0xFFFFFFFF and
0x7F7FFFFF, and the rows past n_rows hold large finite values (zeros, as in the product, in two cases).

K3: every list is deterministic.  As a set, a list is select_model over its own allowed rows (the paged scan: those strictly
beyond the query's lower bound), every other slot is (+inf, kNoLabel), and a list the contract leaves unwritten -- a compact
index >= *nq_dev, a skipped launch -- still holds the pattern.

K4, k <= 10 (lists in registers): the same, over the slot's own allowed rows at or below init_bound[q]; with cancel raised,
over the block's first tile alone.  sync holds the tile count of every partition when lockstep is on and zeros otherwise, qbound
keeps what it was seeded with; a hand-over launch (run_flag) leaves both at the pattern.

K4, k > 10 (lists in HBM, pruned by a bound that other blocks move while the kernel runs) is the one place held to less than
"equal to the model": which of its own rows beyond the query's k best a list still holds depends on when its lane saw the
shared bound drop.  Asserted are: every non-empty entry is an allowed row of the slot's own rows with the oracle's distance
bits, no label twice, every empty slot (+inf, kNoLabel); every own row that belongs to the query's true top-k is in its list;
all lists of a query merged by select_model are the oracle's top-k; and key(true k-th best allowed distance) <= qbound[q] <= its
initial value."""
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
LIB = HERE / "libflatscanprobe.so"
sys.path.insert(0, str(HERE))
import flat_scan_cases as SC  # noqa: E402

NO_LABEL, INF_BITS, FILLS, INF_KEY = SC.NO_LABEL, SC.INF_BITS, SC.FILLS, SC.INF_KEY
u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
# the product's own flags (csrc/Makefile): the kernels under test are the kernels the library ships
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]


def build_probe():
    src = HERE / "flat_scan_probe.hip"
    deps = (src, CSRC / "flat_scan.hip", CSRC / "flat_gemm.hip", CSRC / "kernels.hpp", CSRC / "device_common.hpp", CSRC / "row_store.hpp")
    newest = max(p.stat().st_mtime for p in deps)
    if not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "-shared", "-fPIC", "-I", str(CSRC), str(src), "-o", str(LIB)])
    return LIB


class GemmIO(C.Structure):
    _fields_ = ([(n, vp) for n in ("rows", "labels", "queries", "allow_bits")] + [("allow_nbits", u64), ("init_bound", vp)]
                + [(n, u32) for n in ("n_rows", "n_alloc", "stride", "bf16", "nq", "k", "nrp", "tile_q", "lockstep", "contig", "prepass", "cancel",
                                      "use_flag", "flag_value", "run_if", "run_hi", "fill")]
                + [(n, vp) for n in ("part_dist", "part_label", "sync", "qbound")])


class ScanIO(C.Structure):
    _fields_ = ([(n, vp) for n in ("rows", "labels", "queries", "allow_bits")] + [("allow_nbits", u64)]
                + [(n, vp) for n in ("lb_dist", "lb_label", "q_index")]
                + [(n, u32) for n in ("n_alloc", "stride", "bf16", "l2", "qb", "e", "row_begin", "row_end", "nq", "k", "nrp", "nq_dev", "use_cancel",
                                      "cancel", "use_flag", "flag_value", "run_if", "run_hi", "fill")]
                + [(n, vp) for n in ("part_dist", "part_label")])


def ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


def rc_text(name, rc):
    return "%s refused its arguments" % name if rc == 1 else "%s: HIP error seen at flat_scan_probe.hip:%d" % (name, rc)


def check_rc(name, rc, expect_rc):
    if rc not in (0, 1):                                          # a HIP error: nothing more is launched on this device by this session
        pytest.exit(rc_text(name, rc), returncode=3)
    assert rc == expect_rc, rc_text(name, rc)


class Out:
    pass


class Probe:
    def __init__(self):
        lib = C.CDLL(str(build_probe()))
        lib.fsc_probe_gemm.argtypes = [C.POINTER(GemmIO)]
        lib.fsc_probe_scan.argtypes = [C.POINTER(ScanIO)]
        lib.fsc_gemm_lds_bytes.restype = u64
        lib.fsc_gemm_lds_bytes.argtypes = [u32, u32]
        lib.fsc_gemm_supported.argtypes = [u32, u64]
        lib.fsc_scan_pick_qb.argtypes = [u64, u32, C.c_int, u32]
        lib.fsc_scan_slots_per_lane.argtypes = [u64]
        for f in (lib.fsc_row_slack, lib.fsc_gemm_tile_q, lib.fsc_gemm_supported):
            f.restype = u32
        self.lib = lib
        self.slack = int(lib.fsc_row_slack())

    def gemm(self, c, rows, labels, queries, bits, nbits, bound, fill, expect_rc=0):
        o = Out()
        o.dist = np.zeros((c.nq, c.nrp * 8, c.k), np.uint32)
        o.label = np.zeros((c.nq, c.nrp * 8, c.k), np.uint64)
        o.sync = np.zeros((c.nrp, 4, 32), np.uint32)
        o.qbound = np.zeros(c.nq, np.uint32)
        use_flag, flag_value, run_if, run_hi = (0, 0, 0, 0) if c.flag is None else (1, *c.flag)
        io = GemmIO(ptr(rows), ptr(labels), ptr(queries), ptr(bits), nbits, ptr(bound), c.n, c.n, c.stride, c.bf16, c.nq, c.k, c.nrp, c.tile_q,
                    c.lockstep, c.contig, c.prepass, c.cancel, use_flag, flag_value, run_if, run_hi, fill, ptr(o.dist), ptr(o.label), ptr(o.sync),
                    ptr(o.qbound))
        rc = self.lib.fsc_probe_gemm(C.byref(io))
        check_rc("fsc_probe_gemm", rc, expect_rc)
        return o

    def scan(self, c, rows, labels, queries, bits, nbits, lb_d, lb_l, fill, expect_rc=0):
        n_lists = c.nrp * (1 if c.e == 1 else 4)
        o = Out()
        o.dist = np.zeros((c.nq, n_lists, c.k), np.uint32)
        o.label = np.zeros((c.nq, n_lists, c.k), np.uint64)
        q_index = np.array(SC.Q_INDEX, np.uint32) if c.redo is not None else None
        if c.flag == "nq_dev":
            use_flag, flag_value, run_if, run_hi = 2, 0, *SC.REDO_FLAG
        else:
            use_flag, flag_value, run_if, run_hi = (0, 0, 0, 0) if c.flag is None else (1, *c.flag)
        io = ScanIO(ptr(rows), ptr(labels), ptr(queries), ptr(bits), nbits, ptr(lb_d), ptr(lb_l), ptr(q_index), SC.N_SCAN, c.stride, c.bf16, c.l2, c.qb,
                    c.e, c.row_begin, c.row_begin + c.row_len, c.nq, c.k, c.nrp, c.redo or 0, 0 if c.cancel is None else 1, c.cancel or 0, use_flag,
                    flag_value, run_if, run_hi, fill, ptr(o.dist), ptr(o.label))
        rc = self.lib.fsc_probe_scan(C.byref(io))
        check_rc("fsc_probe_scan", rc, expect_rc)
        return o


@pytest.fixture(scope="module")
def probe():
    return Probe()


def fill64(fill):
    return np.uint64(fill | (fill << 32))


def chunks(cases, group, size):
    own = [c for c in cases if c.group == group]
    return [pytest.param(own[i:i + size], id="%s-%d" % (group, i // size)) for i in range(0, len(own), size)]


def assert_lists(got_d, got_l, want_d, want_l, what):
    """one query's lists against the model's, as sets"""
    gd, gl = SC.canon(got_d, got_l)
    bad = np.argwhere((gd != want_d) | (gl != want_l))
    assert bad.size == 0, "%s: list %d: holds (%#x, %#x) where the model has (%#x, %#x); %d entries differ" % (
        what, bad[0][0], gd[tuple(bad[0])], gl[tuple(bad[0])], want_d[tuple(bad[0])], want_l[tuple(bad[0])], len(bad))


def assert_pattern(got_d, got_l, fill, what):
    assert (got_d == fill).all() and (got_l == fill64(fill)).all(), "%s: not this launch's to write, and a word changed" % what


def test_host_side_helpers(probe):
    lib = probe.lib
    assert probe.slack >= 128                                     # one K4 tile past the capacity at the least
    for stride, tq in SC.TILE_Q.items():
        assert lib.fsc_gemm_tile_q(stride) == tq, stride
        assert lib.fsc_gemm_lds_bytes(stride, tq) <= 160 * 1024
        assert tq == 32 or lib.fsc_gemm_lds_bytes(stride, tq + 8) > 160 * 1024
        assert lib.fsc_gemm_supported(stride, 1) and lib.fsc_gemm_supported(stride, 256) and not lib.fsc_gemm_supported(stride, 257)
    assert not lib.fsc_gemm_supported(96, 10) and not lib.fsc_gemm_supported(64, 0)
    assert [lib.fsc_scan_slots_per_lane(k) for k in (1, 64, 65, 256, 257, 1024, 1025)] == [1, 1, 4, 4, 16, 16, 0]
    # every (query block, slots per lane) the cases launch is one the product's choice can produce
    picks = {(lib.fsc_scan_pick_qb(nq, 4, e, l2), e) for nq in (1, 2, 3, 4, 7, 8, 100) for e in (1, 4, 16) for l2 in (0, 1)}
    assert {(c.qb, c.e) for c in SC.scan_cases()} <= picks
    assert lib.fsc_scan_pick_qb(100, 4096 // 16, 1, 0) * 4096 * 4 <= 64 * 1024


# ---- K4 --------------------------------------------------------------------------------------------------------------------
GEMM_CASES = SC.gemm_cases()


def gemm_hbm_lists(c, data, labels, allowed, owner, got, initial, q, what):
    """k > 10: what can be said of lists pruned by a bound that moves while the kernel runs (see the module's docstring)"""
    gd, gl = got.dist[q], got.label[q]
    real = gl != np.uint64(NO_LABEL)
    assert (gd[~real] == INF_BITS).all(), what + ": an empty slot without +inf"
    sorter = np.argsort(labels)
    at = np.minimum(np.searchsorted(labels[sorter], gl[real]), labels.size - 1)
    rows = sorter[at]
    assert (labels[rows] == gl[real]).all(), what + ": a label no row of the index has"
    lists = np.broadcast_to(np.arange(gl.shape[0])[:, None], gl.shape)[real]
    assert (owner[rows] == lists).all(), what + ": a row in a list that does not own it"
    assert allowed[rows].all(), what + ": a row the filter does not allow"
    assert (data.table_bits[q, rows] == gd[real]).all(), what + ": distance bits differ from the oracle's"
    srt = np.sort(gl, axis=1)
    assert not ((srt[:, 1:] == srt[:, :-1]) & (srt[:, 1:] != np.uint64(NO_LABEL))).any(), what + ": a label twice in one list"
    kth_key = int(SC.f32_key(SC.kth_best(data.table[q], labels, allowed, c.k)).reshape(-1)[0])
    assert kth_key <= int(got.qbound[q]) <= int(initial[q]), "%s: qbound %#x, the true k-th best has key %#x, it started at %#x" % (
        what, got.qbound[q], kth_key, initial[q])
    if c.cancel:
        return
    top = SC.ranking(data.table[q], labels, allowed)[:c.k]
    present = np.zeros(data.n, bool)
    present[rows] = True
    assert present[top].all(), what + ": a row of the true top-k is missing from its list"
    md, ml = SC.merged(gd, gl, c.k)
    assert md.tolist() == data.table_bits[q, top].tolist() and ml.tolist() == labels[top].tolist(), what + ": the merged lists are not the top-k"


def run_gemm_case(probe, oracle, c):
    data = SC.dataset(oracle, "IP", c.stride, c.bf16, c.n, c.nq, SC.GEMM_DUPS)
    all_labels = SC.make_labels(c.labels, c.n, c.n + probe.slack, 0)
    labels = all_labels[:c.n]
    bits, nbits, allowed = SC.make_filter(labels, c.n, c.filt, 0) if c.filt is not None else (None, 0, np.ones(c.n, bool))
    rows = data.device_rows(c.n, probe.slack, c.slack)
    bound = SC.gemm_bound(c.bound, data, labels, allowed, c.k, c.nq)
    initial = np.full(c.nq, INF_KEY, np.uint32) if bound is None else bound[c.nq:]
    runs = SC.flag_runs(c.flag)
    owner, _count = SC.gemm_owner(c.n, c.nrp, c.contig, first_tile_only=bool(c.cancel))
    tiles = [len(t) for t in SC.gemm_tiles(c.n, c.nrp, c.contig)]
    nqt = (c.nq + c.tile_q - 1) // c.tile_q
    want = None
    if c.k <= 10 and runs:
        want = []
        for q in range(c.nq):
            elig = allowed if bound is None else allowed & (data.table[q] <= bound[:c.nq].view(np.float32)[q])
            want.append(SC.lists_want(data.table[q], labels, elig, owner, c.nrp * 8, c.k)[:2])
    for fill in FILLS:
        what = "%r fill %#x" % (c, fill)
        o = probe.gemm(c, rows, all_labels, data.Q, bits, nbits, bound, fill)
        if not runs:
            assert_pattern(o.dist, o.label, fill, what)
        elif c.k <= 10:
            for q in range(c.nq):
                assert_lists(o.dist[q], o.label[q], want[q][0], want[q][1], "%s query %d" % (what, q))
        else:
            for q in range(c.nq):
                gemm_hbm_lists(c, data, labels, allowed, owner, o, initial, q, "%s query %d" % (what, q))
        if c.flag is not None:                                    # the hand-over launch: nobody prepares or touches either
            assert (o.sync == fill).all() and (o.qbound == fill).all(), what + ": sync / qbound of a hand-over launch"
            continue
        ws = np.zeros((c.nrp, 4, 32), np.uint32)
        if c.lockstep:
            for rp in range(c.nrp):
                ws[rp, :, :nqt] = min(tiles[rp], 1) if c.cancel else tiles[rp]
        assert (o.sync == ws).all(), what + ": the progress words"
        if c.k <= 10:
            assert (o.qbound == initial).all(), what + ": qbound of a launch with register lists"


@pytest.mark.parametrize("cases", [p for g in ("shapes", "strides", "lockstep", "kinds", "bounds", "filters", "control") for p in chunks(GEMM_CASES, g, 12)])
def test_gemm(probe, oracle, cases):
    for c in cases:
        run_gemm_case(probe, oracle, c)


def test_gemm_refuses(probe, oracle):
    c = SC.gcase("refuse")
    data = SC.dataset(oracle, "IP", c.stride, c.bf16, c.n, c.nq, SC.GEMM_DUPS)
    labels = SC.make_labels(c.labels, c.n, c.n + probe.slack, 0)
    rows = data.device_rows(c.n, probe.slack, c.slack)
    for bad in (c._replace(nrp=12), c._replace(nrp=0), c._replace(tile_q=8), c._replace(k=257), c._replace(k=0), c._replace(stride=96),
                c._replace(stride=1536, tile_q=32), c._replace(nq=0), c._replace(k=11, flag=(1, 1, 0))):
        probe.gemm(bad, rows, labels, data.Q, None, 0, None, 0, expect_rc=1)


# ---- K3 --------------------------------------------------------------------------------------------------------------------
SCAN_CASES = SC.scan_cases()


def run_scan_case(probe, oracle, c):
    data = SC.dataset(oracle, "L2" if c.l2 else "IP", c.stride, c.bf16, SC.N_SCAN, SC.SCAN_NQ, SC.SCAN_DUPS)
    all_labels = SC.make_labels("small", SC.N_SCAN, SC.N_SCAN + probe.slack, 1)
    labels = all_labels[:SC.N_SCAN]
    bits, nbits, allowed = SC.make_filter(labels, SC.N_SCAN, c.filt, 1) if c.filt is not None else (None, 0, np.ones(SC.N_SCAN, bool))
    rows = data.device_rows(SC.N_SCAN, probe.slack, "large")
    owner, n_lists, elig, lb_d, lb_l = SC.scan_setup(c, data, labels, allowed)
    runs = SC.scan_runs(c)
    # list index -> the query it serves (None: not written)
    served = list(range(c.nq)) if c.redo is None else [SC.Q_INDEX[i] if i < c.redo else None for i in range(c.nq)]
    want = {}
    for q in {s for s in served if s is not None}:
        e = np.zeros(SC.N_SCAN, bool) if c.cancel else elig[q]    # cancel raised before the launch: the poll precedes the first tile
        want[q] = SC.lists_want(data.table[q], labels, e, owner, n_lists, c.k)
    queries = np.ascontiguousarray(data.Q[:c.nq])
    for fill in FILLS:
        what = "%r fill %#x" % (c, fill)
        o = probe.scan(c, rows, all_labels, queries, bits, nbits, lb_d, lb_l, fill)
        for i in range(c.nq):
            if not runs or served[i] is None:
                assert_pattern(o.dist[i], o.label[i], fill, "%s list %d" % (what, i))
                continue
            wd, wl, _rows = want[served[i]]
            assert_lists(o.dist[i], o.label[i], wd, wl, "%s list %d (query %d)" % (what, i, served[i]))
            if c.lb is not None:                                  # the lists merged: entries j + 1 .. j + k of the ranking, exactly
                md, ml = SC.merged(o.dist[i], o.label[i], c.k)
                full = SC.ranking(data.table[i], labels, (owner >= 0) & allowed)[c.lb + 1:c.lb + 1 + c.k]
                assert md.tolist() == data.table_bits[i, full].tolist() and ml.tolist() == labels[full].tolist(), what + ": the page"


@pytest.mark.parametrize("cases", [p for g in ("variants", "nq", "strides", "windows", "filters", "paged", "redo", "control") for p in chunks(SCAN_CASES, g, 12)])
def test_scan(probe, oracle, cases):
    for c in cases:
        run_scan_case(probe, oracle, c)


def test_scan_refuses(probe, oracle):
    c = SC.scase("refuse", 4, 1, 10)
    data = SC.dataset(oracle, "IP", c.stride, c.bf16, SC.N_SCAN, SC.SCAN_NQ, SC.SCAN_DUPS)
    labels = SC.make_labels("small", SC.N_SCAN, SC.N_SCAN + probe.slack, 1)
    rows = data.device_rows(SC.N_SCAN, probe.slack, "large")
    q = np.ascontiguousarray(data.Q[:c.nq])
    for bad in (c._replace(nrp=12), c._replace(qb=3), c._replace(e=2), c._replace(k=65), c._replace(e=16, qb=2), c._replace(row_len=0),
                c._replace(row_len=SC.N_SCAN + 1), c._replace(stride=96), c._replace(flag="nq_dev")):
        probe.scan(bad, rows, labels, q, None, 0, None, None, 0, expect_rc=1)
