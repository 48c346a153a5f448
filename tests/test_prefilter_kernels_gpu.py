"""The two kernels of the batched pre-filter search (csrc/prefilter_select.hip) on their own, through
tests/helpers/prefilter_probe.hip -- a small library that includes that translation unit, so the product's kernels run.

Through the C ABI the host's heap rule gives the right answer over ANY superset of {distance <= T}, so a select kernel
(K8c) that hands back too much, or the right entries under a wrong threshold, is invisible there.  Here K8c's count word
and every (index, distance bits) pair it stores are compared with one independent statement in numpy:

    key(d)   = the documented order-preserving u32 of a float (-0 maps to +0, then the sign flip)
    T        = the min(k, n)-th smallest key, from a sort
    want_idx = the indices with key <= T, in order

    len(want_idx) <= cap : count == len(want_idx), cand[:count] == (index, f32 bits) of want_idx, bit for bit
    len(want_idx) >  cap : count > cap (the kernel does not promise the number), cand[:cap] == the first cap of want_idx
    any NaN              : count == 0xFFFFFFFF
    n == 0               : count == 0

prefilter_select_model (csrc/prefilter_host.hpp, what the CPU suite pins the heap rule against) is run on the same inputs
and must agree with the same statement: model and kernel are pinned to one reference, not to each other.

Segment lengths sit where the kernel changes path: the descent keeps 8 x 256 = 2048 keys in registers and re-reads the rest
of a segment from memory in each of its 32 passes; the compaction walks 256 entries per step.  K8b (the distances) is checked
bit for bit against the oracle's distance function on the same f32 row and query, at the edges of its 64-entry tiles, as a
CSR and as a shared list (whose grid rounds the tile count up to eight and deals blocks by b % 8)."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "helpers"
CSRC = ROOT / "valkey-search_amd" / "csrc"
LIB = HERE / "libprefilterprobe.so"

NAN_COUNT = 0xFFFFFFFF
UNWRITTEN = 0xEEEEEEEE                       # what the probe fills count / cand / dist with before the launch
REG = 2048                                   # kSelReg * 256: keys the descent holds in registers
LENGTHS = [0, 1, 255, 256, 257, 2047, 2048, 2049, 2303, 2304, 2305, 4095, 4096, 4097, 10000]
CSR_ORDER = [1, 255, 256, 0, 257, 2047, 2048, 2049, 2303, 0, 2304, 2305, 4095, 4096, 4097, 10000, 0]   # empties: middle and end
KS = [1, 10, 64, 4096]
CLASSES = ["normal", "bits", "three", "equal", "zeros", "kth_in_tail", "overflow_in_tail", "nan_first", "nan_tail", "nan_last",
           "nan_negative"]
VARIANTS = 3                                 # per (class, k, length): variant 0 is the CSR's segment, 0..2 the shared run's queries


def build_probe():
    src = HERE / "prefilter_probe.hip"
    newest = max(p.stat().st_mtime for p in (src, CSRC / "prefilter_select.hip", CSRC / "prefilter_host.hpp", CSRC / "kernels.hpp",
                                             CSRC / "device_common.hpp"))
    if not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", "-I", str(CSRC), str(src),
                               "-o", str(LIB)])
    return LIB


class Probe:
    def __init__(self):
        lib = C.CDLL(str(build_probe()))
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        lib.pf_probe_select.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp]
        lib.pf_probe_select.restype = C.c_int
        lib.pf_probe_distance_select.argtypes = [vp, u32, u32, vp, u32, vp, vp, vp, u32, C.c_int, u32, u32, vp, vp, vp]
        lib.pf_probe_distance_select.restype = C.c_int
        lib.pf_probe_model.argtypes = [vp, u64, u64, u64, vp, vp]
        lib.pf_probe_model.restype = u32
        lib.pf_probe_tiles.argtypes = [u64]
        lib.pf_probe_tiles.restype = u32
        self.lib = lib

    def select(self, segs, k, shared):
        """K8c over the segments (shared: equally long, laid out [nq][len]); returns count [nq], cand [nq][cap][2]"""
        nq, cap = len(segs), k + 64
        dist = np.ascontiguousarray(np.concatenate(segs), np.float32) if nq else np.zeros(0, np.float32)
        if shared:
            assert len({s.size for s in segs}) == 1
            seg, shared_len = None, segs[0].size
        else:
            seg, shared_len = offsets([s.size for s in segs]), 0
        count = np.zeros(nq, np.uint32)
        cand = np.zeros((nq, cap, 2), np.uint32)
        rc = self.lib.pf_probe_select(dist.ctypes.data, None if seg is None else seg.ctypes.data, nq, shared_len, k, cap,
                                      count.ctypes.data, cand.ctypes.data)
        assert rc == 0, f"pf_probe_select: HIP error seen at prefilter_probe.hip:{rc}" if rc > 1 else "pf_probe_select refused its arguments"
        return count, cand

    def distance_select(self, rows, Q, lists, l2, k, shared):
        """K8b then K8c; rows [n][stride], Q [nq][stride] zero padded; lists: per query row slots (shared: one list)"""
        nq, cap = Q.shape[0], k + 64
        if shared:
            idx, seg, tile, shared_len, entries = np.ascontiguousarray(lists[0], np.uint32), None, None, lists[0].size, nq * lists[0].size
        else:
            assert len(lists) == nq
            idx = np.ascontiguousarray(np.concatenate(lists), np.uint32)
            seg = offsets([l.size for l in lists])
            tile = offsets([self.lib.pf_probe_tiles(l.size) for l in lists])
            shared_len, entries = 0, idx.size
        dist = np.zeros(entries, np.float32)
        count = np.zeros(nq, np.uint32)
        cand = np.zeros((nq, cap, 2), np.uint32)
        rc = self.lib.pf_probe_distance_select(rows.ctypes.data, rows.shape[0], rows.shape[1], Q.ctypes.data, nq, idx.ctypes.data,
                                               None if seg is None else seg.ctypes.data, None if tile is None else tile.ctypes.data,
                                               shared_len, 1 if l2 else 0, k, cap, dist.ctypes.data, count.ctypes.data, cand.ctypes.data)
        assert rc == 0, f"pf_probe_distance_select: HIP error seen at prefilter_probe.hip:{rc}" if rc > 1 else "pf_probe_distance_select refused its arguments"
        return dist, count, cand

    def model(self, d, k):
        """prefilter_select_model on one segment: (count word, stored indices)"""
        cap = k + 64
        d = np.ascontiguousarray(d, np.float32)
        idx = np.zeros(cap, np.uint32)
        stored = C.c_uint32(0)
        count = self.lib.pf_probe_model(d.ctypes.data, d.size, k, cap, idx.ctypes.data, C.byref(stored))
        return count, idx[:stored.value]


@pytest.fixture(scope="module")
def probe():
    return Probe()


def offsets(lengths):
    b = np.zeros(len(lengths) + 1, np.uint32)
    b[1:] = np.cumsum(lengths)
    return b


# ---- the reference -----------------------------------------------------------------------------------------------------
def keys_of(d):
    """the documented mapping: -0 -> +0, then negatives inverted, the rest get the top bit: u32 order == float order"""
    u = np.ascontiguousarray(d, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def reference(d, k):
    """("nan" | "empty" | "fits" | "overflow", want_idx)"""
    if d.size == 0:
        return "empty", np.zeros(0, np.int64)
    if np.isnan(d).any():
        return "nan", None
    key = keys_of(d)
    T = np.sort(key)[min(k, d.size) - 1]
    want = np.flatnonzero(key <= T)
    return ("fits" if want.size <= k + 64 else "overflow"), want


def check_segment(d, k, count, cand, what):
    cap = k + 64
    outcome, want = reference(d, k)
    bits = np.ascontiguousarray(d, np.float32).view(np.uint32)
    if outcome == "nan":
        assert count == NAN_COUNT, (what, hex(int(count)))
    elif outcome == "empty":
        assert count == 0, (what, hex(int(count)))
    elif outcome == "fits":
        assert count == want.size, (what, int(count), want.size)
        assert cand[:want.size, 0].tolist() == want.tolist(), what
        assert cand[:want.size, 1].tolist() == bits[want].tolist(), what
    else:
        assert cap < count != NAN_COUNT, (what, int(count), want.size)
        assert cand[:cap, 0].tolist() == want[:cap].tolist(), what
        assert cand[:cap, 1].tolist() == bits[want[:cap]].tolist(), what
    return outcome


def check_model(probe, d, k, what):
    cap = k + 64
    outcome, want = reference(d, k)
    count, idx = probe.model(d, k)
    if outcome == "nan":
        assert count == NAN_COUNT, what
    elif outcome == "empty":
        assert count == 0 and idx.size == 0, what
    else:
        assert count == want.size, (what, count, want.size)       # (the model counts every entry, also beyond the cap)
        assert idx.tolist() == want[:cap].tolist(), what


# ---- the inputs --------------------------------------------------------------------------------------------------------
def make_segment(cls, k, n, rng):
    """n distances of one value class.  The classes that place something at or beyond index 2048 do so where the segment
    has such indices (and room); a shorter segment gets the same values wherever they fit."""
    if n == 0:
        return np.zeros(0, np.float32)
    tail = n - REG                                                 # entries the descent re-reads from memory
    if cls in ("normal", "nan_first", "nan_tail", "nan_last", "nan_negative"):
        d = rng.standard_normal(n).astype(np.float32)
        if cls == "nan_first":
            d[0] = np.nan
        elif cls == "nan_tail":
            d[rng.integers(REG, n) if tail > 0 else rng.integers(0, n)] = np.nan
        elif cls == "nan_last":
            d[n - 1] = np.nan
        elif cls == "nan_negative":
            d.view(np.uint32)[rng.integers(0, n)] = 0xFFC00000 | int(rng.integers(0, 1 << 22))
        return d
    if cls == "bits":                                              # the whole order: negatives, denormals, +-0, +-inf
        u = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F800000,
                            0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
        at = rng.random(n) < 0.05
        u[at] = rng.choice(special, int(at.sum()))
        d = u.view(np.float32)
        nan = np.isnan(d)
        u[nan] &= np.uint32(0x807FFFFF)                            # NaNs removed: the same mantissa as a denormal
        return u.view(np.float32)
    if cls == "three":
        return rng.choice(np.array([-1.5, 0.25, 3.0], np.float32), n)
    if cls == "equal":
        return np.full(n, np.float32(rng.standard_normal()), np.float32)
    if cls == "zeros":                                             # T lands on zero: -0 and +0 are one key
        d = rng.choice(np.array([0.0, -0.0], np.float32), n)
        neg = rng.choice(n, size=min(n, max(1, min(k - 1, 5))) if k > 1 else 0, replace=False)
        d[neg] = -1.0 - rng.random(neg.size).astype(np.float32)
        return d
    big = (1000.0 + rng.random(n)).astype(np.float32)
    if cls == "kth_in_tail":                                       # the k smallest only at indices >= 2048
        m = min(k, n)
        where = REG + rng.choice(tail, size=m, replace=False) if tail >= m else n - m + np.arange(m)
        big[where] = rng.permutation(m).astype(np.float32) / np.float32(m)     # m distinct values in [0, 1)
        return big
    if cls == "overflow_in_tail":                                  # k - 1 small ones below 2048 (as many as fit), T's value k + 65 times beyond
        head = min(n, REG)
        small = min(k - 1, head // 2)
        big[rng.choice(head, size=small, replace=False)] = rng.permutation(small).astype(np.float32) / np.float32(max(small, 1))
        if tail > 0:
            copies = min(k + 65, tail)
            big[REG + rng.choice(tail, size=copies, replace=False)] = np.float32(2.0)
        return big
    raise AssertionError(cls)


@pytest.fixture(scope="module")
def inputs():
    """every segment of the select tests, and the conditions they must meet -- asserted here, from numpy alone, before any
    of them reaches the GPU"""
    segs = {}
    seen = set()                 # outcomes among segments longer than 2048
    t_only_in_tail = False       # some long segment whose T is a value found only at index >= 2048
    for ci, cls in enumerate(CLASSES):
        for k in KS:
            for n in LENGTHS:
                for v in range(VARIANTS):
                    d = make_segment(cls, k, n, np.random.default_rng([ci, k, n, v]))
                    assert d.size == n and d.dtype == np.float32
                    segs[cls, k, n, v] = d
                    if n <= REG:
                        continue
                    outcome, want = reference(d, k)
                    seen.add(outcome)
                    if outcome != "nan":
                        key = keys_of(d)
                        T = np.sort(key)[min(k, n) - 1]
                        t_only_in_tail |= bool((key[REG:] == T).any() and not (key[:REG] == T).any())
            if cls.startswith("nan"):
                assert all(np.isnan(segs[cls, k, n, v]).sum() == 1 for n in LENGTHS[1:] for v in range(VARIANTS))
                if cls == "nan_tail":
                    assert all(np.isnan(segs[cls, k, n, v][REG:]).any() for n in LENGTHS if n > REG for v in range(VARIANTS))
                if cls == "nan_negative":
                    assert all((segs[cls, k, n, v].view(np.uint32)[np.isnan(segs[cls, k, n, v])] >> 31).all() for n in LENGTHS[1:] for v in range(VARIANTS))
            else:
                assert not any(np.isnan(segs[cls, k, n, v]).any() for n in LENGTHS for v in range(VARIANTS))
    assert seen >= {"fits", "overflow", "nan"}, seen
    assert t_only_in_tail
    # the two classes built for the re-read loop do what they were built for, on every segment that has the room
    for k in KS:
        for n in LENGTHS:
            if n - REG >= k:
                d = segs["kth_in_tail", k, n, 0]
                outcome, want = reference(d, k)
                assert outcome == "fits" and want.size == k and want.min() >= REG, (k, n)
            if n - REG >= k + 65:
                d = segs["overflow_in_tail", k, n, 0]
                outcome, want = reference(d, k)
                assert outcome == "overflow" and (want < REG).sum() <= k - 1 and (want >= REG).sum() == k + 65, (k, n)
    return segs


# ---- K8c ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("cls", CLASSES)
def test_select_kernel_against_a_sort(probe, inputs, cls, k):
    # one CSR of every length, empty segments in the middle and at the end
    segs = [inputs[cls, k, n, 0] for n in CSR_ORDER]
    count, cand = probe.select(segs, k, shared=False)
    for q, d in enumerate(segs):
        check_segment(d, k, count[q], cand[q], (cls, k, "csr", q, d.size))
    # each length as a shared list: [nq][len]
    for n in LENGTHS:
        for nq in (1, 3):
            segs = [inputs[cls, k, n, v] for v in range(nq)]
            count, cand = probe.select(segs, k, shared=True)
            for q, d in enumerate(segs):
                check_segment(d, k, count[q], cand[q], (cls, k, "shared", nq, q, n))


@pytest.mark.parametrize("cls", CLASSES)
def test_select_model_against_the_same_sort(probe, inputs, cls):
    """host only (the probe's pf_probe_model calls prefilter_select_model): the model the CPU suite pins the heap rule against
    states what this file's reference states"""
    for k in KS:
        for n in LENGTHS:
            for v in range(VARIANTS):
                check_model(probe, inputs[cls, k, n, v], k, (cls, k, n, v))


# ---- K8b then K8c ------------------------------------------------------------------------------------------------------
DIST_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 513, 2049]
DIST_CSR_ORDER = [1, 15, 16, 0, 17, 63, 64, 65, 0, 127, 128, 129, 513, 2049, 0]
SHARED_LENGTHS = DIST_LENGTHS + [512, 1024]        # 8 and 16 tiles: multiples of the eight the shared grid rounds up to
N_ROWS = 300


def test_the_tile_counts_cover_multiples_of_eight_and_others(probe):
    tiles = [probe.lib.pf_probe_tiles(n) for n in SHARED_LENGTHS]
    assert tiles == [(n + 63) // 64 for n in SHARED_LENGTHS]
    assert any(t and t % 8 == 0 for t in tiles) and any(t % 8 for t in tiles) and any(t > 8 and t % 8 for t in tiles)


@pytest.mark.parametrize("metric", ["L2", "IP"])
@pytest.mark.parametrize("dim", [1, 16, 100, 768])
def test_distance_then_select(probe, oracle, dim, metric):
    rng = np.random.default_rng([dim, ord(metric[0])])
    stride = (dim + 63) // 64 * 64
    nq_max = max(9, len(DIST_CSR_ORDER))
    rows = np.zeros((N_ROWS, stride), np.float32)
    rows[:, :dim] = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    Q = np.zeros((nq_max, stride), np.float32)
    Q[:, :dim] = rng.standard_normal((nq_max, dim)).astype(np.float32)
    # the reference, once: the oracle's distance of every (query, row), on the very f32 values the kernel reads
    table = np.array([[oracle.distance(metric, rows[r, :dim], Q[q, :dim]) for r in range(N_ROWS)] for q in range(nq_max)], np.float32)
    assert not np.isnan(table).any()
    ks = [1, 10, 64]

    def check(lists, nq, k, shared, what):
        dist, count, cand = probe.distance_select(rows, np.ascontiguousarray(Q[:nq]), lists, metric == "L2", k, shared)
        at = 0
        for q in range(nq):
            idx = lists[0] if shared else lists[q]
            got = dist[at:at + idx.size]
            at += idx.size
            assert got.view(np.uint32).tolist() == table[q][idx].view(np.uint32).tolist(), (what, q, idx.size)   # every distance, bit for bit
            check_segment(table[q][idx], k, count[q], cand[q], (what, q, idx.size, k))
        assert at == dist.size

    lists = [rng.integers(0, N_ROWS, n).astype(np.uint32) for n in DIST_CSR_ORDER]            # slots repeat freely
    check(lists, len(lists), ks[dim % 3], False, (dim, metric, "csr"))
    run = 0
    for n in SHARED_LENGTHS:
        for nq in (1, 3, 8, 9):
            check([rng.integers(0, N_ROWS, n).astype(np.uint32)], nq, ks[run % 3], True, (dim, metric, "shared", nq))
            run += 1
