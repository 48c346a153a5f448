"""The device sort of the one-pass FLAT search's hand-back (csrc/flat_large_k.hip: tile sort, merge passes, dense output) on its
own, through tests/helpers/flat_large_k_sort_probe.hip, which includes that translation unit and is built with the library's
flags.  The test writes what the emit leaves (state words, distance bits, labels: one query per value class) itself.

Every case runs from a second buffer pair and a dense hand-back filled with 0x00000000, 0xFFFFFFFF and 0x7F7FFFFF.  Against ONE
numpy statement, np.lexsort((label, key)) cut at min(k, n): the dense labels and distance bits are equal word for word, the fill
is intact behind them and behind n in the second pair, the state words are unchanged, and the emit's buffers hold in [0, n)
the entries they held (the tile sort works in place, so their order may change; with cap within one tile they are untouched)
and behind n every word they held.  Nothing of a flagged query is touched."""
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
LIB = HERE / "libflatlargeksortprobe.so"
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]      # csrc/Makefile's
FILLS = (0x00000000, 0xFFFFFFFF, 0x7F7FFFFF)
T, PAD = 4096, 5
CLASSES = ("random", "one_key", "label_bits", "pm_zero", "plus_inf", "ordered", "reversed", "tie_edges")
NS = (0, 1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5, 5 * T + 17, 33 * T + 3)

sys.path.insert(0, str(HERE))
import flat_large_k_cases as LK  # noqa: E402


@pytest.fixture(scope="module")
def probe():
    src = HERE / "flat_large_k_sort_probe.hip"
    deps = (src, HERE / "probe_common.hpp", CSRC / "flat_large_k.hip", CSRC / "flat_large_k_host.hpp", CSRC / "kernels.hpp", CSRC / "device_common.hpp")
    if not LIB.exists() or LIB.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "-shared", "-fPIC", "-I", str(CSRC), str(src), "-o", str(LIB)])
    lib = C.CDLL(str(LIB))
    lib.lks_probe_sort.argtypes = [C.c_uint32] * 4 + [C.c_uint64] * 2 + [C.c_void_p] * 7
    lib.lks_probe_passes.argtypes = [C.c_uint64]
    assert lib.lks_probe_tile() == T
    return lib


def entries(cls, n, seed):
    """one query's emitted (distance bits, labels), n of each, in the order the emit is said to have left them"""
    rng = np.random.default_rng([n, seed, CLASSES.index(cls)])
    lab = LK.labels_for(max(n, 1), seed)[:n]
    f = rng.permutation(np.unique(rng.standard_normal(2 * n + 8).astype(np.float32)))[:n]      # distinct, both signs
    if cls == "one_key":
        f[:] = -2.5
    elif cls == "label_bits":          # four keys; the eight labels of a group differ in bits 63, 32 and 31 only
        i = np.arange(n, dtype=np.uint64)
        lab = rng.permutation((i >> np.uint64(3)) | ((i & np.uint64(1)) << np.uint64(63)) | ((i & np.uint64(2)) << np.uint64(31)) | ((i & np.uint64(4)) << np.uint64(29)))
        f = rng.integers(0, 4, n).astype(np.float32)
    elif cls == "pm_zero":
        z = rng.random(n)
        f[z < 0.4], f[z > 0.6] = 0.0, -0.0
    elif cls == "plus_inf":
        f[rng.random(n) < 0.3] = np.inf
    elif cls == "ordered":
        f = np.sort(f)
    elif cls == "reversed":
        f = np.sort(f)[::-1].copy()
    elif cls == "tie_edges":           # by rank: 80 entries share a key around every multiple of the tile (block edges, merge splits)
        rank = np.arange(n)
        for e in range(T, n, T):
            rank[e - 40:e + 40] = e - 40
        f = rng.permutation((rank - n // 2).astype(np.float32))
    return np.ascontiguousarray(f).view(np.uint32).copy(), lab


def run(probe, fill, qc, k, cap, state, bits, label):
    le, de = qc * cap + PAD, qc * k + PAD
    st, b, l = state.copy(), bits.copy(), label.copy()
    b2, l2, db, dl = np.empty(le, np.uint32), np.empty(le, np.uint64), np.empty(de, np.uint32), np.empty(de, np.uint64)
    rc = probe.lks_probe_sort(fill, qc, k, cap, le, de, *(x.ctypes.data for x in (st, b, l, b2, l2, db, dl)))
    assert rc == 0, rc
    return st, b, l, b2, l2, db, dl


def check(probe, ns, flags, k, cap, seed=0):
    """queries of ns[q] entries each (flags[q]: flagged by the select), one probe call per fill"""
    qc = len(ns)
    rng = np.random.default_rng([k, cap, seed])
    bits = rng.integers(0, 1 << 32, qc * cap + PAD, dtype=np.uint32)               # whatever lies behind n: any words
    label = rng.integers(0, 1 << 63, qc * cap + PAD, dtype=np.uint64)
    state = np.zeros((qc, LK.STATE_WORDS), np.uint32)
    for q, n in enumerate(ns):
        bits[q * cap:q * cap + n], label[q * cap:q * cap + n] = entries(CLASSES[q % len(CLASSES)], n, seed)
        state[q] = [0x80000000, 1, n // 3, n - n // 3, n, n, flags[q], 0]
    outs = [run(probe, fill, qc, k, cap, state, bits, label) for fill in FILLS]
    for fill, (st, b, l, b2, l2, db, dl) in zip(FILLS, outs):
        fill64 = np.uint64(fill | (fill << 32))
        assert np.array_equal(st, state) and np.array_equal(b, outs[0][1]) and np.array_equal(l, outs[0][2])
        assert np.all(db[qc * k:] == fill) and np.all(dl[qc * k:] == fill64) and np.all(b2[qc * cap:] == fill) and np.all(l2[qc * cap:] == fill64)
        for q, n in enumerate(ns):
            s, gb, gl = slice(q * cap, (q + 1) * cap), bits[q * cap:q * cap + n], label[q * cap:q * cap + n]
            m = 0 if flags[q] else min(k, n)
            order = np.lexsort((gl, LK.key_of(gb)))[:m]                              # THE statement: by key, then label
            assert np.array_equal(dl[q * k:q * k + m], gl[order]) and np.array_equal(db[q * k:q * k + m], gb[order]), (q, n, k, fill)
            assert np.all(db[q * k + m:(q + 1) * k] == fill) and np.all(dl[q * k + m:(q + 1) * k] == fill64), (q, n, k)
            written = 0 if flags[q] else n
            assert np.all(b2[s][written:] == fill) and np.all(l2[s][written:] == fill64), (q, n, k)
            assert np.array_equal(b[s][n:], bits[s][n:]) and np.array_equal(l[s][n:], label[s][n:])
            if flags[q] or cap <= T:
                assert np.array_equal(b[s], bits[s]) and np.array_equal(l[s], label[s])
            else:                                                                    # labels are distinct: the same entries by label
                o0, o1 = np.argsort(gl), np.argsort(l[s][:n])
                assert np.array_equal(l[s][:n][o1], gl[o0]) and np.array_equal(b[s][:n][o1], gb[o0])


@pytest.mark.parametrize("n", NS)
def test_sorted_hand_back_equals_lexsort_from_dirty_buffers(probe, n):
    ks = sorted({k for k in (1, n - 1, n, n + 1, T // 2 + 3 if n > T else 0) if k >= 1})
    for k in ks:
        check(probe, [n] * len(CLASSES), [0] * len(CLASSES), k, max(n, 1))
    check(probe, [n] * len(CLASSES), [0] * len(CLASSES), ks[-1], max(n, 1) + 3)      # cap just beyond n: a pass more at n = T, 2T


@pytest.mark.parametrize("flagged", (1, 2))
@pytest.mark.parametrize("cap", (2 * T + 1, 9 * T + 7))       # ... and a cap that is no multiple of the tile, well above n: four passes
def test_three_queries_one_flagged(probe, cap, flagged):
    assert probe.lks_probe_passes(cap) == (2 if cap == 2 * T + 1 else 4)
    for k in (T - 1, 2 * T + 1, 3 * T):
        check(probe, [0, 2 * T + 1, T - 1], [int(q == flagged) for q in range(3)], k, cap, seed=flagged)
