"""The kernels of the one-pass FLAT search for k > 1024 (csrc/flat_large_k.hip) on their own, through
tests/helpers/flat_large_k_probe.hip -- a small library that includes that translation unit, built with the library's flags, so
the product's kernels and launchers run, on buffers the test owns.

Every case runs three times, from output and scratch buffers filled with 0x00000000, 0xFFFFFFFF and 0x7F7FFFFF (the probe
zeroes the histogram bins, as the product does, and nothing else); every buffer comes back whole and the three results must be
equal word for word.

Distance: every candidate's bits equal the CPU oracle's distance, NaN sits exactly at the rows without a label and the rows the
bitmap rejects (labels at nbits - 1 and at nbits included), and the fill is intact at and beyond count, between the rows of
dist and behind the last one.  Select + emit: the state words (T, n_less, n_eq, n_real, counter, flag) equal the numpy model of
tests/helpers/flat_large_k_cases.py, the emitted set equals the model's, the fill is intact behind the entries, nothing is
written for a flagged query, and the histogram bins are left zeroed.  The probe polls the stream with a time limit."""
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
LIB = HERE / "libflatlargekprobe.so"
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]      # csrc/Makefile's
FILLS = (0x00000000, 0xFFFFFFFF, 0x7F7FFFFF)
PAD = 7

sys.path.insert(0, str(HERE))
sys.path.insert(0, str(ROOT))
import flat_large_k_cases as LK  # noqa: E402


def build_probe():
    src = HERE / "flat_large_k_probe.hip"
    deps = (src, HERE / "probe_common.hpp", CSRC / "flat_large_k.hip", CSRC / "flat_large_k_host.hpp", CSRC / "kernels.hpp",
            CSRC / "device_common.hpp")
    newest = max(p.stat().st_mtime for p in deps)
    if not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "-shared", "-fPIC", "-I", str(CSRC), str(src),
                               "-o", str(LIB)])
    return LIB


@pytest.fixture(scope="module")
def probe():
    lib = C.CDLL(str(build_probe()))
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    lib.lk_probe_distance.argtypes = [u32, i32, i32, i32, vp, u32, vp, u32, vp, u32, vp, u64, u64, u64, u64, vp]
    lib.lk_probe_distance.restype = i32
    lib.lk_probe_select_emit.argtypes = [u32, vp, vp, u32, u32, u64, u32, u32, u64, vp, vp, vp, vp]
    lib.lk_probe_select_emit.restype = i32
    for f in (lib.lk_probe_slice, lib.lk_probe_dist_blocks, lib.lk_probe_bins, lib.lk_probe_state_words):
        f.restype = u32
    lib.lk_probe_cap.argtypes = [u64]
    lib.lk_probe_cap.restype = u64
    return lib


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def test_the_probe_exports_the_restated_constants(probe):
    assert probe.lk_probe_slice() == LK.SLICE and probe.lk_probe_dist_blocks() == LK.DIST_BLOCKS
    assert probe.lk_probe_bins() == LK.BINS and probe.lk_probe_state_words() == LK.STATE_WORDS
    for k in (1, 1025, 4096, 4097, 10000, 100000):
        assert probe.lk_probe_cap(k) == LK.cap_of(k)


# ---- distance ----------------------------------------------------------------------------------------------------------------
N_TABLE, NQ_TABLE, QB = 1000, 9, 8
COUNTS = (1, 15, 16, 17, 63, 64, 65, 1000)
QCS = (1, QB - 1, QB, QB + 1)
SECOND_TRIP = LK.DIST_BLOCKS * 4 * 16 + 16 * 5 + 3     # every wave of the distance grid strides once; the last tile is partial


def bf16_round(x):
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def make_table(O, dim, space, bf16, n, nq):
    """rows (as the device holds them, zero padded to 16 elements), padded queries, table[q][row] = the oracle's distance"""
    stride = (dim + 15) // 16 * 16
    rng = np.random.default_rng([dim, int(bf16), n, nq, len(space)])
    X = (rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(np.float32)
    X = bf16_round(X) if bf16 else X
    Q = np.zeros((nq, stride), np.float32)
    Q[:, :dim] = rng.standard_normal((nq, dim)).astype(np.float32)
    o = O.Flat(dim, space, max_elements=n)
    o.add_many(X, np.arange(n, dtype=np.uint64))
    table = np.zeros((nq, n), np.float32)
    for q in range(nq):
        od, ol = o.search(Q[q, :dim], n)
        assert ol.size == n
        table[q, ol.astype(np.int64)] = od
    R = np.zeros((n, stride), np.float32)
    R[:, :dim] = X
    rows = (R.view(np.uint32) >> 16).astype(np.uint16) if bf16 else R
    return stride, np.ascontiguousarray(rows), Q, table.view(np.uint32)


def labels_and_filter(count, seed, with_filter=True):
    """labels: a permutation of 0 .. count - 1, every seventh row (and row 0 of a table of three or more) without a label;
    nbits = count - 1, so label count - 2 is the last one inside and label count - 1 the first outside"""
    rng = np.random.default_rng([count, seed, 3])
    lab = rng.permutation(count).astype(np.uint64)
    dead = (np.arange(count) % 7 == 3) | ((np.arange(count) == 0) & (count >= 3))
    lab[dead] = LK.NO_LABEL
    cand = ~dead
    if not with_filter:
        return lab, None, 0, cand
    nbits = max(count - 1, 1)
    on = rng.random(nbits) < 0.7
    on[nbits - 1] = True
    bits = np.zeros(nbits // 64 + 2, np.uint64)       # (a slack word of stray bits behind the filter's last word)
    idx = np.flatnonzero(on).astype(np.uint64)
    np.bitwise_or.at(bits, (idx >> np.uint64(6)).astype(np.int64), np.uint64(1) << (idx & np.uint64(63)))
    bits[(nbits + 63) // 64:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    if nbits % 64:
        bits[nbits // 64] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(nbits % 64)   # stray bits above nbits: ignored
    li = lab.astype(np.int64)
    inside = cand & (lab < np.uint64(nbits))
    cand = inside & on[np.where(inside, li, 0)]
    return lab, bits, nbits, cand


def run_distance(probe, fill, l2, bf16, qb, rows, stride, lab, count, Q, qc, bits, nbits, ld):
    words = qc * ld + PAD
    out = np.empty(words, np.uint32)
    rc = probe.lk_probe_distance(fill, l2, bf16, qb, rows.ctypes.data, stride, lab.ctypes.data, count, Q.ctypes.data, qc,
                                 None if bits is None else bits.ctypes.data, 0 if bits is None else len(bits), nbits, ld, words, out.ctypes.data)
    assert rc == 0, rc
    return out


def check_distance(out, fill, table_bits, cand, count, qc, ld):
    body = out[:qc * ld].reshape(qc, ld)
    assert np.all(body[:, count:] == fill) and np.all(out[qc * ld:] == fill)          # at and beyond count, between and behind the rows
    got = body[:, :count]
    assert np.all(LK.is_nan(got) == ~cand[None, :count]), np.argwhere(LK.is_nan(got) != ~cand[None, :count])[:4]
    sel = np.broadcast_to(cand[None, :count], got.shape)
    assert np.array_equal(got[sel], table_bits[:qc, :count][sel])


@pytest.mark.parametrize("bf16", (0, 1))
@pytest.mark.parametrize("space", ("L2", "IP"))
@pytest.mark.parametrize("dim", (1, 100, 257, 768))
def test_dense_distance_equals_the_oracle_from_dirty_buffers(probe, oracle, dim, space, bf16):
    stride, rows, Q, table = make_table(oracle, dim, space, bf16, N_TABLE, NQ_TABLE)
    for count in COUNTS:
        lab, bits, nbits, cand = labels_and_filter(count, dim)
        for qc in QCS:
            ld = count + (5 if qc % 2 else 0)          # ld == count, and rows of dist with a gap between them
            outs = [run_distance(probe, fill, int(space == "L2"), bf16, QB, rows, stride, lab, count, Q, qc, bits, nbits, ld) for fill in FILLS]
            for fill, out in zip(FILLS, outs):
                check_distance(out, fill, table, cand, count, qc, ld)


@pytest.mark.parametrize("qb,qc", [(1, 2), (2, 3), (4, 5)])
def test_dense_distance_with_smaller_query_blocks_and_no_filter(probe, oracle, qb, qc):
    stride, rows, Q, table = make_table(oracle, 100, "IP", 0, N_TABLE, NQ_TABLE)
    for count in (17, 1000):
        lab, bits, nbits, cand = labels_and_filter(count, qb, with_filter=False)
        for fill in FILLS:
            check_distance(run_distance(probe, fill, 0, 0, qb, rows, stride, lab, count, Q, qc, None, 0, count + 1), fill, table, cand, count, qc,
                           count + 1)


def test_dense_distance_where_every_wave_makes_a_second_trip(probe, oracle):
    count, dim = SECOND_TRIP, 1
    assert (count + 15) // 16 > LK.DIST_BLOCKS * 4
    stride, rows, Q, table = make_table(oracle, dim, "L2", 0, count, 2)
    lab, bits, nbits, cand = labels_and_filter(count, 1)
    for fill in FILLS:
        check_distance(run_distance(probe, fill, 1, 0, 2, rows, stride, lab, count, Q, 2, bits, nbits, count), fill, table, cand, count, 2, count)


# ---- select + emit -------------------------------------------------------------------------------------------------------------
def run_select(probe, fill, dist, lab, count, k, cap):
    qc = dist.shape[0]
    entries = qc * cap + PAD
    state = np.empty(qc * LK.STATE_WORDS, np.uint32)
    hist = np.empty(qc * LK.BINS, np.uint32)
    ob, ol = np.empty(entries, np.uint32), np.empty(entries, np.uint64)
    d = np.ascontiguousarray(dist)
    rc = probe.lk_probe_select_emit(fill, d.ctypes.data, lab.ctypes.data, count, qc, d.shape[1], k, cap, entries, state.ctypes.data,
                                    hist.ctypes.data, ob.ctypes.data, ol.ctypes.data)
    assert rc == 0, rc
    return state.reshape(qc, LK.STATE_WORDS), hist, ob, ol


@pytest.mark.parametrize("size", list(LK.COUNTS))
def test_select_and_emit_equal_the_model_from_dirty_buffers(probe, size):
    count = LK.COUNTS[size]
    for k in LK.ks(count):
        cap = LK.cap_of(k)
        made, dist, lab = LK.case(count, k)
        ld = count + 3
        padded = np.full((dist.shape[0], ld), 0x7F7FFFFF, np.uint32)       # (finite words behind count: never read)
        padded[:, :count] = dist
        want = [LK.model(dist[q], lab, k, cap) for q in range(len(made))]
        for fill in FILLS:
            fill64 = np.uint64(fill | (fill << 32))
            state, hist, ob, ol = run_select(probe, fill, padded, lab, count, k, cap)
            assert not hist.any()
            assert np.all(ob[len(made) * cap:] == fill) and np.all(ol[len(made) * cap:] == fill64)
            for q, cls in enumerate(made):
                ws, wb, wl = want[q]
                assert state[q].tolist() == ws, (cls, k, state[q].tolist(), ws)
                n = len(wb)
                gb, gl = ob[q * cap:(q + 1) * cap], ol[q * cap:(q + 1) * cap]
                assert np.all(gb[n:] == fill) and np.all(gl[n:] == fill64), (cls, k)      # behind the entries; a flagged query: all of it
                a, b = LK.canon(gb[:n], gl[:n]), LK.canon(wb, wl)
                assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0]), (cls, k)
