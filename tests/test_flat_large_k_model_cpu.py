"""The numpy model behind tests/test_flat_large_k_kernels_gpu.py (tests/helpers/flat_large_k_cases.py) without a device: its one
sorting statement against Python's sorted over (float compare with -0 == +0, label), and a census showing that every case
reaches the path it is named for -- a case that no longer does would let a broken kernel pass."""
import struct
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import flat_large_k_cases as LK  # noqa: E402


def as_float(bits):
    return struct.unpack("<f", struct.pack("<I", int(bits)))[0]


def python_model(bits, labels, k, cap):
    real = [(as_float(b), int(l), int(b)) for b, l in zip(bits, labels) if as_float(b) == as_float(b)]
    real = sorted(real, key=lambda e: (e[0], e[1]))       # Python's float compare: -0.0 == 0.0, then the label
    if not real:
        return None, 0, 0, 0, []
    t = real[min(k, len(real)) - 1][0]
    less = [e for e in real if e[0] < t]
    eq = [e for e in real if e[0] == t]
    took = [] if len(less) + len(eq) > cap else sorted((e[1], e[2]) for e in less + eq)
    return t, len(less), len(eq), len(real), took


def test_the_numpy_statement_against_sorted():
    for count in (1, 37, 700):
        for k in LK.ks(count) + [5]:
            made, dist, lab = LK.case(count, k, seed=1)
            cap = min(LK.cap_of(k), 40)        # (a small cap, so that flagged queries occur at these sizes too)
            for q, cls in enumerate(made):
                state, wb, wl = LK.model(dist[q], lab, k, cap)
                t, n_less, n_eq, n_real, took = python_model(dist[q], lab, k, cap)
                assert state[2:5] == [n_less, n_eq, n_real], (cls, count, k)
                if n_real:
                    t_bits = struct.unpack("<I", struct.pack("<f", t))[0]
                    assert state[0] == int(LK.key_of(np.array([t_bits], np.uint32))[0])
                assert state[6] == int(n_less + n_eq > cap)
                assert sorted(zip(wl.tolist(), wb.tolist())) == took, (cls, count, k)


def test_keys_order_like_floats_and_zeros_share_a_key():
    f = np.array([-np.inf, -3.0, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    key = LK.key_of(f.view(np.uint32))
    assert key[3] == key[4] and np.all(np.diff(key.astype(np.int64))[[0, 1, 2, 4, 5, 6]] > 0)
    assert LK.is_nan(np.array([LK.NAN_POS, LK.NAN_NEG, 0x7F800000, 0xFF800000], np.uint32)).tolist() == [True, True, False, False]


def test_census_every_case_reaches_its_path():
    seen = {c: 0 for c in LK.CLASSES}
    flagged = exact_fit = short = two_slices = 0
    for size, count in LK.COUNTS.items():
        assert LK.ks(count)[0] == 1 and (count + 1) in LK.ks(count)
        for k in LK.ks(count):
            cap = LK.cap_of(k)
            made, dist, lab = LK.case(count, k)
            assert len(set(lab.tolist())) == count
            for q, cls in enumerate(made):
                seen[cls] += 1
                st, wb, wl = LK.model(dist[q], lab, k, cap)
                key = LK.key_of(dist[q])
                if cls == "tie_past":
                    assert st[6] == 1 and st[2] + st[3] == cap + 1 and st[2] < k <= st[2] + st[3]
                if cls == "tie_inside" and count >= cap:
                    assert st[6] == 0 and st[2] + st[3] == cap and st[2] < k
                    exact_fit += 1
                if cls == "fewer":
                    assert 0 < st[4] < k and st[2] + st[3] == st[4]
                    short += 1
                if cls == "none":
                    assert st == [0] * 8
                if cls == "negative":
                    assert np.all(key < 0x80000000)
                if cls == "pm_zero" and count >= 100:
                    b = dist[q]
                    assert (b == 0).any() and (b == 0x80000000).any()
                if cls == "plus_inf" and k >= count >= 100:
                    assert st[0] == 0xFF800000
                if cls == "nan_ends":
                    assert LK.is_nan(dist[q][[0, count // 2, count - 1]]).all() and st[4] >= count - 3
                if cls == "low_digit":
                    assert np.all(key >> 10 == key[0] >> 10) and (count < 100 or len(set((key & 1023).tolist())) > 50)
                if cls == "high_digit":
                    assert np.all(key & ((1 << 21) - 1) == (key[0] & ((1 << 21) - 1))) and (count < 100 or len(set((key >> 21).tolist())) > 50)
                flagged += st[6]
            two_slices += count > LK.SLICE
    assert all(seen.values()), seen
    assert flagged >= 5 and exact_fit >= 3 and short >= 5 and two_slices >= 5
    assert LK.COUNTS["slice"] == LK.SLICE and LK.COUNTS["slice-1"] == LK.SLICE - 1 and LK.COUNTS["slice+1"] == LK.SLICE + 1


def test_the_plan_restated():
    assert LK.plan(9, 5000, 2500, 1 << 30) == (True, 5056, 8, 2)
    assert LK.plan(9, 5000, 2500, 5056 * 4 - 1)[0] is False and LK.plan(1, 5000, 2500, 5056 * 4) == (True, 5056, 1, 1)
    assert LK.plan(33, 5000, 5000, 1 << 30) == (True, 5056, 32, 2)
