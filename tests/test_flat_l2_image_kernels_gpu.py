"""The early and the main pass of an f32 L2 index over the f16 image of the rows (option flat-l2-image; flat_filter_body with the
DMA row path and the half norms staged by its producers), through tests/helpers/filter_l2_image_probe.hip: row statistics, qprep
and both passes against bounds this test sets, once through registers (rows16 = nullptr) and once over the image, from a
workspace that holds a fill pattern.

  same survivors   the image holds what the register path converts and the half norms are the same words, so both paths keep the
                   same (row, score bits) per query -- no tolerance
  against float64  every pair whose float64 score (q.x - |x|^2 / 2) clears the bound by the column's margin at its tile's norm
                   (the polynomial qprep wrote) is among the survivors

Shapes: 128 t + 37 rows (a partial last tile) on four blocks (t = 1: two of them own no tile; every block's first tile belongs to
the early pass, the rest to the main pass), one and six stages of 64 (six: the ring of five row stages wraps), one query, two
full query tiles, and one column into the third."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

HELPERS = Path(__file__).resolve().parent / "helpers"
pytestmark = pytest.mark.gpu
FILLS = [0x00000000, 0xFFFFFFFF, 0x7F7FFFFF]
KEEP = 12                                                    # the bound of a query: its KEEP-th best float64 score


class Cfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_rows", "stride", "nq", "image", "cap", "blocks", "early_tiles", "fill")]


class IO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rows", "queries", "qbound", "tile_norm", "qcoef", "cnt", "cand")]


@pytest.fixture(scope="module")
def probe():
    lib = C.CDLL(str(HELPERS / "libfilterl2imageprobe.so"))
    lib.l2i_probe_passes.argtypes = [C.POINTER(Cfg), C.POINTER(IO)]
    lib.l2i_probe_passes.restype = C.c_int
    return lib


def _passes(probe, X, Q, bound, image, fill):
    """-> per query the set of (row, score bits), the tile norms and the margin polynomials"""
    n, dp = X.shape
    nq, nqt, n_tiles = Q.shape[0], (Q.shape[0] + 31) // 32, (n + 127) // 128
    cap = n
    qb = np.full(nqt * 32, np.inf, np.float32)
    qb[:nq] = bound
    tn = np.zeros(n_tiles + 2, np.uint32)
    qcoef = np.zeros((nqt * 32, 4), np.float32)
    cnt = np.zeros(nq, np.uint32)
    cand = np.zeros((2, nq, cap), np.uint32)
    cfg = Cfg(n, dp, nq, image, cap, 4, 1, fill)
    io = IO(*(a.ctypes.data for a in (X, Q, qb, tn, qcoef, cnt, cand)))
    rc = probe.l2i_probe_passes(C.byref(cfg), C.byref(io))
    assert rc == 0, rc
    assert (cnt <= cap).all()
    sets = [set(zip(cand[0, q, :cnt[q]].tolist(), cand[1, q, :cnt[q]].tolist())) for q in range(nq)]
    assert all(len(s) == int(c) for s, c in zip(sets, cnt)), "a pair was stored twice"
    return sets, tn[:n_tiles].view(np.float32), qcoef[:nq]


@pytest.mark.parametrize("nq", [1, 64, 65])
@pytest.mark.parametrize("dim", [64, 384])
@pytest.mark.parametrize("t", [1, 5, 12])
def test_image_and_register_path_keep_the_same_survivors(probe, t, dim, nq):
    n = 128 * t + 37
    rng = np.random.default_rng(1000 * t + dim + nq)
    X = (rng.standard_normal((n, dim)) * np.exp(rng.uniform(np.log(0.3), np.log(3.0), (n, 1)))).astype(np.float32)
    Q = np.ascontiguousarray(X[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, dim)), dtype=np.float32)
    X64 = X.astype(np.float64)
    score = Q.astype(np.float64) @ X64.T - 0.5 * (X64 * X64).sum(axis=1)[None, :]          # [nq][n], accumulator space
    bound = np.sort(score, axis=1)[:, -KEEP].astype(np.float32)
    for fill in FILLS:
        reg, tn, qcoef = _passes(probe, X, Q, bound, 0, fill)
        img, tn_i, qcoef_i = _passes(probe, X, Q, bound, 1, fill)
        assert (tn.view(np.uint32) == tn_i.view(np.uint32)).all() and (qcoef.view(np.uint32) == qcoef_i.view(np.uint32)).all()
        assert np.isfinite(tn).all() and (qcoef[:, 3] == 0).all()
        for q in range(nq):
            assert img[q] == reg[q], (hex(fill), q, sorted(img[q] ^ reg[q])[:4])
            assert all(row < n for row, _ in img[q])
        # float64: margin of column q at the norm of the row's tile, as the gate evaluates it (rounded up a little here)
        R = np.repeat(tn.astype(np.float64), 128)[:n]
        c2, c1, c0 = (qcoef[:, i].astype(np.float64)[:, None] for i in range(3))
        margin = ((c2 * R[None, :] + c1) * R[None, :] + c0) * (1 + 1e-6) + 2.0 ** -21 * np.maximum(1.0, np.abs(bound.astype(np.float64)))[:, None]
        must = score - margin >= bound.astype(np.float64)[:, None]
        assert must.sum() >= nq                                                       # (the check bites: somebody has to survive)
        for q in range(nq):
            rows = {row for row, _ in img[q]}
            missing = [r for r in np.flatnonzero(must[q]).tolist() if r not in rows]
            assert not missing, (hex(fill), q, missing[:4])
            # ... and what survived carries the approximate score of its pair: within the margin of float64
            for row, bits in img[q]:
                s = float(np.array([bits], np.uint32).view(np.float32)[0])
                assert abs(s - score[q, row]) <= margin[q, row], (q, row, s, score[q, row], margin[q, row])
