"""K8m (prefilter_mfma_kernel, csrc/prefilter_select.hip) through tests/helpers/prefilter_mfma_probe.hip: the distances of a
shared list from the matrix cores against K8b's and the oracle's.

Per case: K8m's output is bit-equal to the oracle's inner-product distance on the very f32 (or bf16-rounded) values the kernel
reads and to K8b's output, and the 64 guard words behind it still hold 0xEEEEEEEE.  f32 rows also: |d - (1 - x.q in f64)| <=
D * 2^-23 for unit vectors -- derived: each of the D fmaf steps adds at most half an ulp of a partial sum of at most 1.
Every value of one axis against a default for the others, plus two corners.  BIG makes a block walk two tiles: with 256 CUs and
two (three) query tiles the grid has 128 (80) row partitions, BIG has 130 tiles, the last one ragged.  No NaN / inf / denormal
inputs for bit equality (what the matrix cores do with denormal products is not established); one NaN row: NaN where K8b has NaN."""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = Path(__file__).resolve().parent / "helpers"
N_ROWS, NQ_MAX, GUARD = 131, 70, 64
BIG = 128 * 129 + 5
DIM = {64: 50, 128: 100, 768: 768, 896: 896, 1664: 1664, 1728: 1728}   # 896: a 24-query tile; 1664: the longest; 1728: K8b's
DEFAULT = dict(shared_len=129, nq=33, stride=128, idx="random", bf16=False)
CASES = ([dict(shared_len=n) for n in (1, 31, 32, 33, 127, 128, BIG)] + [dict(nq=n) for n in (5, 31, 32, 70)] +
         [dict(stride=s) for s in (64, 768, 896, 1664, 1728)] + [dict(idx=i) for i in ("ascending", "descending", "same", "ends")] +
         [dict(bf16=True), dict(bf16=True, stride=768, nq=70, shared_len=127), dict(),   # (the stride axis holds the corner 129, 33, 64)
          dict(shared_len=BIG, nq=70, stride=768), dict(nan=True)])


@pytest.fixture(scope="module")
def probe():
    lib = C.CDLL(str(HERE / "libprefiltermfmaprobe.so"))   # one of build()'s products
    vp, u32 = C.c_void_p, C.c_uint32
    lib.pm_probe_distance.argtypes = [vp, u32, u32, vp, u32, vp, u32, C.c_int, u32, vp]
    lib.pm_probe_takes.argtypes = [u32, u32]
    lib.pm_probe_tile_q.argtypes = [u32]
    lib.pm_probe_tile_q.restype = u32
    return lib


@lru_cache(maxsize=None)
def world(stride, bf16):
    """rows as the kernel reads them, queries, and the reference, once: the oracle's distance of every (query, row) and the f64 one"""
    from oracle import oracle as O
    dim = DIM[stride]
    rng = np.random.default_rng([stride, int(bf16)])
    unit = lambda n: np.stack([O.normalize(v)[0] for v in rng.standard_normal((n, dim)).astype(np.float32)])
    rows = np.zeros((N_ROWS, stride), np.float32)
    rows[:, :dim] = unit(N_ROWS)
    Q = np.zeros((NQ_MAX, stride), np.float32)
    Q[:, :dim] = unit(NQ_MAX)
    dev = rows
    if bf16:   # round to nearest even, as the index does at ingest
        u = rows.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        rows = u.astype(np.uint32).view(np.float32)
        dev = np.ascontiguousarray((u >> 16).astype(np.uint16))
    table = np.array([[O.distance("IP", rows[r, :dim], Q[q, :dim]) for r in range(N_ROWS)] for q in range(NQ_MAX)], np.float32)
    table64 = 1.0 - Q.astype(np.float64) @ rows.astype(np.float64).T
    return dev, Q, table, table64


def run(probe, dev, stride, Q, idx, bf16, mfma):
    out = np.zeros(Q.shape[0] * idx.size + GUARD, np.uint32)
    rc = probe.pm_probe_distance(dev.ctypes.data, N_ROWS, stride, Q.ctypes.data, Q.shape[0], idx.ctypes.data, idx.size, int(bf16), mfma,
                                 out.ctypes.data)
    assert rc == 0, f"HIP error seen at prefilter_mfma_probe.hip:{rc}" if rc > 1 else "the probe refused its arguments"
    assert np.all(out[-GUARD:] == 0xEEEEEEEE), "a guard word was written"
    return out[:-GUARD].reshape(Q.shape[0], idx.size)


@pytest.mark.parametrize("case", CASES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()) or "default")
def test_k8m_bits(probe, case):
    c = dict(DEFAULT, **case)
    n, nq, stride, bf16 = c["shared_len"], c["nq"], c["stride"], c["bf16"]
    dev, Q, table, table64 = world(stride, bf16)
    rng = np.random.default_rng(n * 1000 + nq)
    idx = {"random": rng.integers(0, N_ROWS, n), "ascending": np.sort(rng.integers(0, N_ROWS, n)),
           "descending": np.sort(rng.integers(0, N_ROWS, n))[::-1], "same": np.full(n, 77),
           "ends": np.resize([0, N_ROWS - 1, N_ROWS - 1, 0, 5], n)}[c["idx"]]
    idx, Q = np.ascontiguousarray(idx, np.uint32), np.ascontiguousarray(Q[:nq])
    assert probe.pm_probe_takes(stride, nq) == (stride != 1728)                    # 1728: the first stride K8m does not hold
    assert (probe.pm_probe_tile_q(896), probe.pm_probe_tile_q(1664), probe.pm_probe_tile_q(1728)) == (24, 16, 0)
    if c.get("nan"):
        dev = dev.copy()
        dev[idx[3], 17] = np.nan
        m1, m0 = (run(probe, dev, stride, Q, idx, bf16, m).view(np.float32) for m in (1, 0))
        assert np.isnan(m0[:, idx == idx[3]]).all() and (np.isnan(m1) == np.isnan(m0)).all()
        keep = ~np.isnan(m0)
        assert m1[keep].view(np.uint32).tolist() == m0[keep].view(np.uint32).tolist()
        return
    m1, m0 = run(probe, dev, stride, Q, idx, bf16, 1), run(probe, dev, stride, Q, idx, bf16, 0)
    want = table[:nq][:, idx]
    assert not np.isnan(want).any()
    assert np.array_equal(m1, want.view(np.uint32)), "K8m against the oracle"
    assert np.array_equal(m1, m0), "K8m against K8b"
    if not bf16:
        assert np.abs(m1.view(np.float32).astype(np.float64) - table64[:nq][:, idx]).max() <= DIM[stride] * 2.0 ** -23
