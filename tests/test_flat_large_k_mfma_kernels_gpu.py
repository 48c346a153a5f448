"""flat_dense_mfma_kernel (csrc/flat_large_k.hip, option flat-large-k-mfma) through tests/helpers/flat_large_k_mfma_probe.hip.

Per case the whole buffer -- [qc][ld] and 64 guard words, filled with 0xEEEEEEEE -- is bit-equal to flat_dense_distance_kernel's; a
candidate's distance is bit-equal to the oracle's IP distance on the very f32 (or bf16-rounded) values the kernel reads; a row
without a label or rejected by the bitmap is NaN for every query; [count, ld) of every query and the guard still hold the fill.
f32 rows also: |d - (1 - x.q in f64)| <= D * 2^-23 for unit vectors (each of the D fmaf steps adds at most half an ulp of a partial
sum of at most 1).  One axis at a time against a default, plus two corners.  BIG has more 128-row tiles than the launch has row
partitions (asserted from the launcher's own answer) and a ragged last tile.  No NaN / inf / denormal inputs for bit equality; one
NaN in a row: NaN where the vector kernel has NaN."""
import ctypes as C
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N_ROWS, NQ_MAX, GUARD, FILL, NO_LABEL, BIG = 131, 70, 64, 0xEEEEEEEE, 2 ** 64 - 1, 128 * 129 + 5
DIM = {64: 50, 128: 100, 768: 768, 896: 896, 1664: 1664, 1728: 1728}   # 896: a 24-query tile; 1664: the longest; 1728: declined
DEFAULT = dict(count=129, qc=33, stride=128, pad=0, mask="none", bf16=False)
CASES = ([dict(count=n) for n in (1, 31, 32, 33, 127, 128, BIG)] + [dict(qc=n) for n in (5, 31, 32, 70)] +
         [dict(stride=s) for s in (64, 768, 896, 1664, 1728)] + [dict(pad=37)] + [dict(mask=m) for m in ("holes", "bitmap", "both")] +
         [dict(bf16=True), dict(bf16=True, stride=768, qc=70, count=127, mask="both", pad=37), dict(),
          dict(count=BIG, qc=70, stride=768, mask="both", pad=37), dict(nan=True)])


@pytest.fixture(scope="module")
def probe():
    lib = C.CDLL(str(Path(__file__).resolve().parent / "helpers" / "libflatlargekmfmaprobe.so"))   # one of build()'s products
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.lkm_probe_distance.argtypes = [u32, C.c_int, C.c_int, C.c_int, vp, u32, vp, u32, vp, u32, vp, u64, u64, u64, u64, vp]
    lib.lkm_probe_takes.argtypes = [u32, u32]
    lib.lkm_probe_nrp.argtypes = [u32, u32, u32]
    lib.lkm_probe_nrp.restype = u32
    return lib


@lru_cache(maxsize=None)
def world(stride, bf16):
    """131 rows as the kernel reads them, queries, and the reference, once: the oracle's distance of every (query, row) and the f64 one"""
    from oracle import oracle as O
    dim = DIM[stride]
    rng = np.random.default_rng([stride, int(bf16)])
    unit = lambda n: np.stack([O.normalize(v)[0] for v in rng.standard_normal((n, dim)).astype(np.float32)])
    rows, Q = np.zeros((N_ROWS, stride), np.float32), np.zeros((NQ_MAX, stride), np.float32)
    rows[:, :dim], Q[:, :dim] = unit(N_ROWS), unit(NQ_MAX)
    dev = rows
    if bf16:   # round to nearest even, as the index does at ingest
        u = rows.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        rows, dev = u.astype(np.uint32).view(np.float32), np.ascontiguousarray((u >> 16).astype(np.uint16))
    table = np.array([[O.distance("IP", rows[r, :dim], Q[q, :dim]) for r in range(N_ROWS)] for q in range(NQ_MAX)], np.float32)
    return dev, Q, table, 1.0 - Q.astype(np.float64) @ rows.astype(np.float64).T


def run(probe, mfma, dev, stride, labels, Q, allow, nbits, ld, bf16):
    out = np.zeros(Q.shape[0] * ld + GUARD, np.uint32)
    rc = probe.lkm_probe_distance(FILL, mfma, int(bf16), 4, dev.ctypes.data, stride, labels.ctypes.data, labels.size, Q.ctypes.data, Q.shape[0],
                                  None if allow is None else allow.ctypes.data, 0 if allow is None else allow.size, nbits, ld, out.size, out.ctypes.data)
    assert rc == 0, {1: "the probe refused its arguments", 2: "time limit"}.get(rc, f"HIP error seen at flat_large_k_mfma_probe.hip:{rc}")
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()) or "default")
def test_dense_mfma_bits(probe, case):
    c = dict(DEFAULT, **case)
    count, qc, stride, bf16, ld = c["count"], c["qc"], c["stride"], c["bf16"], c["count"] + c["pad"]
    assert probe.lkm_probe_takes(stride, qc) == (stride != 1728) and probe.lkm_probe_takes(stride, 4) == 0
    if stride == 1728:   # the first stride the kernel cannot hold: the decision declines, there is no grid, nothing is launched
        assert probe.lkm_probe_nrp(count, stride, qc) == 0
        return
    if count == BIG:
        assert (count + 127) // 128 > probe.lkm_probe_nrp(count, stride, qc) >= 8 and count % 128 != 0
    dev, Q, table, table64 = world(stride, bf16)
    src = np.arange(count) % N_ROWS                                      # row r of the table is row r % 131 of the world
    dev, Q = np.ascontiguousarray(dev[src]), np.ascontiguousarray(Q[:qc])
    rng = np.random.default_rng(count * 1000 + qc)
    labels = np.arange(count, dtype=np.uint64) * np.uint64(3) + np.uint64(2)
    cand, allow, nbits = np.ones(count, bool), None, 0
    if c["mask"] in ("holes", "both"):                                   # rows without a label: the first, the last, a tenth of the others
        holes = np.unique(np.concatenate([[0, count - 1], np.flatnonzero(rng.random(count) < 0.1)]))
        labels[holes], cand[holes] = NO_LABEL, False
    if c["mask"] in ("bitmap", "both"):                                  # a bitmap that ends below the largest label
        nbits = 3 * count - 30
        allow = rng.integers(0, 2 ** 64, (nbits + 63) // 64, dtype=np.uint64)
        lab = np.minimum(labels, np.uint64(nbits - 1)).astype(np.int64)
        cand &= (labels < nbits) & (((allow[lab >> 6] >> (lab & 63).astype(np.uint64)) & np.uint64(1)) == 1)
    if c.get("nan"):
        dev = dev.copy()
        dev[3, 17] = np.nan
    m1, m0 = (run(probe, m, dev, stride, labels, Q, allow, nbits, ld, bf16) for m in (1, 0))
    body1, body0 = m1[:-GUARD].reshape(qc, ld), m0[:-GUARD].reshape(qc, ld)
    assert np.all(m1[-GUARD:] == FILL) and np.all(body1[:, count:] == FILL), "a word at or beyond count was written"
    got = body1[:, :count].view(np.float32)
    if c.get("nan"):
        nan0 = np.isnan(body0[:, :count].view(np.float32))
        assert nan0[:, 3].all() and nan0.sum() == qc and np.array_equal(np.isnan(got), nan0)
        assert np.array_equal(body1[:, :count][~nan0], body0[:, :count][~nan0])
        return
    assert np.array_equal(m1, m0), "the matrix-core kernel against the vector kernel"
    assert np.isnan(got[:, ~cand]).all() and not np.isnan(got[:, cand]).any()
    assert np.array_equal(got[:, cand].view(np.uint32), table[:qc][:, src][:, cand].view(np.uint32)), "the matrix-core kernel against the oracle"
    if not bf16:
        assert np.abs(got[:, cand].astype(np.float64) - table64[:qc][:, src][:, cand]).max(initial=0.0) <= DIM[stride] * 2.0 ** -23
