"""Option flat-l2-gemm through the C ABI: L2 batches answered by K4e (flat_l2_gemm_kernel, csrc/flat_l2_gemm.hip: a bound from the
matrix cores, exact distances for the pairs it leaves) against the CPU oracle per query -- labels equal, distance BITS equal -- and
against the same index with the option at 0 (the scan kernel).  vk_flat_l2_gemm_stats says which batches ran where.  One axis at a
time from n = 700, dim = 100, nq = 33, k = 10, Gaussian rows.

The gate must BIND for the GEMM, the norms and E to matter: with gemm-prepass-rows = 16 the pre-pass seeds finite bounds from 128
rows per 10 of k on, and wherever it ran on rows the bound can separate, fewer pairs than rows x queries may have been evaluated.
(Shifted rows are the exception by construction: E is some 3000 there against distances of 0.02, so a sound gate lets every pair
through -- what the case shows is that a finite bound loses no neighbour.)  Blocks walk several tiles only above 256 tiles per
query tile: the 30 000 / 70 000 / 150 000-row cases."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
OPT = "flat-l2-gemm"
BASE = dict(n=700, dim=100, nq=33, k=10, dtype="f32", rows="gauss", taken=True, prepass=16)
CASES = [dict(n=1), dict(n=255), dict(n=257),
         dict(n=70_000), dict(n=70_000, dtype="bf16"),                                # 274 tiles over 256 blocks, a ragged end (tile_q 64)
         dict(n=30_000, dim=768, nq=70), dict(n=30_000, dim=768, nq=70, dtype="bf16"),   # 118 tiles over 80 blocks x 3 query tiles (tile_q 32)
         dict(nq=5), dict(nq=31), dict(nq=65), dict(nq=70), dict(nq=4, taken=False),  # below kGemmMinQueries: refused
         dict(dim=50), dict(dim=768), dict(dim=1000), dict(dim=1856),                 # tile_q 64 / 32 / 24 / 16 (the last stride served)
         dict(dim=768, dtype="bf16"), dict(dim=1857, taken=False),                    # stride 1920: the first one refused
         dict(k=1), dict(k=11), dict(k=256), dict(n=4000, k=256), dict(k=257, taken=False), dict(n=100, k=200),   # k > n
         dict(dtype="bf16"), dict(rows="bitmap", prepass=32), dict(rows="removed"), dict(rows="duplicated"), dict(rows="shifted"),
         dict(rows="nonfinite"),
         dict(n=150_000, dim=128, nq=70, prepass=None)]                               # the default pre-pass: above 8 x its 16 384 rows


def bf16_round(x):
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: " ".join(f"{k}={v}" for k, v in c.items()))
def test_the_oracles_bits_and_the_scan_kernels(oracle, case):
    import _pkg
    vsa, O = _pkg.vsa, oracle
    c = {**BASE, **case}
    n, dim, nq, k = c["n"], c["dim"], c["nq"], c["k"]
    rng = np.random.default_rng([n, dim, nq, k])
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    kw = {}
    if c["rows"] == "duplicated":      # every row three times under different labels: ties at the k-th place, decided by label
        X = np.concatenate([X[:234]] * 3)
    labels = np.arange(len(X), dtype=np.uint64) * np.uint64(3) + np.uint64(10)
    if c["rows"] == "shifted":         # cancellation in |x|^2 + |q|^2 - 2 x.q far beyond the gaps between distances
        X, Q = (1000 + 0.01 * X).astype(np.float32), (1000 + 0.01 * Q).astype(np.float32)
    if c["rows"] == "nonfinite":
        X[3, 7], X[400, 99] = np.nan, np.inf
    if c["rows"] == "bitmap":          # a host bitmap that ends below the largest label
        nbits = int(labels[-1]) - 90
        kw = dict(allow=O.allow_bitmap(labels[(rng.random(len(X)) < 0.7) & (labels < nbits)], nbits), allow_nbits=nbits)
    ix = vsa.Index("FLAT", dim, "L2", initial_cap=len(X), device_id=0, dtype=c["dtype"])
    ix.add_batch(X, labels)
    gone = (0, 345, len(X) - 1) if c["rows"] == "removed" else ()
    assert all(ix.remove(int(labels[g])) == 0 for g in gone) and ix.get_option(OPT) == 0   # ships off
    pre = 16384
    if c["prepass"] is not None:
        ix.set_option("gemm-prepass-rows", c["prepass"])
        pre = c["prepass"]
    outs, moved = [], []
    for v in (1, 0):
        ix.set_option(OPT, v)
        s0 = ix.l2_gemm_stats()
        outs.append([np.ascontiguousarray(a) for a in ix.search_batch(Q, k, **kw)])
        s1 = ix.l2_gemm_stats()
        moved.append([getattr(s1, f) - getattr(s0, f) for f in ("launches", "queries", "rows", "evaluated", "declined")])
    live = len(X) - len(gone)
    evaluated = moved[0].pop(3)
    assert moved == [[1, nq, live, 0] if c["taken"] else [0, 0, 0, 1], [0, 0, 0, 0, 0]] and (evaluated > 0) == c["taken"]
    if c["taken"] and live >= 8 * pre * ((k + 9) // 10) and c["rows"] != "shifted":
        assert evaluated < live * nq, "the pre-pass ran and the gate pruned nothing"    # (the pre-pass's own pairs are in the count)
    (d, l, cnt), scan = outs
    assert all(a.tobytes() == b.tobytes() for a, b in zip(outs[0], scan))
    if c["rows"] != "nonfinite":       # (the oracle's order of NaN distances is not the contract; the scan kernel's answer is)
        o = O.Flat(dim, "L2", max_elements=len(X))
        o.add_many(bf16_round(X) if c["dtype"] == "bf16" else X, labels)
        for g in gone:
            o.remove(int(labels[g]))
        for q in range(nq):
            od, ol = o.search(Q[q], k, **kw)
            assert cnt[q] == ol.size and (l[q, :ol.size] == ol).all() and (d[q, :ol.size].view(np.uint32) == od.view(np.uint32)).all(), q
    ix.close()
