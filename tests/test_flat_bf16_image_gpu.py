"""The 16-bit image of an f32 index's rows in its two number formats (option flat-image-format: 0 = f16, 1 = bf16) and the bf16
index's filter passes over a bf16 image.

  image bits    row_stats_kernel through tests/helpers/bf16_image_probe.hip: every element the numpy restatement of round to
                nearest even, padding zero, nothing written outside the rows asked for, non-finite rows open their tile
  margin audit  the launches FlatIndex::scan_filter makes for an f32 index behind a bf16 image, on random and on adversarial
                inputs (both operands just past bf16 rounding midpoints, all errors adding: tests/helpers/bf16_image_cases.py),
                every stage against float64
  C ABI         format 0, format 1 and the f32 rows (flat-f16-image = 0) answer byte for byte alike, and like the CPU oracle

The C-ABI cases use the smallest indexes the candidate filter serves at all -- 8 x 1024 rows per ten of k (FlatIndex::search:
count >= 8 * filter_prepass_rows(k)), i.e. 9 000 rows up to k = 10 and 58 000 at k = 64; an index of 3 000 rows is answered by
the exact kernels whatever the option says (one such case is kept: same answers, no filter pass).
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

HELPERS = Path(__file__).resolve().parent / "helpers"
sys.path.insert(0, str(HELPERS))
import bf16_image_cases as BC  # noqa: E402

pytestmark = pytest.mark.gpu
INF_BITS = 0x7F800000
OPTS = {"filter-prepass-rows": 1024, "filter-min-rows": 0, "filter-two-pass-min-tiles": 2}


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


class Cfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_rows", "stride", "nq", "k", "format", "mfma16", "cap", "sample_rows", "blocks", "early_tiles", "fill")]


class IO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rows", "queries", "tile_norm", "stats", "thr", "qbound_select", "smax", "cnt", "cand", "layout")]


@pytest.fixture(scope="module")
def probe():
    lib = C.CDLL(str(HELPERS / "libbf16imageprobe.so"))
    lib.bi_probe_image.argtypes = [C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 3
    lib.bi_probe_image.restype = C.c_int
    lib.bi_probe_chain.argtypes = [C.POINTER(Cfg), C.POINTER(IO)]
    lib.bi_probe_chain.restype = C.c_int
    return lib


def _ptr(a):
    return a.ctypes.data


def _pad(x, dp):
    out = np.zeros((x.shape[0], dp), np.float32)
    out[:, :x.shape[1]] = x
    return out


# ---- image bits ------------------------------------------------------------------------------------------------------------
SPECIAL_BITS = np.array([
    0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,   # midpoints on both sides of an even / odd kept bit
    0xBF808000, 0xBF818000, 0xBF808001, 0xBF817FFF,
    0x3FFF8000, 0x3FFFFFFF,                                                    # the carry into the exponent
    0x00000000, 0x80000000, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,   # +-0, f32 subnormals
    0x33808000, 0x46FF8000,                                                    # midpoints far down and just below 32768
], dtype=np.uint32)


def _image(probe, x, dp, lo, hi, fmt, fill):
    n = x.shape[0]
    n_tiles = (n + 127) // 128
    alloc = n_tiles * 128 + 256
    tn = np.zeros(n_tiles + 2, np.uint32)
    st = np.zeros(16, np.uint32)
    img = np.zeros((alloc, dp), np.uint16)
    rc = probe.bi_probe_image(_ptr(x), dp, n, lo, hi, fmt, fill, _ptr(tn), _ptr(st), _ptr(img))
    assert rc == 0, rc
    return tn, st, img


@pytest.mark.parametrize("dim", [1, 100, 257, 768])
def test_image_bits(probe, dim):
    dp = (dim + 63) // 64 * 64
    rng = np.random.default_rng(dim)
    fills = (0x00000000, 0xFFFFFFFF, 0x7F7FFFFF)
    for n in (1, 127, 128, 129, 300):
        x = _pad((rng.standard_normal((n, dim)) * np.exp(rng.uniform(-6, 6, (n, 1)))).astype(np.float32), dp)
        flat = x[:, :dim].reshape(-1)                       # (a copy for dim < dp)
        m = min(flat.size, SPECIAL_BITS.size * 3)
        flat[:m] = np.resize(SPECIAL_BITS, m).view(np.float32)
        x[:, :dim] = flat.reshape(n, dim)
        with np.errstate(over="ignore"):
            want16 = x.astype(np.float16).view(np.uint16)
        for fill in fills:
            f16pat = np.array([fill & 0xFFFF, fill >> 16], np.uint16)
            for lo, hi in ((0, n),) + (((130, 290),) if n == 300 else ()):
                lo_eff = lo & ~127
                tn, st, img = _image(probe, x, dp, lo, hi, 1, fill)
                assert (img[lo_eff:hi] == BC.bf16_bits(x[lo_eff:hi])).all(), (n, hex(fill))
                assert (img[lo_eff:hi, dim:] == 0).all()
                rest = np.concatenate([img[:lo_eff].reshape(-1), img[hi:].reshape(-1)])
                assert (rest.reshape(-1, 2) == f16pat).all(), "image written outside [lo, hi)"
                # the tile norms come from the f32 rows: at or above the true norm, within the kernel's rounding up
                for t in range(lo_eff // 128, (hi + 127) // 128):
                    true = np.linalg.norm(x[max(t * 128, lo_eff):min(t * 128 + 128, hi)].astype(np.float64), axis=1).max()
                    got = float(tn[t:t + 1].view(np.float32)[0])
                    assert true <= got <= true * 1.001 + 1e-30, (t, true, got)
                # the f16 format of the same kernel: today's bytes
                _, _, img0 = _image(probe, x, dp, lo, hi, 0, fill)
                assert (img0[lo_eff:hi] == want16[lo_eff:hi]).all()
                rest0 = np.concatenate([img0[:lo_eff].reshape(-1), img0[hi:].reshape(-1)])
                assert (rest0.reshape(-1, 2) == f16pat).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf, float(np.array([0x7F7FFFFF], np.uint32).view(np.float32)[0]), 1.0e6])
def test_image_rows_the_pipe_cannot_carry(probe, bad):
    """a NaN, an infinity, the largest finite f32 (bf16: +inf) or a value beyond 32768 gives its tile the +inf norm in either
    format; the other tiles keep finite norms and every finite element its rounding"""
    dim = dp = 128
    rng = np.random.default_rng(3)
    x = rng.standard_normal((300, dim)).astype(np.float32)
    x[140, 7] = bad
    for fmt in (1, 0):
        tn, st, img = _image(probe, x, dp, 0, 300, fmt, 0xFFFFFFFF)
        assert tn[1] == INF_BITS and tn[0] < INF_BITS and tn[2] < INF_BITS and st[2] == 1
        if fmt == 1:
            want = BC.bf16_bits(x)
            ok = np.ones(x.shape, bool)
            ok[140, 7] = False                               # (a non-finite element: whatever bits)
            assert (img[:300][ok] == want[ok]).all()
            if np.isfinite(bad):
                assert img[140, 7] == want[140, 7]           # (the largest finite f32 comes out as bf16 +inf)


# ---- margin audit ----------------------------------------------------------------------------------------------------------
def _chain(probe, X, Q, k, fmt, mfma16, blocks, early_tiles, fill=0xFFFFFFFF):
    n, dp = X.shape
    nq = Q.shape[0]
    cap = max(n, 64)
    cfg = Cfg(n, dp, nq, k, fmt, mfma16, cap, 1024, blocks, early_tiles, fill)
    n_tiles, nqt = (n + 127) // 128, (nq + 31) // 32
    lay = np.zeros(6, np.uint32)
    out = dict(tile_norm=np.zeros(n_tiles + 2, np.uint32), stats=np.zeros(16, np.uint32), thr=np.zeros(nqt * 32 * 6, np.float32),
               qbound_select=np.zeros(nqt * 32, np.float32), smax=np.zeros(nq * 4096, np.float32), cnt=np.zeros(2 * nq + 2, np.uint32),
               cand=np.zeros(nq * cap * 2, np.uint32))
    io = IO(_ptr(X), _ptr(Q), _ptr(out["tile_norm"]), _ptr(out["stats"]), _ptr(out["thr"]), _ptr(out["qbound_select"]), _ptr(out["smax"]),
            _ptr(out["cnt"]), _ptr(out["cand"]), _ptr(lay))
    rc = probe.bi_probe_chain(C.byref(cfg), C.byref(io))
    assert rc == 0, rc
    out["layout"] = lay
    out["cap"] = cap
    return out


def _audit(X, Q, k, fmt, out, label):
    """the three checks of the audit against float64; returns (largest |approx - exact| / E, survivors per query)"""
    n, dp = X.shape
    nq = Q.shape[0]
    n_s, gap, fine, groups, smax_ld, nqt = (int(v) for v in out["layout"])
    assert fine == 1
    cap = out["cap"]
    exact = X.astype(np.float64) @ Q.astype(np.float64).T            # [n][nq]
    coef = out["thr"][:nqt * 32 * 4].reshape(-1, 4).astype(np.float64)
    assert (coef[:nq, 3] == 0).all() and (coef[:nq, 0] == 0).all()
    assert (out["cnt"][nq:2 * nq] == 0).all() and out["cnt"][2 * nq] == 0, "a query was handed over / the spill pool was used"
    qb_sel = out["qbound_select"][:nq].astype(np.float64)
    qb_fin = out["thr"][nqt * 32 * 4:nqt * 32 * 5][:nq].astype(np.float64)
    R = out["tile_norm"][:(n + 127) // 128].view(np.float32).astype(np.float64)
    assert np.isfinite(R).all()
    kth = np.sort(exact, axis=0)[-k]
    # 2. every group bound lies at or below the best exact score of its group's rows (a fortiori: the k-th largest of them at or
    #    below the k-th best exact score), and so do the selected and the tightened bound
    kR = 16 if fmt == 1 else 8
    smax = out["smax"][:nq * smax_ld].reshape(nq, smax_ld)
    r16 = np.arange(16)
    for t in range(n_s):
        for rt in range(4):
            for g in range(2):
                i = rt * 32 + (r16 & 3) + 8 * (r16 >> 2) + 4 * g
                rows = ((i // kR * n_s + t) * kR + i % kR) * gap
                assert rows.max() < n
                b = smax[:, (t * 4 + rt) * 2 + g].astype(np.float64)
                assert not np.isnan(b).any()
                assert (b <= exact[rows].max(axis=0)).all(), (label, "group bound above its rows' best exact score", t, rt, g)
    assert (qb_sel <= kth).all(), (label, "selected bound above the k-th best exact score", float((qb_sel - kth).max()))
    assert (qb_fin <= kth).all(), (label, "tightened bound above the k-th best exact score", float((qb_fin - kth).max()))
    assert (qb_fin >= qb_sel).all()
    # 1. and 3. per query: the stored survivors' scores within E_q(R_tile) of exact, and a superset of the true top k (every row
    #    at or above the k-th best exact score, ties included)
    use, total = 0.0, 0
    cand_rows = out["cand"][:nq * cap].reshape(nq, cap)
    cand_vals = out["cand"][nq * cap:].view(np.float32).reshape(nq, cap)
    for q in range(nq):
        c = int(out["cnt"][q])
        assert c <= cap
        rows = cand_rows[q, :c].astype(np.int64)
        assert rows.size == np.unique(rows).size and (rows < n).all()
        E = coef[q, 1] * R[rows >> 7] + coef[q, 2]
        err = np.abs(cand_vals[q, :c].astype(np.float64) - exact[rows, q])
        assert (err <= E).all(), (label, "error model violated", q, float((err / E).max()))
        use = max(use, float((err / E).max())) if c else use
        need = np.nonzero(exact[:, q] >= kth[q])[0]
        assert np.isin(need, rows).all(), (label, "a true neighbour did not survive", q)
        total += c
    print("%s: largest |approx - exact| / E = %.3f, survivors per query %.1f of %d rows" % (label, use, total / nq, n))
    return use, total / nq


def _unit(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


AUDIT_CASES = {
    # name: (n rows, dim, queries, k, blocks, early tiles)
    "random-768": (3000, 768, 256, 10, 4, 1),
    "random-192": (1300, 192, 33, 10, 11, 0),
    "random-64-k1": (300, 64, 5, 1, 3, 0),
    "adversarial-up-64": (300, 64, 5, 10, 3, 0),
    "adversarial-down-192": (1300, 192, 33, 10, 2, 1),
    "adversarial-up-768": (640, 768, 33, 10, 5, 0),
    "norm-1e-3": (640, 192, 33, 10, 5, 0),
    "norm-1e3": (640, 192, 33, 10, 5, 0),
    "adversarial-norm-2^10": (640, 64, 33, 10, 5, 0),
    "one-long-row": (1300, 64, 33, 10, 2, 1),
}


@pytest.mark.parametrize("name", list(AUDIT_CASES))
def test_margin_audit(probe, name):
    n, dim, nq, k, blocks, early = AUDIT_CASES[name]
    dp = (dim + 63) // 64 * 64
    rng = np.random.default_rng(len(name) * 131 + n)
    adversarial = name.startswith("adversarial")
    if adversarial:
        X, Q = BC.adversarial(n, nq, dim, dp, -1 if "down" in name else 1, 10 if "2^10" in name else 0, seed=n)
    else:
        X, Q = _pad(_unit(rng, n, dim), dp), _pad(_unit(rng, nq, dim), dp)
        Q[: nq // 2] = X[rng.integers(0, n, nq // 2)] + 0.3 * Q[: nq // 2]      # near neighbours for half the queries
        if name == "norm-1e-3":
            X *= np.float32(1e-3)
        if name == "norm-1e3":
            X *= np.float32(1e3)
        if name == "one-long-row":
            X[700] *= np.float32(100.0)
    for mfma16 in (1, 0):
        out = _chain(probe, X, Q, k, 1, mfma16, blocks, early)
        use, per_q = _audit(X, Q, k, 1, out, "%s bf16 image mfma16=%d" % (name, mfma16))
        if adversarial:
            assert use >= 0.9, "the adversarial input did not reach the bound: the audit would pass on slack"
        if name == "random-768":
            assert per_q < n / 4                              # (the gate does prune)
        if name == "one-long-row":
            R = out["tile_norm"][:(n + 127) // 128].view(np.float32)
            assert R[700 >> 7] > 99 and (np.delete(R, 700 >> 7) < 1.01).all()
    # the f16 image through the same probe and the same checks: its survivors are a superset of the true top k as well
    out0 = _chain(probe, X, Q, k, 0, 1, blocks, early)
    _audit(X, Q, k, 0, out0, "%s f16 image" % name)


# ---- through the C ABI -----------------------------------------------------------------------------------------------------
def _same(a, b):
    (ad, al, an), (bd, bl, bn) = a, b
    assert np.asarray(an).tolist() == np.asarray(bn).tolist()
    assert (al == bl).all()
    assert (ad.view(np.uint32) == bd.view(np.uint32)).all()


def _same_as_oracle(got, o, Q, k, picks, **kw):
    D, L, N = got
    for i in picks:
        od, ol = o.search(Q[i], k, **kw)
        assert int(N[i]) == len(ol), (i, k)
        assert L[i, :len(ol)].tolist() == ol.tolist(), (i, k)
        assert D[i, :len(ol)].view(np.uint32).tolist() == od.view(np.uint32).tolist(), (i, k)


def _rows(rng, n, dim, metric, nc=24):
    centres = rng.standard_normal((nc, dim), dtype=np.float32)
    x = 0.4 * rng.standard_normal((n, dim), dtype=np.float32) + centres[rng.integers(0, nc, n)]
    if metric == "COSINE":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    else:
        x *= np.exp(rng.uniform(np.log(3e-2), np.log(30.0), (n, 1))).astype(np.float32)
    return centres, np.ascontiguousarray(x, dtype=np.float32)


def _queries(rng, centres, nq, metric):
    Q = centres[rng.integers(0, len(centres), nq)] + 0.4 * rng.standard_normal((nq, centres.shape[1]), dtype=np.float32)
    if metric == "COSINE":
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return np.ascontiguousarray(Q, dtype=np.float32)


def _three_ways(ix, search, filtered=True):
    """one batch from the f16 image, from the bf16 image and from the f32 rows; -> (answer, survivors of the three)"""
    res, cands = [], []
    for fmt, image in ((0, 1), (1, 1), (0, 0)):
        ix.set_option("flat-image-format", fmt)
        ix.set_option("flat-f16-image", image)
        res.append(search())
        st = ix.stats()
        if filtered:
            assert st.last_filter_candidates > 0 and st.last_filter_fallback == 0, (fmt, image)
            assert (ix.filter_image_bytes() > 0) == bool(image), (fmt, image)
        cands.append(st.last_filter_candidates)
    ix.set_option("flat-f16-image", 1)
    _same(res[0], res[1])
    _same(res[0], res[2])
    return res[1], cands


@pytest.mark.parametrize("metric,dim,nq,k,n", [("COSINE", 768, 257, 10, 9000), ("IP", 257, 33, 10, 9000), ("COSINE", 100, 5, 1, 9000),
                                               ("IP", 1, 33, 10, 9000), ("IP", 100, 33, 64, 58000), ("COSINE", 100, 33, 10, 3000)])
def test_formats_and_f32_rows_answer_alike(vsa, oracle, metric, dim, nq, k, n):
    rng = np.random.default_rng(dim * 7 + nq)
    centres, x = _rows(rng, n, dim, metric)
    x[500:520] = x[499]                                      # ties across the k-th place go by label
    Q = _queries(rng, centres, nq, metric)
    Q[3] = x[499]
    labels = rng.permutation(2 * n)[:n].astype(np.uint64)
    nb = int(labels.max()) + 1
    allowed = labels[rng.random(n) < 0.3]
    third = oracle.allow_bitmap(allowed, nb)
    ix = vsa.Index("FLAT", dim, metric, initial_cap=n, options=OPTS)
    ix.add_batch(x, labels)
    o = oracle.Flat(dim, metric, max_elements=n)
    o.add_many(x, labels, borrowed=True)
    filtered = n >= 8192
    picks = sorted({0, 3, nq - 1})
    for shape in (1, 0):
        ix.set_option("filter-mfma-shape", shape)
        got, cands = _three_ways(ix, lambda: ix.search_batch(Q, k), filtered)
        _same_as_oracle(got, o, Q, k, picks)
        if dim == 768:
            assert cands[0] == cands[2] and cands[1] != cands[0]     # the f16 image multiplies what the f32 path converts; bf16 does not
        got, _ = _three_ways(ix, lambda: ix.search_batch(Q, k, allow=third, allow_nbits=nb), filtered)
        _same_as_oracle(got, o, Q, k, picks, allow=third, allow_nbits=nb)
    f = ix.make_filter(nb, labels=allowed)
    got, _ = _three_ways(ix, lambda: ix.search_batch_filter_handles(Q, k, [f] * nq), filtered=False)
    _same_as_oracle(got, o, Q, k, picks, allow=third, allow_nbits=nb)
    f.release()


def test_the_bf16_image_follows_writes_growth_and_format_flips(vsa, oracle):
    rng = np.random.default_rng(12)
    n0, n, dim = 9000, 12000, 100
    centres, x = _rows(rng, n, dim, "COSINE")
    Q = _queries(rng, centres, 33, "COSINE")
    ix = vsa.Index("FLAT", dim, "COSINE", initial_cap=n0, options={**OPTS, "flat-image-format": 1})
    ix.add_batch(x[:n0])
    o = oracle.Flat(dim, "COSINE", max_elements=n0)
    o.add_many(x[:n0])
    picks = (0, 7, 21, 32)

    def check():
        got, _ = _three_ways(ix, lambda: ix.search_batch(Q, 10))
        _same_as_oracle(got, o, Q, 10, picks)
        ix.set_option("flat-image-format", 1)
        return got

    check()
    for lab in (5, 129, 4000, n0 - 1):                       # updates in place, one of them three times as long
        row = (3.0 if lab == 5 else 1.0) * x[n - 1 - lab % 1000]
        assert ix.add(lab, row) == vsa.VK_OK
        o.add(row, lab)
    Q[7] = x[n - 1 - 129]
    assert check()[1][7, 0] == 129
    for lab in range(0, 3000, 7):                            # removes: the last row moves into the hole
        assert ix.remove(lab) == vsa.VK_OK
        o.remove(lab)
    check()
    ix.resize(n)                                             # growth past the allocated rows: the image is re-made at the new size
    o.resize(n)
    ix.add_batch(x[n0:], np.arange(n0, n, dtype=np.uint64))
    o.add_many(x[n0:], np.arange(n0, n, dtype=np.uint64))
    check()
    # the format flipped between consecutive batches with nothing written in between: the WHOLE image is rewritten each time (a
    # partial rewrite would leave rows of the other format under the passes: lost neighbours or a flood of survivors)
    base = ix.search_batch(Q, 10)
    c1 = ix.stats().last_filter_candidates
    for fmt in (0, 1, 0, 1):
        ix.set_option("flat-image-format", fmt)
        _same(ix.search_batch(Q, 10), base)
        st = ix.stats()
        assert st.last_filter_fallback == 0 and ix.filter_image_bytes() > 0
        if fmt == 1:
            assert st.last_filter_candidates == c1           # the same image as before the flips, bit for bit
        else:
            c0 = st.last_filter_candidates
    ix.set_option("flat-f16-image", 0)
    _same(ix.search_batch(Q, 10), base)
    assert ix.stats().last_filter_candidates == c0            # the f16 image multiplied what the f32 path converts


def test_four_logical_shards(vsa, oracle):
    rng = np.random.default_rng(4)
    n, dim = 36000, 100
    centres, x = _rows(rng, n, dim, "IP")
    Q = _queries(rng, centres, 33, "IP")
    sh = vsa.Index("FLAT", dim, "IP", initial_cap=n, shard_devices=[0, 0, 0, 0], options=OPTS)
    sh.add_batch(x)
    o = oracle.Flat(dim, "IP", max_elements=n)
    o.add_many(x, borrowed=True)
    res = []
    for fmt, image in ((0, 1), (1, 1), (0, 0)):
        sh.set_option("flat-image-format", fmt)
        sh.set_option("flat-f16-image", image)
        assert sh.get_option("flat-image-format") == fmt
        before = [sh.shard_stats(s).filter_batches for s in range(4)]
        res.append(sh.search_batch(Q, 10))
        assert (sh.filter_image_bytes() > 0) == bool(image)
        assert all(sh.shard_stats(s).filter_batches == before[s] + 1 for s in range(4)), (fmt, image)   # every shard took the filter
    _same(res[0], res[1])
    _same(res[0], res[2])
    _same_as_oracle(res[1], o, Q, 10, (0, 11, 32))


@pytest.mark.parametrize("metric,dtype", [("L2", "f32"), ("IP", "bf16"), ("COSINE", "bf16")])
def test_l2_and_bf16_indexes_ignore_the_option(vsa, metric, dtype):
    rng = np.random.default_rng(31)
    n, dim = 9000, 100
    centres, x = _rows(rng, n, dim, "COSINE")
    ix = vsa.Index("FLAT", dim, metric, initial_cap=n, dtype=dtype, options=OPTS)
    ix.add_batch(x)
    Q = _queries(rng, centres, 33, "COSINE")
    a = ix.search_batch(Q, 10)
    st = ix.stats()
    assert st.last_filter_candidates > 0 and ix.filter_image_bytes() == 0
    ix.set_option("flat-image-format", 1)
    _same(ix.search_batch(Q, 10), a)
    st1 = ix.stats()
    assert ix.filter_image_bytes() == 0 and st1.device_bytes == st.device_bytes and st1.last_filter_candidates == st.last_filter_candidates


def test_the_default_picks_the_format_by_size(vsa):
    """flat-image-format = 2 (the default): bf16 from kImageBf16AutoRows = 1 250 000 rows on, f16 below -- told apart by the survivor
    counts, which are the explicit format's to the last pair; one row removed crosses the line and the image is rewritten"""
    rng = np.random.default_rng(77)
    n, dim = 1_250_000, 64
    centres = rng.standard_normal((50, dim), dtype=np.float32)
    x = np.empty((n, dim), np.float32)
    for i in range(0, n, 250_000):
        x[i:i + 250_000] = 0.5 * rng.standard_normal((250_000, dim), dtype=np.float32) + centres[rng.integers(0, 50, 250_000)]
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    Q = _queries(rng, centres, 33, "COSINE")
    # (one pass over the rows: the survivor set is then a function of the scores alone -- the early pass's harvest reads the
    #  first entries of lists whose order is the order of arrival)
    ix = vsa.Index("FLAT", dim, "COSINE", initial_cap=n, options={"filter-two-pass": 0})
    assert ix.get_option("flat-image-format") == 2
    ix.add_batch(x)

    def run(fmt):
        ix.set_option("flat-image-format", fmt)
        got = ix.search_batch(Q, 10)
        st = ix.stats()
        assert st.last_filter_candidates > 0 and st.last_filter_fallback == 0 and ix.filter_image_bytes() > 0
        return got, st.last_filter_candidates

    auto, c_auto = run(2)
    bf, c_bf = run(1)
    f16, c_f16 = run(0)
    _same(auto, bf)
    _same(auto, f16)
    assert c_auto == c_bf != c_f16
    assert ix.remove(n - 1) == vsa.VK_OK                     # 1 249 999 rows
    below, c_below = run(2)
    _, c_f16b = run(0)
    _, c_bfb = run(1)
    assert c_below == c_f16b != c_bfb
    ix.set_option("flat-f16-image", 0)
    _same(ix.search_batch(Q, 10), below)
