"""The 16x16x32 consumers of the candidate filter's final passes (FlatFilterArgs::mfma16, option filter-mfma-shape; flat_filter_body
<kM16> and filter_gate16 in csrc/flat_filter.hip).  They read the LDS images the 32x32x16 consumers read, in another fragment
order, and map an accumulator register to another (row, query): a wrong row, column, k-piece or subtile is a wrong score or a
pair stored twice or never.  tests/helpers/filter_shape_probe.hip runs qprep and ONE final pass on buffers this file fills, so
every stored pair is held against float64 here:

  * gate open: every (query, row) pair exactly once, its score within E_q(R_t) of the float64 dot product of the rounded operands
    (the coefficients qprep wrote, the tile norm the test supplied) -- for the f32 image, the f32 register path and the bf16 DMA
    kernel, over every query count that fills a sixteenth, a tile, a wave or the launch differently;
  * the edges of the gate: partial tiles, one query, a closed column, a tile beyond f16, an allow bitmap, one block / more blocks
    than tiles, the early + main split;
  * a real bound: survivors a superset of {exact >= bound}, scores within the margin;
  * image and register path: the same survivors, the same score bits;
  * the C ABI with the option at 0 and at 1: labels, counts and distance bits equal the oracle's and each other's.
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32_IMAGE, F32_REG, BF16_DMA = 0, 1, 2
VARIANTS = [F32_IMAGE, F32_REG, BF16_DMA]
VNAME = {F32_IMAGE: "f32_image", F32_REG: "f32_reg", BF16_DMA: "bf16_dma"}
NAN_FILL = 0x7FC07FC0          # a NaN as f32, and as two f16 or two bf16: what lies behind n_rows passes every gate


class Cfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_rows", "stride", "nq", "variant", "mfma16", "blocks", "early_tiles", "cap", "allow_nbits", "fill")]


class IO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rows", "rows16", "queries", "labels", "allow_bits", "tile_norm", "qbound", "cand_cnt", "ovf_q",
                                         "cand_row", "cand_val", "qcoef", "cnt_early")]


@pytest.fixture(scope="module")
def probe():
    path = Path(__file__).resolve().parent / "helpers" / "libfiltershapeprobe.so"
    assert path.exists(), f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
    lib = C.CDLL(str(path))
    lib.filter_shape_probe_run.argtypes = [C.POINTER(Cfg), C.POINTER(IO)]
    lib.filter_shape_probe_run.restype = C.c_int
    return lib


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _pad(a, stride):
    out = np.zeros((a.shape[0], stride), np.float32)
    out[:, :a.shape[1]] = a
    return out


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Case:
    """rows and queries of one probe run, with what the kernel multiplies (the rounded operands) in float64"""

    def __init__(self, variant, x, Q):
        dim = x.shape[1]
        self.variant, self.stride = variant, (dim + 63) // 64 * 64
        self.x = _pad(bf16_round(x) if variant == BF16_DMA else x, self.stride)      # a bf16 index stores the rounded rows
        self.Q = _pad(Q, self.stride)
        self.n, self.nq = x.shape[0], Q.shape[0]
        with np.errstate(invalid="ignore", over="ignore"):
            if variant == BF16_DMA:
                self.dev_rows = np.ascontiguousarray((self.x.view(np.uint32) >> 16).astype(np.uint16))
                self.rows16, qr = None, bf16_round(self.Q)
                xr = self.x
            else:
                self.dev_rows = self.x
                xr = self.x.astype(np.float16)
                self.rows16 = np.ascontiguousarray(xr.view(np.uint16)) if variant == F32_IMAGE else None
                qr = self.Q.astype(np.float16)
            self.approx64 = xr.astype(np.float64) @ qr.astype(np.float64).T      # [row][query]: the rounded operands
            self.exact64 = self.x.astype(np.float64) @ self.Q.astype(np.float64).T
        n_tiles = (self.n + 127) // 128
        norms = np.sqrt((self.x.astype(np.float64) ** 2).sum(1))
        tn = np.zeros(n_tiles, np.float32)
        for t in range(n_tiles):
            tn[t] = np.float32(np.nanmax(norms[t * 128:(t + 1) * 128]) * 1.0002)
        self.tile_norm = tn
        self.labels = np.arange(self.n, dtype=np.uint64) * 3 + 1


def run(probe, case, mfma16, qbound=None, blocks=2, early_tiles=0, allow=None, allow_nbits=0, tile_norm=None, cap=None):
    nq, n = case.nq, case.n
    cap = cap or max(64, (n + 127) // 128 * 128)
    nqt = (nq + 31) // 32
    qb = np.full(nq, -np.inf, np.float32) if qbound is None else np.ascontiguousarray(qbound, np.float32)
    tn = np.ascontiguousarray(case.tile_norm if tile_norm is None else tile_norm, np.float32)
    out = dict(cnt=np.full(nq, 0xDEAD, np.uint32), ovf=np.full(nq, 0xDEAD, np.uint32), row=np.zeros((nq, cap), np.uint32),
               val=np.zeros((nq, cap), np.float32), qcoef=np.zeros((nqt * 32, 4), np.float32), cnt_early=np.zeros(nq, np.uint32))
    cfg = Cfg(n, case.stride, nq, case.variant, mfma16, blocks, early_tiles, cap, allow_nbits, NAN_FILL)
    io = IO(_ptr(case.dev_rows), _ptr(case.rows16), _ptr(case.Q), _ptr(case.labels), _ptr(allow), _ptr(tn), _ptr(qb), _ptr(out["cnt"]),
            _ptr(out["ovf"]), _ptr(out["row"]), _ptr(out["val"]), _ptr(out["qcoef"]), _ptr(out["cnt_early"]))
    rc = probe.filter_shape_probe_run(C.byref(cfg), C.byref(io))
    assert rc == 0, f"filter_shape_probe_run: {rc}"
    out["tile_norm"] = tn
    return out


def survivors(out, q):
    """{row: score} of query q; a row stored twice fails here"""
    c = int(out["cnt"][q])
    assert c <= out["row"].shape[1], (q, c)
    rows = out["row"][q, :c]
    assert len(np.unique(rows)) == c, f"query {q}: a pair stored twice"
    return dict(zip(rows.tolist(), out["val"][q, :c].tolist()))


def margin(out, q, rows):
    """E_q(R_t) = c1 R_t + c0 (inner-product space: c2 = 0) at the rows' tile norms"""
    c2, c1, c0, closed = out["qcoef"][q].astype(np.float64)
    assert c2 == 0 and closed == 0
    return c1 * out["tile_norm"][np.asarray(rows) >> 7].astype(np.float64) + c0


def check_all_pairs(case, out, n_rows=None, ref=None):
    n_rows = case.n if n_rows is None else n_rows
    ref = case.approx64 if ref is None else ref
    for q in range(case.nq):
        assert out["ovf"][q] == 0
        s = survivors(out, q)
        assert sorted(s) == list(range(n_rows)), f"query {q}: {len(s)} pairs stored, {n_rows} rows"
        rows = np.arange(n_rows)
        got = np.array([s[r] for r in range(n_rows)], np.float64)
        err = np.abs(got - ref[:n_rows, q])
        assert (err <= margin(out, q, rows)).all(), (q, float(err.max()))


def _data(seed, n, dim, nq):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dim), dtype=np.float32), rng.standard_normal((nq, dim), dtype=np.float32)


# ---- 1. mapping -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 100, 128, 768])
@pytest.mark.parametrize("variant", VARIANTS, ids=VNAME.get)
def test_every_pair_once_and_within_the_margin(probe, variant, dim):
    x, Q = _data(dim, 256, dim, 256)
    for nq in (1, 17, 33, 64, 65, 256):
        case = Case(variant, x, Q[:nq])
        check_all_pairs(case, run(probe, case, 1))


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=VNAME.get)
def test_partial_tiles_and_block_counts(probe, variant):
    x, Q = _data(7, 1000, 128, 33)
    for n in (1, 127, 129, 1000):
        for nq in ((1, 33) if n == 129 else (33,)):       # (one query: fifteen idle columns of its sixteenth, three waves without queries)
            case = Case(variant, x[:n], Q[:nq])
            tiles = (n + 127) // 128
            for blocks in (1, tiles + 3):
                check_all_pairs(case, run(probe, case, 1, blocks=blocks))


@pytest.mark.parametrize("variant", VARIANTS, ids=VNAME.get)
def test_closed_column_inf_tile_and_allow_bitmap(probe, variant):
    x, Q = _data(11, 384, 128, 40)
    Qn = Q.copy()
    Qn[2, 5] = np.nan                                      # a query that cannot go through f16: closed, handed to the exact pass
    case = Case(variant, x, Qn)
    out = run(probe, case, 1)
    assert out["cnt"][2] == 0 and out["ovf"][2] == 1
    for q in range(case.nq):
        if q != 2:
            assert out["ovf"][q] == 0 and sorted(survivors(out, q)) == list(range(384)), q
    # a tile beyond f16 behind a bound nothing reaches: its rows, all of them, and no others
    case = Case(variant, x, Q)
    tn = case.tile_norm.copy()
    tn[1] = np.inf
    out = run(probe, case, 1, qbound=np.full(case.nq, 1e30, np.float32), tile_norm=tn)
    for q in range(case.nq):
        assert sorted(survivors(out, q)) == list(range(128, 256)), q
    # an allow bitmap over the labels
    rng = np.random.default_rng(5)
    nbits = int(case.labels.max()) + 1
    ok = rng.random(case.n) < 0.5
    bits = np.zeros((nbits + 63) // 64, np.uint64)
    for lab in case.labels[ok].tolist():
        bits[lab >> 6] |= np.uint64(1) << np.uint64(lab & 63)
    out = run(probe, case, 1, allow=bits, allow_nbits=nbits)
    want = np.nonzero(ok)[0].tolist()
    for q in range(case.nq):
        assert sorted(survivors(out, q)) == want, q


@pytest.mark.parametrize("variant", VARIANTS, ids=VNAME.get)
def test_early_and_main_pass_together_store_what_one_pass_stores(probe, variant):
    x, Q = _data(13, 2048, 64, 33)                          # 16 tiles, two blocks of eight
    case = Case(variant, x, Q)
    one = run(probe, case, 1, blocks=2)
    two = run(probe, case, 1, blocks=2, early_tiles=3)
    assert (two["cnt_early"] == 2 * 3 * 128).all()
    for q in range(case.nq):
        assert survivors(one, q) == survivors(two, q), q
    check_all_pairs(case, two)


# ---- 3. the gate against float64, 4. image and register path ----------------------------------------------------------------
@pytest.fixture(scope="module")
def gate_data():
    x, Q = _data(17, 2048, 768, 64)
    x[100:140] = Q[:40] * np.float32(1.5)                    # near neighbours: pairs at and about the bound
    return x, Q


def _kth_bound(case, k=10):
    """the k-th best exact score per query, rounded down to f32"""
    kth = np.sort(case.exact64, axis=0)[-k]
    b = kth.astype(np.float32)
    return np.where(b.astype(np.float64) > kth, np.nextafter(b, np.float32(-np.inf)), b)


@pytest.mark.parametrize("variant", VARIANTS, ids=VNAME.get)
def test_gate_keeps_every_pair_at_or_above_the_bound(probe, gate_data, variant):
    case = Case(variant, *gate_data)
    bound = _kth_bound(case)
    out = run(probe, case, 1, qbound=bound, blocks=5)
    kept = 0
    for q in range(case.nq):
        s = survivors(out, q)
        must = np.nonzero(case.exact64[:, q] >= float(bound[q]))[0].tolist()
        assert len(must) >= 10 and set(must) <= set(s), (q, sorted(set(must) - set(s)))
        rows = np.array(sorted(s))
        err = np.abs(np.array([s[r] for r in rows.tolist()], np.float64) - case.exact64[rows, q])
        assert (err <= margin(out, q, rows)).all(), (q, float(err.max()))
        kept += len(s)
    assert kept < case.nq * case.n // 4                     # (the gate is a gate)


def test_image_and_register_path_store_the_same_pairs_and_score_bits(probe, gate_data):
    img, reg = Case(F32_IMAGE, *gate_data), Case(F32_REG, *gate_data)
    for qbound in (None, _kth_bound(img)):
        a, b = run(probe, img, 1, qbound=qbound, blocks=5), run(probe, reg, 1, qbound=qbound, blocks=5)
        for q in range(img.nq):
            sa, sb = survivors(a, q), survivors(b, q)
            assert sorted(sa) == sorted(sb), q
            assert all(np.float32(sa[r]).view(np.uint32) == np.float32(sb[r]).view(np.uint32) for r in sa), q


# ---- 5. C ABI ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


OPTS = {"filter-prepass-rows": 1024, "filter-min-rows": 8192}


def _clustered(rng, n, dim, metric, nc=40):
    centres = rng.standard_normal((nc, dim), dtype=np.float32)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    x *= np.float32(0.4)
    x += centres[rng.integers(0, nc, n)]
    Q = centres[rng.integers(0, nc, 64)] + 0.4 * rng.standard_normal((64, dim), dtype=np.float32)
    if metric == "COSINE":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return x, np.ascontiguousarray(Q, dtype=np.float32)


# 20 000 rows: one tile per block, so one pass whatever the threshold says, and the filter serves k <= 10; 70 000 x 96 rows are
# two tiles per block (the two-pass pipeline at filter-two-pass-min-tiles 2) and enough for k = 64
@pytest.mark.parametrize("n,dim", [(20_000, 96), (20_000, 768), (70_000, 96)])
@pytest.mark.parametrize("metric,dtype", [("COSINE", "f32"), ("IP", "f32"), ("IP", "bf16")])
def test_c_abi_answers_equal_the_oracle_with_either_shape(vsa, oracle, metric, dtype, n, dim):
    rng = np.random.default_rng(n + dim)
    x, Q = _clustered(rng, n, dim, metric)
    x[500:520] = x[499]                                      # ties across the k-th place: they go by label
    Q[3] = x[499]
    labels = rng.permutation(2 * n)[:n].astype(np.uint64)
    nb = int(labels.max()) + 1
    third = oracle.allow_bitmap(labels[rng.random(n) < 0.3], nb)
    ix = vsa.Index("FLAT", dim, metric, initial_cap=n, options=OPTS, dtype=dtype)
    ix.add_batch(x, labels)
    o = oracle.Flat(dim, metric, max_elements=n)
    o.add_many(bf16_round(x) if dtype == "bf16" else x, labels, borrowed=True)
    filtered = 0
    for k in (1, 10, 64):
        for kw in ({}, {"allow": third, "allow_nbits": nb}):
            for two_pass_min in (2, 16):
                ix.set_option("filter-two-pass-min-tiles", two_pass_min)
                got = []
                for shape in (0, 1):
                    ix.set_option("filter-mfma-shape", shape)
                    got.append(ix.search_batch(Q, k, **kw))
                    st = ix.stats()
                    assert st.last_filter_fallback == 0
                    filtered += 1 if st.last_filter_candidates > 0 else 0
                (d0, l0, n0), (d1, l1, n1) = got
                assert n0.tolist() == n1.tolist() and (l0 == l1).all() and (d0.view(np.uint32) == d1.view(np.uint32)).all(), (k, two_pass_min)
                for i in (0, 3, 40):
                    od, ol = o.search(Q[i], k, **kw)
                    assert int(n1[i]) == len(ol) and l1[i, :len(ol)].tolist() == ol.tolist(), (i, k)
                    assert d1[i, :len(ol)].view(np.uint32).tolist() == od.view(np.uint32).tolist(), (i, k)
    assert filtered >= (24 if n > 20_000 else 16)           # (the candidate filter answered: k <= 10 everywhere, k = 64 from 57 344 rows on)
