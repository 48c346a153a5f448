"""The resident f16 image of an f32 index's rows (option flat-f16-image; FlatIndex::ensure_image, row_stats_kernel, the DMA
row path of flat_filter_body).  The image holds, element for element, what the filter's row producers make of the f32 rows on
their way into LDS, so a batch answered from it has the same ids, the same distance bits and the same counts as the same
batch answered from the f32 rows on the same index (the option is read per batch) -- and as the CPU oracle.
vk_index_filter_image_bytes() says which of the two a batch read, so no comparison here can pass with both runs on one
path."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = {"filter-prepass-rows": 1024, "filter-min-rows": 32768, "filter-two-pass-min-tiles": 2}
N_BIG, N_SMALL = 230_000, 40_000          # k = 256 takes the filter from 8 x 26 624 rows on; 40 000 rows are 1.2 tiles per block: one pass


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


def _same(a, b):
    (ad, al, an), (bd, bl, bn) = a, b
    assert an.tolist() == bn.tolist()
    assert (al == bl).all()
    assert (ad.view(np.uint32) == bd.view(np.uint32)).all()


def _same_as_oracle(got, o, Q, k, picks, **kw):
    D, L, N = got
    for i in picks:
        od, ol = o.search(Q[i], k, **kw)
        assert int(N[i]) == len(ol), (i, k)
        assert L[i, :len(ol)].tolist() == ol.tolist(), (i, k)
        assert D[i, :len(ol)].view(np.uint32).tolist() == od.view(np.uint32).tolist(), (i, k)


def _rows(rng, n, dim, metric, nc=40):
    """clustered rows (near neighbours within the filter's margin of each other); COSINE: unit norm, IP: norms over three decades"""
    centres = rng.standard_normal((nc, dim), dtype=np.float32)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    x *= np.float32(0.4)
    x += centres[rng.integers(0, nc, n)]
    if metric == "COSINE":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    else:
        x *= np.exp(rng.uniform(np.log(3e-2), np.log(30.0), (n, 1))).astype(np.float32)
    return centres, x


def _queries(rng, centres, nq, metric):
    Q = centres[rng.integers(0, len(centres), nq)] + 0.4 * rng.standard_normal((nq, centres.shape[1]), dtype=np.float32)
    if metric == "COSINE":
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return np.ascontiguousarray(Q, dtype=np.float32)


def _stats(ix):
    """vk_index_stats, with what vk_index_filter_image_bytes says about the same batch next to it"""
    st = ix.stats()
    st.filter_image_bytes = ix.filter_image_bytes()
    return st


def _image_bytes(ix, dim):
    """what filter_image_bytes must say when the image was read: allocated rows x padded dim x 2 (the allocated rows from
    device_bytes with the image released: rows x (row bytes + 8))"""
    dp = (dim + 63) // 64 * 64
    old = ix.get_option("flat-f16-image")
    ix.set_option("flat-f16-image", 0)
    ix.search_batch(np.zeros((8, dim), np.float32), 1)       # (the next row-statistics step releases the image)
    off = _stats(ix).device_bytes
    ix.set_option("flat-f16-image", old)
    assert off % (dp * 4 + 8) == 0
    return off // (dp * 4 + 8) * dp * 2, off


def _on_off(ix, Q, k, want_bytes, **kw):
    """one batch from the image, the same batch from the f32 rows; the statistics tell the two apart"""
    ix.set_option("flat-f16-image", 1)
    a = ix.search_batch(Q, k, **kw)
    sa = _stats(ix)
    assert sa.filter_image_bytes == want_bytes if want_bytes is not None else sa.filter_image_bytes > 0, (sa.filter_image_bytes, want_bytes)
    assert sa.last_filter_candidates > 0 and sa.last_filter_fallback == 0
    ix.set_option("flat-f16-image", 0)
    b = ix.search_batch(Q, k, **kw)
    sb = _stats(ix)
    assert sb.filter_image_bytes == 0
    assert sb.last_filter_candidates > 0 and sb.last_filter_fallback == 0
    ix.set_option("flat-f16-image", 1)
    _same(a, b)
    return a, sa, sb


@pytest.mark.parametrize("dim", [64, 100, 768])             # padded (100 -> 128) and not; 1, 2 and 12 pipeline stages
@pytest.mark.parametrize("metric", ["COSINE", "IP"])
def test_image_and_f32_rows_give_the_same_answer_as_the_oracle(vsa, oracle, metric, dim):
    rng = np.random.default_rng(1000 + dim)
    centres, x = _rows(rng, N_BIG, dim, metric)
    x[5000:5200] = x[4999]                                   # ties across the k-th place: they go by label
    Q = _queries(rng, centres, 64, metric)
    Q[3] = x[4999]
    labels = rng.permutation(2 * N_BIG)[:N_BIG].astype(np.uint64)
    nb = int(labels.max()) + 1
    third = oracle.allow_bitmap(labels[rng.random(N_BIG) < 0.3], nb)
    big = vsa.Index("FLAT", dim, metric, initial_cap=N_BIG, options=OPTS)
    big.add_batch(x, labels)
    o = oracle.Flat(dim, metric, max_elements=N_BIG)
    o.add_many(x, labels, borrowed=True)
    want, off = _image_bytes(big, dim)
    dp = (dim + 63) // 64 * 64
    for k in (1, 10, 256):
        for kw in ({}, {"allow": third, "allow_nbits": nb}):
            # enough rows for the two-pass pipeline (seven tiles per block) ...
            big.set_option("filter-two-pass-min-tiles", 2)
            got, st, _ = _on_off(big, Q, k, want, **kw)
            assert 0 < st.last_filter_final_rows < N_BIG
            _same_as_oracle(got, o, Q, k, (0, 3, 40), **kw)
            # ... and the one-pass pipeline over the same rows (few enough under the default threshold): same arithmetic and
            # the same bound on both sides, hence the same survivors too
            big.set_option("filter-two-pass-min-tiles", 16)
            got1, s1, s0 = _on_off(big, Q, k, want, **kw)
            assert s1.last_filter_final_rows == N_BIG
            assert s1.last_filter_candidates == s0.last_filter_candidates, (k, sorted(kw))
            _same(got1, got)
    # the image is counted in device_bytes (rows + slack, rounded to the allocation granule), and is gone with the option off
    big.search_batch(Q, 10)
    assert _stats(big).device_bytes - off == ((want // (dp * 2) + 256) * dp * 2 + 4095) // 4096 * 4096
    del big
    # few enough rows that one pass runs at the tests' threshold as well
    small = vsa.Index("FLAT", dim, metric, initial_cap=N_SMALL, options=OPTS)
    small.add_batch(x[:N_SMALL], labels[:N_SMALL])
    os_ = oracle.Flat(dim, metric, max_elements=N_SMALL)
    os_.add_many(x[:N_SMALL], labels[:N_SMALL], borrowed=True)
    want_s, _ = _image_bytes(small, dim)
    for k in (1, 10):
        for kw in ({}, {"allow": third, "allow_nbits": nb}):
            got, s1, s0 = _on_off(small, Q, k, want_s, **kw)
            assert s1.last_filter_final_rows == N_SMALL and s1.last_filter_candidates == s0.last_filter_candidates
            _same_as_oracle(got, os_, Q, k, (1, 3, 50), **kw)


@pytest.mark.parametrize("metric,dtype", [("L2", "f32"), ("IP", "bf16"), ("COSINE", "bf16")])
def test_l2_and_bf16_indexes_keep_no_image(vsa, metric, dtype):
    """L2 indexes keep their kernel (the DMA row path has no half-norm K-step), bf16 rows already are the 16-bit stream"""
    rng = np.random.default_rng(31)
    n, dim = 70_000, 100
    centres, x = _rows(rng, n, dim, "COSINE")
    ix = vsa.Index("FLAT", dim, metric, initial_cap=n, dtype=dtype, options=OPTS)
    ix.add_batch(x)
    Q = _queries(rng, centres, 64, "COSINE")
    a = ix.search_batch(Q, 10)
    st = _stats(ix)
    assert st.last_filter_candidates > 0 and st.filter_image_bytes == 0
    assert st.device_bytes % (128 * (2 if dtype == "bf16" else 4) + 8) == 0          # the row table alone
    ix.set_option("flat-f16-image", 0)
    _same(ix.search_batch(Q, 10), a)
    assert _stats(ix).device_bytes == st.device_bytes


def test_the_image_follows_writer_phases(vsa, oracle):
    """rows overwritten, removed, added past a growth of the table, re-added -- with the option turned off and on again in
    between (off releases the image, on builds it anew): every batch from the image equals the batch from the f32 rows and
    the oracle that saw the same writes"""
    rng = np.random.default_rng(8)
    n0, n, dim = 40_000, 50_000, 100
    centres, x = _rows(rng, n, dim, "COSINE")
    Q = _queries(rng, centres, 64, "COSINE")
    ix = vsa.Index("FLAT", dim, "COSINE", initial_cap=n0, options=OPTS)
    ix.add_batch(x[:n0])
    o = oracle.Flat(dim, "COSINE", max_elements=n0)
    o.add_many(x[:n0])
    picks = (0, 7, 21, 63)

    def check():
        """image released and re-made whole, then a batch from either side; leaves the image in place and current"""
        want, _ = _image_bytes(ix, dim)
        got, _, _ = _on_off(ix, Q, 10, want)
        _same_as_oracle(got, o, Q, 10, picks)
        ix.search_batch(Q, 10)
        assert _stats(ix).filter_image_bytes == want
        return want

    w0 = check()
    # overwrite rows in place (one of them three times as long: the tile's norm bound grows with it); the image is there and
    # current, so only the written rows are converted
    for lab in (5, 129, 20_000, n0 - 1):
        row = (3.0 if lab == 5 else 1.0) * x[n - 1 - lab % 1000]
        assert ix.add(lab, row) == vsa.VK_OK
        o.add(row, lab)
    Q[7] = x[n - 1 - 129]                                    # the new content of row 129 must be found ...
    got, _, _ = _on_off(ix, Q, 10, w0)
    assert got[1][7, 0] == 129
    _same_as_oracle(got, o, Q, 10, picks)
    # remove (the last row moves into the hole), with the option off while it happens
    ix.set_option("flat-f16-image", 0)
    for lab in range(0, 3000, 7):
        assert ix.remove(lab) == vsa.VK_OK
        o.remove(lab)
    ix.search_batch(Q, 10)
    assert _stats(ix).filter_image_bytes == 0
    ix.set_option("flat-f16-image", 1)
    check()
    # add past a growth of the row table: the image is re-made at the new size
    ix.resize(n)
    o.resize(n)
    ix.add_batch(x[n0:], np.arange(n0, n, dtype=np.uint64))
    o.add_many(x[n0:], np.arange(n0, n, dtype=np.uint64))
    w1 = check()
    assert w1 > w0
    # re-add what was removed (new slots at the end), off and on again without a search in between
    ix.set_option("flat-f16-image", 0)
    ix.set_option("flat-f16-image", 1)
    for lab in range(0, 3000, 7):
        assert ix.add(lab, x[lab]) == vsa.VK_OK
        o.add(x[lab], lab)
    Q[21] = x[7 * 11]
    got, st, _ = _on_off(ix, Q, 10, None)                    # (the image was there all along: only the written rows are converted)
    assert st.filter_image_bytes == _image_bytes(ix, dim)[0] >= w1
    assert got[1][21, 0] == 77
    _same_as_oracle(got, o, Q, 10, picks)


def test_tiles_the_f16_pipe_cannot_carry(vsa, oracle):
    """1e6, inf and NaN in the rows: the image holds inf / NaN there as the producers' conversion does, the tile's gate is open
    either way and the exact re-rank settles it from the f32 rows"""
    rng = np.random.default_rng(6)
    n, dim = 50_000, 64
    x = rng.standard_normal((n, dim), dtype=np.float32)
    x[123, 5] = 1.0e6                                        # does not fit f16
    x[40_000, 9] = np.float32(np.inf)
    x[40_001, 3] = np.float32(np.nan)
    ix = vsa.Index("FLAT", dim, "IP", initial_cap=n, options=OPTS)
    ix.add_batch(x)
    o = oracle.Flat(dim, "IP", max_elements=n)
    o.add_many(x)
    Q = rng.standard_normal((64, dim), dtype=np.float32)
    want, _ = _image_bytes(ix, dim)
    got, st, _ = _on_off(ix, Q, 10, want)
    assert st.last_filter_candidates >= 64 * 2 * 128         # two whole tiles per query
    _same_as_oracle(got, o, Q, 10, range(0, 64, 5))


def _occupy(torch, leave_bytes):
    """take the device's free memory down to about leave_bytes (blocks of 1 GiB, then 64 MiB, then 4 MiB)"""
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    held = []
    for block in (1 << 30, 64 << 20, 4 << 20):
        while torch.cuda.mem_get_info()[0] > leave_bytes + block:
            try:
                held.append(torch.empty(block, dtype=torch.uint8, device="cuda"))
            except torch.OutOfMemoryError:
                break
    return held


def test_the_image_refused_under_memory_pressure(vsa, oracle):
    """no room for the image: the batch is answered from the f32 rows (never an error), the refusal is remembered until the
    next writer phase, and after memory is back and a write the image is"""
    import torch
    rng = np.random.default_rng(41)
    n, dim = 70_000, 768                                     # rows 215 MB, image 108 MB
    centres, x = _rows(rng, n, dim, "COSINE")
    Q = _queries(rng, centres, 64, "COSINE")
    ix = vsa.Index("FLAT", dim, "COSINE", initial_cap=n, options={**OPTS, "flat-f16-image": 0})
    ix.add_batch(x)
    base = ix.search_batch(Q, 10)                            # (the batch's scratch exists before the squeeze)
    st = _stats(ix)
    assert st.filter_image_bytes == 0 and st.last_filter_candidates > 0
    off = st.device_bytes
    o = oracle.Flat(dim, "COSINE", max_elements=n)
    o.add_many(x, borrowed=True)
    _same_as_oracle(base, o, Q, 10, (0, 9, 33))
    held = _occupy(torch, 48 << 20)
    try:
        ix.set_option("flat-f16-image", 1)
        for _ in range(2):
            _same(ix.search_batch(Q, 10), base)
            st = _stats(ix)
            assert st.filter_image_bytes == 0 and st.last_filter_candidates > 0 and st.device_bytes == off
    finally:
        del held
        torch.cuda.empty_cache()
    _same(ix.search_batch(Q, 10), base)                      # memory is back, but nothing was written: no new attempt
    assert _stats(ix).filter_image_bytes == 0
    assert ix.add(17, x[17]) == vsa.VK_OK                    # a writer phase (the same row again)
    _same(ix.search_batch(Q, 10), base)
    st = _stats(ix)
    assert st.filter_image_bytes == off // (dim * 4 + 8) * dim * 2 and st.device_bytes > off
