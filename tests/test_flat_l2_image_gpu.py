"""Option flat-l2-image through the C ABI: a batch an f32 L2 index answers from the f16 image of its rows has the ids, distance
bits and survivor count of the same batch with the option off -- and the CPU oracle's answer.  vk_index_filter_image_bytes()
says which path a batch took.  The filter serves a batch from 8 x 1024 rows per ten of k on (FlatIndex::search): 9 000 rows
up to k = 10, 82 000 at k = 100; below that the exact kernels answer whatever the option says, and no image is read."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (the overrides of tests/test_flat_f16_image_gpu.py, with the row floor taken out of the way of the 9 000-row index)
OPTS = {"filter-prepass-rows": 1024, "filter-min-rows": 0, "filter-two-pass-min-tiles": 2}


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


def _filtered(n, k):
    return n >= 8 * 1024 * ((k + 9) // 10)


def _same(a, b):
    (ad, al, an), (bd, bl, bn) = a, b
    assert an.tolist() == bn.tolist()
    assert (al == bl).all()
    assert (ad.view(np.uint32) == bd.view(np.uint32)).all()


def _same_as_oracle(got, o, Q, k, picks):
    D, L, N = got
    for i in picks:
        od, ol = o.search(Q[i], k)
        assert int(N[i]) == len(ol), (i, k)
        assert L[i, :len(ol)].tolist() == ol.tolist(), (i, k)
        assert D[i, :len(ol)].view(np.uint32).tolist() == od.view(np.uint32).tolist(), (i, k)


def _rows(rng, n, dim, nc=40):
    """clustered, un-normalised rows: norms over a decade, near neighbours within the filter's margin of each other"""
    centres = rng.standard_normal((nc, dim), dtype=np.float32)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    x *= np.float32(0.4)
    x += centres[rng.integers(0, nc, n)]
    x *= np.exp(rng.uniform(np.log(0.3), np.log(3.0), (n, 1))).astype(np.float32)
    return centres, x


def _queries(rng, centres, nq):
    Q = centres[rng.integers(0, len(centres), nq)] + 0.4 * rng.standard_normal((nq, centres.shape[1]), dtype=np.float32)
    return np.ascontiguousarray(Q, dtype=np.float32)


def _image_bytes(ix, dim):
    """-> allocated rows x padded dim x 2 (the rows from device_bytes with the image released), that device_bytes; option on"""
    dp = (dim + 63) // 64 * 64
    ix.set_option("flat-l2-image", 0)
    ix.search_batch(np.zeros((8, dim), np.float32), 1)       # (the next row-statistics step releases the image)
    off = ix.stats().device_bytes
    ix.set_option("flat-l2-image", 1)
    assert off % (dp * 4 + 8) == 0                           # option 0: the row table alone
    return off // (dp * 4 + 8) * dp * 2, off


def _on_off(ix, Q, k, want_bytes, same_count=True):
    """one batch from the image, the same batch from the f32 rows.  same_count: one pass gates every row against the sample's
    bound, so the survivors are the same set; behind an early pass the bound comes from the first 512 survivors in arrival
    order and the count differs from run to run on one path (tests/test_flat_l2_image_kernels_gpu.py compares those sets)"""
    ix.set_option("flat-l2-image", 1)
    a = ix.search_batch(Q, k)
    sa, ba = ix.stats(), ix.filter_image_bytes()
    ix.set_option("flat-l2-image", 0)
    b = ix.search_batch(Q, k)
    sb, bb = ix.stats(), ix.filter_image_bytes()
    ix.set_option("flat-l2-image", 1)
    assert ba == want_bytes and bb == 0, (ba, bb, want_bytes)
    assert sa.last_filter_candidates > 0 and sa.last_filter_fallback == 0
    assert sb.last_filter_candidates > 0 and sb.last_filter_fallback == 0
    assert not same_count or sa.last_filter_candidates == sb.last_filter_candidates          # the same survivors
    _same(a, b)
    return a


@pytest.mark.parametrize("n,dim", [(9_000, 64), (9_000, 100), (9_000, 384), (70_000, 64), (70_000, 100), (70_000, 384), (82_000, 100)])
def test_image_and_f32_rows_give_the_same_answer_as_the_oracle(vsa, oracle, n, dim):
    """1, 2 (padded: 100 -> 128) and 6 stages of 64 (six: the ring of five row stages wraps); 5, 33 and 256 queries; 9 000 rows are
    one pass, 70 000 an early and a main pass"""
    rng = np.random.default_rng(n + dim)
    centres, x = _rows(rng, n, dim)
    x[500:520] = x[499]                                      # ties across the k-th place: they go by label
    Qall = _queries(rng, centres, 256)
    Qall[3] = x[499]
    ix = vsa.Index("FLAT", dim, "L2", initial_cap=n, options=OPTS)
    assert ix.get_option("flat-l2-image") == 0               # ships off
    ix.add_batch(x)
    ix.search_batch(Qall[:33], 1)
    assert ix.filter_image_bytes() == 0                      # default options: no image, whatever flat-f16-image says
    o = oracle.Flat(dim, "L2", max_elements=n)
    o.add_many(x, borrowed=True)
    want, _ = _image_bytes(ix, dim)
    for nq in (5, 33, 256):
        Q = Qall[:nq]
        for k in (1, 10, 100):
            if _filtered(n, k):
                ix.set_option("filter-two-pass-min-tiles", 16)                # one pass over every row: the same survivors
                got = _on_off(ix, Q, k, want)
                if n >= 2 * 256 * 128:                                        # two tiles for each of 256 blocks: early + main pass
                    ix.set_option("filter-two-pass-min-tiles", 2)
                    _same(_on_off(ix, Q, k, want, same_count=False), got)
                    assert ix.stats().last_filter_final_rows < n
            else:                                            # the exact kernels serve it: the option changes nothing
                got = ix.search_batch(Q, k)
                assert ix.filter_image_bytes() == 0
            _same_as_oracle(got, o, Q, k, (0, 3, nq - 1))


def test_the_image_follows_writer_phases(vsa, oracle):
    """rows overwritten, removed, added past a growth of the table, the option 1 -> 0 -> 1: every batch from the image equals the
    batch from the f32 rows and the oracle that saw the same writes; option 0 brings device_bytes back to the row table"""
    rng = np.random.default_rng(8)
    n0, n, dim = 40_000, 50_000, 100
    centres, x = _rows(rng, n, dim)
    Q = _queries(rng, centres, 64)
    ix = vsa.Index("FLAT", dim, "L2", initial_cap=n0, options=OPTS)
    ix.add_batch(x[:n0])
    o = oracle.Flat(dim, "L2", max_elements=n0)
    o.add_many(x[:n0])
    picks = (0, 7, 21, 63)

    def check():
        want, off = _image_bytes(ix, dim)                    # (released and re-made whole)
        _same_as_oracle(_on_off(ix, Q, 10, want), o, Q, 10, picks)
        ix.search_batch(Q, 10)
        assert ix.filter_image_bytes() == want and ix.stats().device_bytes > off
        return want

    w0 = check()
    ix.set_option("flat-image-format", 1)                    # the L2 image is f16 whatever the format option says
    _same_as_oracle(_on_off(ix, Q, 10, w0), o, Q, 10, picks)
    ix.set_option("flat-image-format", 2)
    # overwrite rows in place (one of them three times as long: its half norm and its tile's norm bound grow with it)
    for lab in (5, 129, 20_000, n0 - 1):
        row = (3.0 if lab == 5 else 1.0) * x[n - 1 - lab % 1000]
        assert ix.add(lab, row) == vsa.VK_OK
        o.add(row, lab)
    Q[7] = x[n - 1 - 129]                                    # the new content of row 129 must be found
    got = _on_off(ix, Q, 10, w0)
    assert got[1][7, 0] == 129
    _same_as_oracle(got, o, Q, 10, picks)
    # remove (the last row moves into the hole), with the option off while it happens
    ix.set_option("flat-l2-image", 0)
    for lab in range(0, 3000, 7):
        assert ix.remove(lab) == vsa.VK_OK
        o.remove(lab)
    ix.search_batch(Q, 10)
    assert ix.filter_image_bytes() == 0
    check()
    # add past a growth of the row table: the image is re-made at the new size
    ix.resize(n)
    o.resize(n)
    ix.add_batch(x[n0:], np.arange(n0, n, dtype=np.uint64))
    o.add_many(x[n0:], np.arange(n0, n, dtype=np.uint64))
    assert check() > w0


def test_tiles_the_f16_pipe_cannot_carry(vsa, oracle):
    """an element beyond 32768, a half norm beyond f16 and a NaN row: three tiles whose gate is open; the image holds what the
    producers' conversion makes of them, and the exact re-rank settles those pairs from the f32 rows"""
    rng = np.random.default_rng(6)
    n, dim = 50_000, 64
    x = rng.standard_normal((n, dim), dtype=np.float32)
    x[123, 5] = 1.0e6                                        # does not fit f16
    x[20_000] = 50.0                                         # |x|^2 / 2 = 80 000: beyond the 60 000 the half norm may reach
    x[40_001, 3] = np.float32(np.nan)
    bad_tiles = 3
    assert bad_tiles * 64 <= n // 128                        # (FlatIndex::search: few enough that the index stays on the filter)
    ix = vsa.Index("FLAT", dim, "L2", initial_cap=n, options=OPTS)
    ix.add_batch(x)
    o = oracle.Flat(dim, "L2", max_elements=n)
    o.add_many(x)
    Q = rng.standard_normal((64, dim), dtype=np.float32)
    want, _ = _image_bytes(ix, dim)
    got = _on_off(ix, Q, 10, want)
    assert ix.stats().last_filter_candidates >= 64 * bad_tiles * 128                # every pair of the three (full) tiles, per query
    _same_as_oracle(got, o, Q, 10, range(0, 64, 5))
