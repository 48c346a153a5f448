"""B operands by LDS DMA on the DMA row path (option filter-bdma = 2; flat_filter_body<..., kDma, kBDma> in csrc/flat_filter.hip).

With the option at 2 the passes that stream 16-bit rows by DMA -- a bf16 index, the bf16 or the f16 image of an f32 index, inner-product
space -- also take their query fragments L2 -> LDS by DMA, into a ring of three B stages beside a ring of three row stages (value 1:
five row stages, two B stages written from registers).  The consumers read the same bytes from the same layout, so everything
a batch reports must be equal BIT FOR BIT between the two values: a slot that wraps a stage early or late, a piece that had not
landed when the barrier published it, or a query tile clamped wrongly is another score, i.e. another survivor count or answer.

Shapes: 9 000 rows are 70 tiles and a 40-row remainder (blocks own unequal tile counts; the smallest index the filter serves);
D = 64 .. 320 and 768 are 1, 2, 3, 4, 5 and 12 stages per tile -- below, at and above the length of either ring, so slots wrap inside
a tile and across tiles; 5, 63, 64, 65 and 256 queries exercise the clamp of the query tiles and waves without queries.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTS = {"filter-prepass-rows": 1024, "filter-min-rows": 0, "filter-two-pass-min-tiles": 2}
KINDS = {"bf16": dict(dtype="bf16", metric="IP", opts={}),
         "f32_bf16_image": dict(dtype="f32", metric="COSINE", opts={"flat-image-format": 1}),
         "f32_f16_image": dict(dtype="f32", metric="COSINE", opts={"flat-image-format": 0})}
BATCHES = (5, 63, 64, 65, 256)


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    return _pkg.vsa


def bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def _rows(rng, n, dim, metric, nc=24):
    centres = rng.standard_normal((nc, dim), dtype=np.float32)
    x = 0.4 * rng.standard_normal((n, dim), dtype=np.float32) + centres[rng.integers(0, nc, n)]
    if metric == "COSINE":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    return centres, np.ascontiguousarray(x, dtype=np.float32)


def _queries(rng, centres, nq, metric):
    Q = centres[rng.integers(0, len(centres), nq)] + 0.4 * rng.standard_normal((nq, centres.shape[1]), dtype=np.float32)
    if metric == "COSINE":
        Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return np.ascontiguousarray(Q, dtype=np.float32)


def _same(a, b, what):
    (ad, al, an), (bd, bl, bn) = a, b
    assert np.asarray(an).tolist() == np.asarray(bn).tolist(), what
    assert (al == bl).all(), what
    assert (ad.view(np.uint32) == bd.view(np.uint32)).all(), what


def _same_as_oracle(got, o, Q, k, picks, **kw):
    D, L, N = got
    for i in picks:
        od, ol = o.search(Q[i], k, **kw)
        assert int(N[i]) == len(ol), (i, k)
        assert L[i, :len(ol)].tolist() == ol.tolist(), (i, k)
        assert D[i, :len(ol)].view(np.uint32).tolist() == od.view(np.uint32).tolist(), (i, k)


def _both(ix, search, what):
    """one batch with filter-bdma 1 and with 2 -> the answer, after the two were found equal in every reported bit"""
    out = []
    for v in (1, 2):
        ix.set_option("filter-bdma", v)
        got = search()
        st = ix.stats()
        assert st.last_filter_candidates > 0 and st.last_filter_fallback == 0, (what, v)
        out.append((got, st.last_filter_candidates))
    _same(out[0][0], out[1][0], what)
    # (the survivors, not the re-ranked rows: the re-rank prunes by a bound taken from the first survivors of a list, and the order of a
    #  list is the order in which blocks finished)
    assert out[0][1] == out[1][1], (what, "survivors", out[0][1], out[1][1])
    return out[1][0]


def _index(vsa, oracle, kind, n, dim, seed, borrowed=True):
    kd = KINDS[kind]
    rng = np.random.default_rng(seed)
    centres, x = _rows(rng, n, dim, kd["metric"])
    x[500:520] = x[499]                                      # ties across the k-th place go by label
    Q = _queries(rng, centres, 256, kd["metric"])
    Q[3] = x[499]
    labels = rng.permutation(2 * n)[:n].astype(np.uint64)
    ix = vsa.Index("FLAT", dim, kd["metric"], initial_cap=n, dtype=kd["dtype"], options={**OPTS, **kd["opts"]})
    ix.add_batch(x, labels)
    o = oracle.Flat(dim, kd["metric"], max_elements=n)
    o.add_many(bf16_round(x) if kd["dtype"] == "bf16" else x, labels, borrowed=borrowed)
    return ix, o, x, Q, labels, rng


@pytest.mark.parametrize("dim", [64, 128, 192, 256, 320, 768])
@pytest.mark.parametrize("kind", list(KINDS))
def test_values_1_and_2_answer_bit_for_bit_alike(vsa, oracle, kind, dim):
    n, k = 9000, 10
    ix, o, x, Q, labels, rng = _index(vsa, oracle, kind, n, dim, dim * 3 + len(kind))
    for shape in (1, 0):
        ix.set_option("filter-mfma-shape", shape)
        for min_tiles in (2, 16):                            # two passes (early + main), one pass
            ix.set_option("filter-two-pass-min-tiles", min_tiles)
            for nq in BATCHES:
                got = _both(ix, lambda: ix.search_batch(Q[:nq], k), (kind, dim, shape, min_tiles, nq))
                if shape == 1 or nq == 65:
                    _same_as_oracle(got, o, Q, k, sorted({0, 3, nq - 1}))
    # an allow bitmap: the gate's rare path looks rows up by label
    nb = int(labels.max()) + 1
    third = oracle.allow_bitmap(labels[rng.random(n) < 0.3], nb)
    ix.set_option("filter-mfma-shape", 1)
    ix.set_option("filter-two-pass-min-tiles", 2)
    got = _both(ix, lambda: ix.search_batch(Q[:65], k, allow=third, allow_nbits=nb), (kind, dim, "allow"))
    _same_as_oracle(got, o, Q, k, (0, 3, 64), allow=third, allow_nbits=nb)


@pytest.mark.parametrize("kind", list(KINDS))
def test_k_64_over_58_000_rows(vsa, oracle, kind):
    ix, o, x, Q, labels, rng = _index(vsa, oracle, kind, 58000, 128, 58)
    for shape in (1, 0):
        ix.set_option("filter-mfma-shape", shape)
        for nq in (65, 256):
            got = _both(ix, lambda: ix.search_batch(Q[:nq], 64), (kind, shape, nq))
            _same_as_oracle(got, o, Q, 64, (0, 3, nq - 1))


def test_the_option_flips_between_batches_and_across_a_write_phase(vsa, oracle):
    n, dim = 9000, 192
    ix, o, x, Q, labels, rng = _index(vsa, oracle, "f32_bf16_image", n, dim, 7, borrowed=False)   # (the oracle is written to)
    Q = Q[:65]
    base = ix.search_batch(Q, 10)
    _same_as_oracle(base, o, Q, 10, (0, 3, 64))
    for v in (2, 1, 2):
        ix.set_option("filter-bdma", v)
        assert ix.get_option("filter-bdma") == v
        _same(ix.search_batch(Q, 10), base, v)
    # a write phase under value 2: rows updated in place and removed; the image and the answers follow with either value
    for lab in labels[[5, 129, 4000, n - 1]].tolist():
        row = x[(lab * 7 + 1) % n] * np.float32(1.0)
        assert ix.add(lab, row) == vsa.VK_OK
        o.add(row, lab)
    for lab in labels[0:3000:7].tolist():
        if lab in labels[[5, 129, 4000, n - 1]].tolist():
            continue
        assert ix.remove(lab) == vsa.VK_OK
        o.remove(lab)
    after = _both(ix, lambda: ix.search_batch(Q, 10), "after writes")
    _same_as_oracle(after, o, Q, 10, (0, 3, 7, 64))
    ix.set_option("filter-bdma", 1)
    _same(ix.search_batch(Q, 10), after, "back at 1")
    ix.set_option("filter-bdma", 0)                          # B through registers everywhere: the same answer
    _same(ix.search_batch(Q, 10), after, "at 0")


def test_option_range(vsa):
    ix = vsa.Index("FLAT", 64, "IP", initial_cap=256)
    for v in (0, 1, 2):
        ix.set_option("filter-bdma", v)
        assert ix.get_option("filter-bdma") == v
    with pytest.raises(vsa.VkError) as e:
        ix.set_option("filter-bdma", 3)
    assert e.value.code == vsa.VK_ERR_INVALID
    assert ix.get_option("filter-bdma") == 2                 # (a refused value changes nothing)


def test_l2_keeps_the_register_sets(vsa, oracle):
    """L2 is out of the new kernels' reach (the half norms ride with a B register set): value 2 launches what value 1 launches"""
    rng = np.random.default_rng(3)
    n, dim = 9000, 192
    centres, x = _rows(rng, n, dim, "L2")
    Q = _queries(rng, centres, 65, "L2")
    ix = vsa.Index("FLAT", dim, "L2", initial_cap=n, options=OPTS)
    ix.add_batch(x)
    o = oracle.Flat(dim, "L2", max_elements=n)
    o.add_many(x, borrowed=True)
    got = _both(ix, lambda: ix.search_batch(Q, 10), "l2")
    _same_as_oracle(got, o, Q, 10, (0, 3, 64))
