"""The CPU side of tests/test_flat_scan_kernels_gpu.py: for every case that file runs on the device, the ownership model of
tests/helpers/flat_scan_cases.py puts every row of the window into exactly one list per query, the model's lists merged by
select_model are the oracle's top-k, and the path a case is meant for is really reached by its input."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import flat_scan_cases as SC  # noqa: E402
import flat_select_cases as FS  # noqa: E402


def oracle_topk(oracle, data, labels, allowed, q, k, bits=None, nbits=0):
    """the oracle's answer: without a filter its own search; with one, its full ranking restricted to the allowed rows
    (tests/test_flat_sweep_gpu.py: the reference's bruteforce can under-fill behind a filter)"""
    o = oracle.Flat(data.dim, data.space, max_elements=data.n)
    o.add_many(data.X, labels[:data.n])
    if bits is None:
        od, ol = o.search(data.Q[q, :data.dim], k)
        return od.view(np.uint32), ol
    od, ol = o.search(data.Q[q, :data.dim], data.n)
    ok_labels = set(labels[:data.n][allowed].tolist())
    keep = np.array([int(l) in ok_labels for l in ol.tolist()], bool)
    return od[keep][:k].view(np.uint32), ol[keep][:k]


def test_key_is_monotone():
    v = np.array([-np.inf, -3.0, -1e-40, 0.0, 1e-40, 2.0, np.inf], np.float32)
    key = SC.f32_key(v).tolist()
    assert key == sorted(key) and len(set(key)) == v.size and key[-1] == SC.INF_KEY


def test_gemm_ownership_and_merge(oracle):
    cases = SC.gemm_cases()
    shapes = sorted({(c.n, c.nrp, c.contig) for c in cases})
    for n, nrp, contig in shapes:
        owner, count = SC.gemm_owner(n, nrp, contig)
        assert (count == 1).all() and (owner >= 0).all() and owner.max() < nrp * 8, (n, nrp, contig)
        # the closed form of the same statement
        r = np.arange(n)
        t = r // 128
        tiles = SC.gemm_tiles(n, nrp, contig)
        rp_of_tile = np.zeros(-(-n // 128), np.int64)
        for rp, ts in enumerate(tiles):
            rp_of_tile[ts] = rp
        assert (owner == rp_of_tile[t] * 8 + ((r % 128) // 32) * 2 + (r % 8) // 4).all()
        first, _ = SC.gemm_owner(n, nrp, contig, first_tile_only=True)
        assert ((first >= 0).sum() == sum(min(128, n - 128 * ts[0]) for ts in tiles if ts))
    seen = set()
    for c in cases:
        key = (c.stride, c.bf16, c.n, c.nq, c.k, c.nrp, c.contig, c.filt, c.labels)
        if key in seen or c.stride > 192 or c.nq > 6:
            continue
        seen.add(key)
        data = SC.dataset(oracle, "IP", c.stride, c.bf16, c.n, c.nq, SC.GEMM_DUPS)
        labels = SC.make_labels(c.labels, c.n, c.n, 0)
        bits, nbits, allowed = SC.make_filter(labels, c.n, c.filt, 0) if c.filt is not None else (None, 0, np.ones(c.n, bool))
        owner, _ = SC.gemm_owner(c.n, c.nrp, c.contig)
        for q in (0, c.nq - 1):
            wd, wl, _rows = SC.lists_want(data.table[q], labels, allowed, owner, c.nrp * 8, c.k)
            md, ml = SC.merged(wd, wl, c.k)
            od, ol = oracle_topk(oracle, data, labels, allowed, q, c.k, bits, nbits)
            assert md.tolist() == od.tolist() and ml.tolist() == ol.tolist(), (c, q)
    assert len(seen) >= 20


def test_gemm_paths_are_reached(oracle):
    cases = SC.gemm_cases()
    assert {c.stride: c.tile_q for c in cases} == SC.TILE_Q
    per_block = {(c.n, c.nrp, c.contig): [len(t) for t in SC.gemm_tiles(c.n, c.nrp, c.contig)] for c in cases}
    main1, main0 = per_block[(SC.N_MAIN, 8, 1)], per_block[(SC.N_MAIN, 8, 0)]
    assert sorted(set(main1)) == [3, 4] and main1 == [4, 4, 3, 3, 3, 3, 3, 3]                # t_rem = 2: the remainder split
    assert sorted(set(main0)) == [3, 4] and SC.N_MAIN % 128 != 0                            # the strided walk wraps twice or more
    assert 0 in per_block[(300, 8, 1)] and 0 in per_block[(300, 8, 0)]                      # more partitions than tiles
    assert per_block[(128 * 8, 8, 1)] == [1] * 8 and per_block[(128 * 8 + 1, 8, 1)] == [2] + [1] * 7
    assert per_block[(128 * 5 - 10, 16, 1)].count(0) == 11
    # a lockstep window smaller than the walk, equal to it, larger; two and three query tiles
    assert {(c.lockstep, (c.nq + c.tile_q - 1) // c.tile_q) for c in cases if c.group == "lockstep"} == {(w, t) for w in (0, 1, 2, 64) for t in (2, 3)}
    assert {c.nq - c.tile_q for c in cases if c.group == "strides"} >= {0, 3}
    # ties: the copies of the duplicated vector are the nearest rows of query 0; more of them than k lie in ONE list (k <= 10),
    # 128 j apart and inside one tile, and neighbours 163 / 164 lie in different lists
    data = SC.dataset(oracle, "IP", 64, 0, SC.N_MAIN, 5, SC.GEMM_DUPS)
    labels = SC.make_labels("spread", SC.N_MAIN, SC.N_MAIN, 0)
    rank = SC.ranking(data.table[0], labels, np.ones(SC.N_MAIN, bool))
    nd = data.dups.size
    assert sorted(rank[:nd].tolist()) == sorted(data.dups.tolist()) and len(set(data.table_bits[0, data.dups].tolist())) == 1
    assert data.table_bits[0, rank[nd]] != data.table_bits[0, rank[0]]
    for contig in (0, 1):
        owner, _ = SC.gemm_owner(SC.N_MAIN, 8, contig)
        most = np.bincount(owner[data.dups]).max()
        assert most >= 11 and owner[163] != owner[164]
        if contig:
            assert owner[163] == owner[163 + 128] == owner[163 + 256]
        for k in (1, 5, 10):                                   # the k-th and the (k + 1)-th of that list are copies: labels decide
            wd, wl, rows = SC.lists_want(data.table[0], labels, np.ones(SC.N_MAIN, bool), owner, 64, k + 1)
            l = int(np.argmax(np.bincount(owner[data.dups])))
            assert set(rows[l].tolist()) <= set(data.dups.tolist())
    # the bounds: "true" leaves rows AT the bound (the tie must survive), "first1024" is looser for some query
    true = SC.gemm_bound("true", data, labels, np.ones(SC.N_MAIN, bool), 10, 5)
    first = SC.gemm_bound("first1024", data, labels, np.ones(SC.N_MAIN, bool), 10, 5)
    assert (data.table[0] == true[:5].view(np.float32)[0]).sum() > 1
    assert (first[5:] >= true[5:]).all() and (first[5:] > true[5:]).any() and (true[5:] == SC.f32_key(true[:5].view(np.float32))).all()
    mixed = SC.gemm_bound("mixed", data, labels, np.ones(SC.N_MAIN, bool), 10, 5)
    assert mixed[5 + 1] == SC.INF_KEY and mixed[5] == true[5]
    # the 2 % filter: fewer than k rows allowed in most lists (k = 5) and in the whole index (k = 256); labels beyond nbits exist
    lab = SC.make_labels("small", SC.N_MAIN, SC.N_MAIN, 0)
    bits, nbits, allowed = SC.make_filter(lab, SC.N_MAIN, 0.02, 0)
    owner, _ = SC.gemm_owner(SC.N_MAIN, 8, 1)
    per_list = np.bincount(owner[allowed], minlength=64)
    assert (per_list < 5).sum() > 32 and 0 < allowed.sum() < 256 and (lab >= np.uint64(nbits)).sum() == 8
    assert SC.gemm_bound("true", data, lab, allowed, 256, 5)[5] == SC.INF_KEY


def test_scan_ownership_and_merge(oracle):
    cases = SC.scan_cases()
    for key in sorted({(c.row_begin, c.row_len, c.nrp, c.e) for c in cases}):
        rb, ln, nrp, e = key
        owner, count = SC.scan_owner(SC.N_SCAN, rb, rb + ln, nrp, e)
        inside = (np.arange(SC.N_SCAN) >= rb) & (np.arange(SC.N_SCAN) < rb + ln)
        assert (count[inside] == 1).all() and (count[~inside] == 0).all() and (owner[~inside] == -1).all(), key
        g = ((np.arange(SC.N_SCAN) - rb) // 16) % (4 * nrp)
        assert (owner[inside] == (g if e > 1 else g // 4)[inside]).all()
    seen = set()
    for c in cases:
        key = (c.l2, c.bf16, c.stride, c.e, c.k, c.nrp, c.row_begin, c.row_len, c.filt, c.lb)
        if key in seen or c.group in ("redo", "control") or c.stride > 192:
            continue
        seen.add(key)
        data = SC.dataset(oracle, "L2" if c.l2 else "IP", c.stride, c.bf16, SC.N_SCAN, SC.SCAN_NQ, SC.SCAN_DUPS)
        labels = SC.make_labels("small", SC.N_SCAN, SC.N_SCAN, 1)
        bits, nbits, allowed = SC.make_filter(labels, SC.N_SCAN, c.filt, 1) if c.filt is not None else (None, 0, np.ones(SC.N_SCAN, bool))
        owner, n_lists, elig, lb_d, lb_l = SC.scan_setup(c, data, labels, allowed)
        q = 0
        wd, wl, _rows = SC.lists_want(data.table[q], labels, elig[q], owner, n_lists, c.k)
        md, ml = SC.merged(wd, wl, c.k)
        # the oracle over the rows of the window alone (their table slots, so labels and distances are the same rows')
        win = np.arange(c.row_begin, c.row_begin + c.row_len)
        o = oracle.Flat(data.dim, data.space, max_elements=win.size)
        o.add_many(data.X[win], labels[win])
        od, ol = o.search(data.Q[q, :data.dim], win.size)
        ok = set(labels[:SC.N_SCAN][allowed].tolist())
        keep = np.array([int(l) in ok for l in ol.tolist()], bool)
        od, ol = od[keep], ol[keep]
        if c.lb is not None:                                  # entries j + 1 .. j + k of the ranking, exactly
            assert od[c.lb] == lb_d[q] and ol[c.lb] == lb_l[q]
            assert od[c.lb - 1] == od[c.lb] == od[c.lb + 1], "the lower bound is not inside a run of tied distances"
            od, ol = od[c.lb + 1:], ol[c.lb + 1:]
        assert md.tolist() == od[:c.k].view(np.uint32).tolist() and ml.tolist() == ol[:c.k].tolist(), c
    assert len(seen) >= 40


def test_scan_paths_are_reached(oracle):
    cases = SC.scan_cases()
    assert {(c.qb, c.e, c.k) for c in cases if c.group == "variants"} == set(SC.VARIANTS)
    assert {(c.l2, c.bf16) for c in cases if c.group == "variants" and c.e == 16} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(c.nq < c.qb for c in cases) and any(c.nq > c.qb and c.nq % c.qb for c in cases)
    # chunk counts against the unrolled step (8 pieces in flight, 4 for the block of 8 queries): below it, a step and a
    # remainder, several steps
    assert {c.stride // 16 for c in cases if c.group == "strides"} == {4, 12, 36}
    # waves and whole blocks that own nothing
    for c in cases:
        if c.group == "windows" and c.row_len <= 17:
            owner, _ = SC.scan_owner(SC.N_SCAN, c.row_begin, c.row_begin + c.row_len, c.nrp, 4)
            assert np.unique(owner[owner >= 0]).size <= 2 < 4 * c.nrp
    assert {c.row_len for c in cases if c.group == "windows"} >= {1, 15, 16, 17, 511, 513, 1023, 1025, 3000}
    assert {c.row_begin for c in cases} == {0, 37} and {c.redo for c in cases if c.group == "redo"} == {0, 1, 3, 8}
    assert sorted(set(SC.Q_INDEX)) == [0, 1, 2, 3, 5, 6, 7] and len(SC.Q_INDEX) == 8
    assert [SC.flag_runs((v,) + SC.REDO_FLAG) for v in (0, 1, 3, 8)] == [False, True, True, True]
    assert [SC.flag_runs(f) for f in ((5, 4, 0), (0, 1, 8), (9, 1, 8), (5, 5, 0), (3, 1, 8))] == [False, False, False, True, True]
    # ties at the k-th place inside one wave's rows (e > 1: k = 1 .. 11 of the 12 copies in wave 4's first tile) and across the
    # four waves of a block (e == 1: 22 copies in block 1, k = 10)
    data = SC.dataset(oracle, "L2", 64, 0, SC.N_SCAN, SC.SCAN_NQ, SC.SCAN_DUPS)
    labels = SC.make_labels("small", SC.N_SCAN, SC.N_SCAN, 1)
    every = np.ones(SC.N_SCAN, bool)
    rank = SC.ranking(data.table[0], labels, every)
    nd = data.dups.size
    assert nd == 24 and sorted(rank[:nd].tolist()) == sorted(data.dups.tolist()) and len(set(data.table_bits[0, data.dups].tolist())) == 1
    waves, _ = SC.scan_owner(SC.N_SCAN, 0, 3000, 8, 4)
    blocks, _ = SC.scan_owner(SC.N_SCAN, 0, 3000, 8, 1)
    in_win = data.dups[data.dups < 3000]
    assert np.bincount(waves[in_win])[4] == 13 and np.bincount(blocks[in_win])[1] == 22
    assert len(set(waves[in_win[blocks[in_win] == 1]].tolist())) == 4
    shifted, _ = SC.scan_owner(SC.N_SCAN, 37, 3037, 8, 4)
    assert len(set(shifted[data.dups[:12]].tolist())) == 2      # a window that starts off the table's tiles splits the run
    # the filter: labels at and beyond nbits exist, and a bit of the filter is really consulted for most rows
    bits, nbits, allowed = SC.make_filter(labels, SC.N_SCAN, 0.5, 1)
    assert (labels >= np.uint64(nbits)).sum() == 8 and 0.4 < allowed.mean() < 0.6
