"""The models and cases of tests/test_filter_kernels_gpu.py on the CPU (-m "not gpu"): tests/helpers/filter_kernel_cases.py.

  * the models against oracle.allow_bitmap, against Python sets, and against each other (a combine of two built sets is the
    built set of the numpy set operation; a run list is the id list it spells out);
  * the restated launch geometry against the constants in csrc/filter_build.hip, csrc/node_mask.hip and csrc/hnsw_search.hip;
  * every case named for a threshold really crosses it according to that geometry, and no case list is empty.
"""
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"
sys.path.insert(0, str(ROOT / "tests" / "helpers"))
import filter_kernel_cases as FK  # noqa: E402

from oracle import oracle as O  # noqa: E402


def members(words):
    return set(np.flatnonzero(FK.to_bool(words)).tolist())


def test_the_geometry_is_the_sources():
    fb = (CSRC / "filter_build.hip").read_text()
    assert int(re.search(r"constexpr int kThreads = (\d+);", fb).group(1)) == FK.THREADS
    assert "(items + kThreads - 1) / kThreads), 256 * 8)" in fb and FK.GRID_CAP == 256 * 8
    assert "(words + kThreads * 4 - 1) / (kThreads * 4)), 64)" in fb and FK.BATCH_WORDS_PER_BLOCK == FK.THREADS * 4 and FK.BATCH_GX_CAP == 64
    assert "(max_dst_words + kThreads - 1) / kThreads), std::max<uint32_t>(8, 2048 / n))" in fb
    assert fb.count("if (n > 65535) return hipErrorInvalidValue;") == 2 and FK.BATCH_MAX_N == 65535
    assert "return grid_for(n_runs * 64);" in fb
    assert int(re.search(r"constexpr size_t kPartials = (\d+);", (CSRC / "filter_lane.hpp").read_text()).group(1)) == FK.PARTIALS
    assert int(re.search(r"kFilterDeltaLabelBits = (\d+);", (CSRC / "kernels.hpp").read_text()).group(1)) == FK.LABEL_BITS
    nm = (CSRC / "node_mask.hip").read_text()
    assert "kWordsPerWave = 8, kWordsPerBlock = kWordsPerWave * (kThreads / 64);" in nm and "constexpr int kThreads = 256;" in nm
    assert FK.NODE_WORDS_PER_BLOCK == 8 * 256 // 64
    hs = (CSRC / "hnsw_search.hip").read_text()
    assert hs.count("std::min<uint64_t>((total + 255) / 256, 4096);") == 2 and FK.ROWS_GRID_CAP == 4096
    assert FK.grid_for(0) == 1 and FK.grid_for(256) == 1 and FK.grid_for(257) == 2 and FK.grid_for(10 ** 9) == 2048
    assert FK.delta_copy_gx(5000, 300) == 8 and FK.delta_copy_gx(5000, 1) == 20 and FK.combine_batch_gx(65_537) == 64


def test_bit_helpers():
    rng = np.random.default_rng(1)
    w = FK.random_words(rng, 9)
    assert np.array_equal(FK.to_words(FK.to_bool(w), 9), w)
    assert FK.popcounts(w).tolist() == [bin(int(x)).count("1") for x in w] and FK.popcount(w) == len(members(w))
    assert FK.to_bool(np.array([1 | 1 << 63, 2], np.uint64)).nonzero()[0].tolist() == [0, 63, 65]
    assert [FK.tail_mask(n) for n in (0, 1, 63, 64, 65)] == [FK.M64, 1, (1 << 63) - 1, FK.M64, 1]
    assert FK.fill64(0xEEEEEEEE) == 0xEEEEEEEEEEEEEEEE


def test_set_ids_model_is_the_oracles_bitmap():
    rng = np.random.default_rng(2)
    for nbits in (1, 63, 64, 65, 4097):
        ids = rng.integers(0, 3 * nbits, size=500, dtype=np.uint64)
        empty = np.zeros(FK.words_of(nbits) + 2, np.uint64)
        got, added = FK.set_ids_model(empty, nbits, ids)
        inside = ids[ids < nbits]
        assert np.array_equal(got[:FK.words_of(nbits)], O.allow_bitmap(inside, nbits)) and not got[FK.words_of(nbits):].any()
        assert added == len(set(inside.tolist()))
        # extending: only the new bits count, everything else stays -- also the garbage above nbits and behind the bitmap
        dirty = FK.dirty_bitmap(rng, nbits, density=0.5)
        got, added = FK.set_ids_model(dirty, nbits, ids)
        assert members(got) == members(dirty) | set(inside.tolist()) and added == len(set(inside.tolist()) - members(dirty))


def test_set_runs_model_is_the_ids_it_spells_out():
    rng = np.random.default_rng(3)
    for nbits in (0, 1, 64, 65, 1000):
        runs = [(int(a), int(a + l)) for a, l in zip(rng.integers(0, nbits + 20, size=40), rng.integers(0, 130, size=40))]
        runs += [(5, 4), (nbits, nbits + 3), (0, FK.M64), (FK.M64, FK.M64)]
        ids = [i for lo, hi in runs for i in range(lo, min(hi, nbits - 1) + 1) if lo <= hi]
        dirty = FK.dirty_bitmap(rng, nbits, density=0.3)
        got, added = FK.set_runs_model(dirty, nbits, runs)
        want, want_added = FK.set_ids_model(dirty, nbits, np.array(ids, np.uint64))
        assert np.array_equal(got, want) and added == want_added


def test_combine_of_two_built_sets_is_the_built_set_operation():
    rng = np.random.default_rng(4)
    nbits = 1000
    x, y = rng.choice(nbits, size=400, replace=False), rng.choice(nbits, size=300, replace=False)
    empty = np.zeros(FK.words_of(nbits), np.uint64)
    a, b = FK.set_ids_model(empty, nbits, x)[0], FK.set_ids_model(empty, nbits, y)[0]
    for op, fn in ((0, np.intersect1d), (1, np.union1d), (2, np.setdiff1d)):
        got, count = FK.combine_model(a, b, op)
        want = fn(x, y)
        assert np.array_equal(got, O.allow_bitmap(want, nbits)) and count == len(want)
        assert FK.combine_partials(got, 3).sum() == count


def test_delta_model_is_python_sets():
    rng = np.random.default_rng(5)
    for nbits, base_bits in ((1000, 1000), (1000, 448), (1024, 1024), (70, 640), (0, 64)):
        base = FK.random_words(rng, FK.words_of(base_bits))
        clears, sets = rng.integers(0, nbits + 100, size=300, dtype=np.uint64), rng.integers(0, nbits + 100, size=300, dtype=np.uint64)
        copied, final, change = FK.delta_model(base, FK.words_of(nbits), nbits, clears, sets)
        start = {i for i in members(base) if i < nbits}
        assert members(copied) == start
        want = (start - {int(c) for c in clears if c < nbits}) | {int(s) for s in sets if s < nbits}
        assert members(final) == want and change == len(want) - len(start)
    copied, final, change = FK.delta_model(None, 2, 100, [], [3, 3, 99, 100, 127])
    assert members(copied) == set() and members(final) == {3, 99} and change == 2


def test_node_mask_model_is_the_sentence_in_kernels_hpp():
    rng = np.random.default_rng(6)
    count, nbits = 300, 500
    labels = rng.integers(0, 700, size=count).astype(np.uint64)
    labels[7], labels[8] = (1 << 32) + 5, nbits
    live, bitmap = FK.random_words(rng, FK.words_of(count)), FK.random_words(rng, FK.words_of(nbits) + 1)
    got, cnt = FK.node_mask_model(labels, live, count, bitmap, nbits)
    want = {i for i in range(count) if i in members(live) and int(labels[i]) < nbits and int(labels[i]) in members(bitmap)}
    assert members(got) == want and cnt == len(want) and len(got) == FK.words_of(count)
    assert FK.node_mask_model(labels, live, count, bitmap, 0) [1] == 0


def test_partial_sums_follow_a_block_by_block_walk():
    """where the models call the per-block sums decided, a sequential walk in any block order gives them"""
    rng = np.random.default_rng(8)
    nbits, blocks = 5000, 3
    ids = rng.permutation(nbits)[:2000].astype(np.uint64)
    dirty = FK.dirty_bitmap(rng, nbits, density=0.3)
    got = FK.set_ids_partials(dirty, nbits, ids, blocks)
    seen, want = members(dirty), [0] * blocks
    for b in reversed(range(blocks)):
        for i in range(len(ids)):
            if (i // FK.THREADS) % blocks == b and int(ids[i]) not in seen:
                seen.add(int(ids[i]))
                want[b] += 1
    assert got.tolist() == want
    absent = min(set(range(nbits)) - members(dirty))
    assert FK.set_ids_partials(dirty, nbits, np.full(600, absent, np.uint64), blocks) is None          # one new bit named from three blocks
    runs = [(0, 10), (11, 11), (64, 300), (4000, 9000), (9, 3)]
    got = FK.set_runs_partials(dirty, nbits, runs, 2)
    new = [len(set(range(lo, min(hi, nbits - 1) + 1)) - members(dirty)) for lo, hi in runs]
    assert got.tolist() == [new[0] + new[1] + new[2] + new[3], 0]          # runs 0 - 3: block 0's four waves; run 4 is ignored
    assert FK.set_runs_partials(dirty, nbits, [(0, 10), (10, 12)], 1) is None


def test_no_case_list_is_empty_and_every_case_says_why():
    for kind, make in FK.ALL.items():
        cases = make()
        assert len(cases) >= 6, kind
        assert all(c["why"] for c in cases.values()), kind


def test_set_cases_cross_their_thresholds():
    ids = FK.set_ids_cases()
    reach = {len(c["ids"]): (FK.set_ids_blocks(len(c["ids"])), FK.trips(len(c["ids"]), FK.set_ids_blocks(len(c["ids"])))) for c in ids.values()}
    for n, want in ((0, (1, 0)), (1, (1, 1)), (255, (1, 1)), (256, (1, 1)), (257, (2, 1)), (524_288, (2048, 1)), (524_289, (2048, 2)), (600_000, (2048, 2))):
        assert reach[n] == want, n
        assert ids["n_%d" % n]["reach"] == dict(blocks=want[0], trips=want[1])
    assert {c["nbits"] for c in ids.values()} >= {1, 63, 64, 65, 4097, 1_000_003}
    for name, c in ids.items():
        assert len(c["bits"]) == FK.words_of(c["nbits"]) + 1 + FK.PAD
        assert c["bits"][FK.words_of(c["nbits"]):].all(), name              # the slack word and the pad start dirty
        if c.get("exact_partials"):
            assert FK.set_ids_partials(c["bits"], c["nbits"], c["ids"], FK.set_ids_blocks(len(c["ids"]))) is not None, name
    assert len(set(ids["all_equal"]["ids"].tolist())) == 1 and FK.set_ids_blocks(1000) == 4
    assert set((ids["one_word"]["ids"] >> np.uint64(6)).tolist()) == {1}
    for nbits in (4097, 4096):
        e = set(ids["edges_%d" % nbits]["ids"].tolist())
        assert {nbits - 1, nbits, 1 << 40, FK.M64} <= e
        assert FK.set_ids_model(ids["edges_%d" % nbits]["bits"], nbits, ids["edges_%d" % nbits]["ids"])[1] == 2      # nbits - 1 and 0
    ext = ids["extend"]
    assert 0 < FK.set_ids_model(ext["bits"], ext["nbits"], ext["ids"])[1] < len(set(ext["ids"].tolist()))

    runs = FK.set_runs_cases()
    for n, want in ((1, (1, 1)), (4, (1, 1)), (5, (2, 1)), (8192, (2048, 1)), (8193, (2048, 2)), (9000, (2048, 2))):
        c = runs["n_%d" % n]
        assert len(c["runs"]) == n and c["reach"] == dict(blocks=want[0], wave_trips=want[1])
        assert (FK.set_runs_blocks(n), FK.trips(n, FK.set_runs_blocks(n), 4)) == want
        assert FK.set_runs_partials(c["bits"], c["nbits"], c["runs"], want[0]) is not None
    assert runs["long_4096"]["reach"]["lane_trips"] == 2 and runs["long_12288"]["reach"]["lane_trips"] == 4
    lo, hi = (int(v) for v in runs["long_12288"]["runs"][0])
    assert hi - lo + 1 > 64 * 64 * 3 and (hi >> 6) - (lo >> 6) + 1 > 3 * 64
    assert runs["ends_on_last_bit"]["runs"][0][1] == runs["ends_on_last_bit"]["nbits"] - 1 and runs["ends_on_last_bit"]["nbits"] % 64 == 0
    assert FK.set_runs_model(runs["ignored"]["bits"], 4097, runs["ignored"]["runs"])[1] == 1
    assert FK.set_runs_model(runs["nbits_0"]["bits"], 0, runs["nbits_0"]["runs"])[1] == 0
    got = members(FK.set_runs_model(np.zeros(68, np.uint64), 4097, runs["clamped"]["runs"])[0])
    assert max(got) == 4096 and got == set(range(100, 4097))
    over = runs["overlapping_9000"]
    assert FK.set_runs_partials(over["bits"], over["nbits"], over["runs"], 2048) is None and over["reach"]["wave_trips"] == 2
    assert {tuple(r) for r in runs["single_bits"]["runs"].tolist()} == {(0, 0), (63, 63), (64, 64)}


def test_popcount_and_combine_cases_cross_their_thresholds():
    pop = FK.popcount_cases()
    assert {c["bits"].size: c["reach"]["trips"] for c in pop.values()} == {0: 0, 1: 1, 255: 1, 256: 1, 257: 1, 524_289: 2}
    assert all(c["start"] > 1 << 32 for c in pop.values())
    com = FK.combine_cases()
    for words, want in ((0, (1, 0)), (1, (1, 1)), (64, (1, 1)), (257, (2, 1)), (524_289, (2048, 2))):
        for op in (0, 1, 2):
            c = com["op%d_words_%d" % (op, words)]
            assert c["a"].size == words and c["op"] == op and c["reach"] == dict(blocks=want[0], trips=want[1])
            assert (FK.combine_blocks(words), FK.trips(words, FK.combine_blocks(words))) == want
    for op in (0, 1, 2):      # a written zero among the partial sums
        c = com["op%d_words_257" % op]
        assert FK.combine_partials(FK.combine_model(c["a"], c["b"], op)[0], 2)[0] == 0
    bat = FK.combine_batch_cases()
    assert {(len(c["table"]), c["words"]) for c in bat.values()} >= {(n, w) for n in (1, 3, 97) for w in (0, 1, 1024, 1025)} | {(3, 65_537), (65_536, 1)}
    # (a block is sized for 1024 words, four trips of its 256 threads; behind the cap of 64 blocks a fifth begins)
    assert [bat["n3_words_%d" % w]["reach"] for w in (1, 1024, 1025, 65_537)] == [dict(gx=1, trips=1), dict(gx=1, trips=4), dict(gx=2, trips=3), dict(gx=64, trips=5)]
    assert FK.combine_batch_gx(65_536) == 64 and FK.trips(65_536, 64) == 4
    for name, c in bat.items():
        t = c["table"]
        assert t[0, 0] == t[0, 1] and (len(t) == 1 or (t[1, :2] == t[0, :2]).all()) and c["starts"].all(), name
        assert bool(c.get("refused")) == (len(t) > FK.BATCH_MAX_N), name
        if len(t) >= 3:
            assert set(t[:, 2].tolist()) == {0, 1, 2}


def test_delta_cases_cross_their_thresholds():
    d = FK.delta_cases()
    assert {k for k, c in d.items() if c["copy_only"]} == {"copy_no_base", "copy_same_words_stray", "copy_grow", "copy_nbits_0", "copy_nbits_mod64_0", "copy_batch_300"}
    base, nb = d["copy_same_words_stray"]["items"][0]
    assert len(base) == FK.words_of(nb) and nb % 64 and int(base[-1]) >> (nb % 64) == FK.M64 >> (nb % 64)
    base, nb = d["copy_grow"]["items"][0]
    assert len(base) < FK.words_of(nb)
    assert d["copy_nbits_0"]["items"][0][1] == 0 and d["copy_nbits_mod64_0"]["items"][0][1] % 64 == 0 and d["copy_no_base"]["items"][0][0] is None
    b = d["copy_batch_300"]
    sizes = [FK.words_of(nb) for _, nb in b["items"]]
    assert len(sizes) == 300 and min(sizes) == 0 and max(sizes) == 5000 == b["max_dst_words"] and b["reach"]["gx"] == 8 and b["reach"]["copy_trips"] == 3
    assert sum(s < 256 for s in sizes) >= 1 and sum(256 * 8 < s for s in sizes) >= 100       # idle blocks; second and third trips
    assert any(base is None for base, _ in b["items"]) and any(base is not None and len(base) < FK.words_of(nb) for base, nb in b["items"])

    def item_of(recs):
        return (recs >> np.uint64(FK.LABEL_BITS)).astype(np.int64)

    def label_of(recs):
        return (recs & np.uint64((1 << FK.LABEL_BITS) - 1)).astype(np.int64)

    def waves(recs):
        return [set(item_of(recs[i:i + 64]).tolist()) for i in range(0, len(recs), 64)]

    assert all(len(w) == 1 for w in waves(d["one_item"]["clr"]))
    both = set(label_of(d["one_item"]["clr"]).tolist()) & set(label_of(d["one_item"]["set"]).tolist())
    assert len(both) > 100
    many = d["many_items"]
    assert min(len(w) for w in waves(many["clr"])[:-1]) >= 64 // 3 and min(len(w) for w in waves(many["set"])[:-1]) >= 64 // 3
    assert label_of(many["clr"]).max() >= 256 > label_of(many["clr"]).min()
    for name, top in (("past_nbits_near", None), ("past_nbits_far", (1 << 40) - 1)):
        c = d[name]
        nbs = np.array([nb for _, nb in c["items"]])
        for recs in (c["clr"], c["set"]):
            lab, nb = label_of(recs), nbs[item_of(recs)]
            assert (lab >= nb).any() and (lab < nb).any()
            if top is None:     # all within the item's last word and its slack word
                assert (lab < (nb + 63) // 64 * 64 + 64).all() and set((lab - nb)[lab >= nb].tolist()) >= {0, 1}
            else:
                assert lab.max() == top and ((lab >= nb) & (lab % (1 << 32) < nb)).any()
    t = d["duplicates_tail"]
    assert len(t["clr"]) == len(t["set"]) == 64 * 3 + 5 and len(set(t["clr"].tolist())) < 10
    assert len(waves(t["clr"])[0]) == 1 and any(len(w) == 2 for w in waves(t["clr"]))
    big = d["records_600000"]
    assert len(big["set"]) > 524_288 and big["reach"]["apply_trips"] == 2 and (np.diff(item_of(big["set"])) >= 0).all()
    sp = d["item_65534"]
    assert len(sp["items"]) == 65_535 and set(item_of(sp["clr"]).tolist()) == {0, 40_000, 65_534} == set(item_of(sp["set"]).tolist())
    for c in d.values():
        assert c["starts"].all() and len(c["starts"]) == len(c["items"])
        assert all(base is None or isinstance(base, np.ndarray) for base, _ in c["items"])
    # clears of unset bits and sets of set bits happen: fewer changes than distinct labels
    base, nb = d["one_item"]["items"][0]
    _, final, change = FK.delta_model(base, FK.words_of(nb), nb, label_of(d["one_item"]["clr"]), label_of(d["one_item"]["set"]))
    assert abs(change) < len(set(label_of(d["one_item"]["set"]).tolist()))


def test_node_mask_and_row_cases_cross_their_thresholds():
    nm = FK.node_mask_cases()
    assert {c["count"] for c in nm.values()} >= {1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 5003}
    assert {len(c["filters"]) for c in nm.values()} >= {1, 63, 64, 65, 130}
    assert [nm["count_%d" % c]["reach"]["blocks"] for c in (2047, 2048, 2049)] == [1, 1, 2]
    assert [nm["filters_%d" % n]["reach"]["groups"] for n in (63, 64, 65, 130)] == [1, 1, 2, 3]
    for name, c in nm.items():
        lab = c["labels"]
        assert len(c["live"]) == FK.words_of(c["count"]) and len(lab) == c["count"]
        for b, nb in c["filters"]:
            assert len(b) == FK.words_of(nb) + 1
        if c["count"] >= 63:
            assert (lab >= (1 << 39)).any() and len(set(lab.tolist())) < c["count"] and (np.diff(lab.astype(np.int64)) < 0).any(), name
            nbs = [nb for _, nb in c["filters"]]
            if len(nbs) >= 3:
                small = int(lab[lab < FK.UNIVERSE].max())
                assert 0 in nbs and any(0 < nb < small for nb in nbs) and any(nb > small for nb in nbs), name
    c = nm["filters_130"]
    counts = [FK.node_mask_model(c["labels"], c["live"], c["count"], b, nb)[1] for b, nb in c["filters"]]
    assert sum(x > 0 for x in counts[64:]) >= 40 and len(set(counts[64:])) >= 30       # the later groups' counts are there to be wrong
    assert not nm["live_zero"]["live"].any() and (nm["live_ones"]["live"] == np.uint64(FK.M64)).all() and nm["live_ones"]["count"] % 64
    # a label equal to a filter's nbits, admitted by the random word above the bitmap in at least one case
    hits = 0
    for c in nm.values():
        on = FK.to_bool(c["live"])
        for b, nb in c["filters"]:
            at = np.flatnonzero(c["labels"] == np.uint64(nb))
            hits += sum(1 for i in at if nb and on[i] and (int(b[nb >> 6]) >> (nb & 63)) & 1)
    assert hits >= 3
    rows = FK.rows_cases()
    assert {c["src"].shape for c in rows.values()} >= {(n, s) for n in (1, 257) for s in (1, 17, 33)}
    big = rows["n31800_stride33"]
    assert big["src"].size > 4096 * 256 and big["reach"] == dict(blocks=4096, trips=2)
    for c in rows.values():
        assert len(set(c["idx"].tolist())) == len(c["idx"]) and c["idx"].max() < c["rows"] > len(c["idx"])
