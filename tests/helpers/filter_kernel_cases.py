"""What tests/test_filter_kernels_gpu.py (the device filter kernels through tests/helpers/filter_build_probe.hip, node_mask_probe.hip
and hnsw_search_probe.hip's row entry) and tests/test_filter_kernels_model_cpu.py (which pins the models and the cases' reach
without a GPU) share:

  * the launch geometry of csrc/filter_build.hip, csrc/node_mask.hip and the two row kernels of csrc/hnsw_search.hip, restated,
    so that a case can say which threshold it crosses (a second trip of a grid-stride loop, a capped grid, ...);
  * boolean models of each launcher's contract as kernels.hpp words it: a set of ids, a union of inclusive clamped runs, the
    three set operations, copy-grow-mask then clears then sets, live && label < nbits && bit(label) -- each with the counts;
  * the case lists.  A case is a dict; "why" says what it is there for, "reach" holds the geometry facts the CPU test re-derives.

Bitmaps are numpy uint64 words, bit i of a set = word i // 64, bit i % 64.  Every comparison is exact.
"""
import numpy as np

M64 = (1 << 64) - 1
THREADS = 256
GRID_CAP = 2048             # grid_for: 256 * 8 blocks
PARTIALS = 2048             # filter_lane.hpp kPartials
LABEL_BITS = 40             # kFilterDeltaLabelBits
BATCH_WORDS_PER_BLOCK = 1024
BATCH_GX_CAP = 64
BATCH_MAX_N = 65535
NODE_WORDS_PER_BLOCK = 32   # node_mask.hip: 8 words per wave, 4 waves
ROWS_GRID_CAP = 4096        # launch_scatter_u32 / launch_gather_u32
FILLS = (0x00000000, 0xFFFFFFFF, 0xEEEEEEEE)


def fill64(fill):
    return (fill << 32) | fill


# ---- geometry -------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def grid_for(items):
    return min(max(1, ceil_div(items, THREADS)), GRID_CAP)


def set_ids_blocks(n):
    return grid_for(n)


def set_runs_blocks(n_runs):
    return grid_for(n_runs * 64)


def combine_blocks(words):
    return grid_for(words)


def combine_batch_gx(words):
    return min(max(1, ceil_div(words, BATCH_WORDS_PER_BLOCK)), BATCH_GX_CAP)


def delta_copy_gx(max_dst_words, n):
    return min(max(1, ceil_div(max_dst_words, THREADS)), max(8, GRID_CAP // n))


def trips(items, blocks, per_block=THREADS):
    """the most trips one thread (or one wave, per_block = waves per block) makes through its grid-stride loop"""
    return ceil_div(items, blocks * per_block)


def node_mask_blocks(count):
    return ceil_div(ceil_div(count, 64), NODE_WORDS_PER_BLOCK)


def rows_blocks(total):
    return min(ceil_div(total, THREADS), ROWS_GRID_CAP)


# ---- bit helpers ----------------------------------------------------------------------------------------------------------
def words_of(nbits):
    return (nbits + 63) // 64


def popcounts(words):
    """set bits of each word"""
    w = np.ascontiguousarray(words, np.uint64)
    return np.unpackbits(w.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1).astype(np.int64) if w.size else np.zeros(0, np.int64)


def popcount(words):
    return int(popcounts(words).sum())


def to_bool(words, nbits=None):
    b = np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8), bitorder="little").astype(bool)
    return b if nbits is None else b[:nbits]


def to_words(flags, n_words):
    """bools, bit i = flags[i], as n_words uint64 words (what lies behind the flags is zero)"""
    b = np.zeros(n_words * 64, np.uint8)
    b[:len(flags)] = flags
    return np.packbits(b, bitorder="little").view(np.uint64).copy()


def tail_mask(nbits):
    return M64 if nbits % 64 == 0 else (1 << (nbits % 64)) - 1


# ---- models ---------------------------------------------------------------------------------------------------------------
def set_ids_model(bits_in, nbits, ids):
    """(the words after the launch, bits newly set): ids >= nbits are ignored, everything else of bits_in stays"""
    flags = to_bool(bits_in)
    ids = np.asarray(ids, np.uint64)
    keep = ids[ids < np.uint64(nbits)].astype(np.int64) if nbits else np.zeros(0, np.int64)
    before = int(flags.sum())
    flags[keep] = True
    return to_words(flags, len(bits_in)), int(flags.sum()) - before


def set_runs_model(bits_in, nbits, runs):
    """the union of the runs [lo, hi] with lo <= hi and lo < nbits, hi clamped to nbits - 1, added to bits_in"""
    flags = to_bool(bits_in)
    before = int(flags.sum())
    edge = np.zeros(nbits + 1, np.int64)
    for lo, hi in runs:
        lo, hi = int(lo), int(hi)
        if lo > hi or lo >= nbits:
            continue
        edge[lo] += 1
        edge[min(hi, nbits - 1) + 1] -= 1
    flags[:nbits] |= np.cumsum(edge[:nbits]) > 0
    return to_words(flags, len(bits_in)), int(flags.sum()) - before


def combine_model(a, b, op):
    """(a OP b, its set bits): 0 = and, 1 = or, 2 = and-not"""
    x, y = to_bool(a), to_bool(b)
    r = (x & y) if op == 0 else (x | y) if op == 1 else (x & ~y)
    return to_words(r, len(a)), int(r.sum())


def delta_model(base, dst_words, nbits, clears, sets):
    """(dst after the copy, dst after the clears and then the sets, population change of the two apply steps)"""
    flags = np.zeros(dst_words * 64, bool)
    if base is not None:
        m = min(len(base), dst_words)
        flags[:m * 64] = to_bool(base[:m])
    flags[nbits:] = False                      # the last word masked to nbits (dst_words = words_of(nbits))
    copied = flags.copy()
    for labels, value in ((clears, False), (sets, True)):
        labels = np.asarray(labels, np.uint64)
        flags[labels[labels < np.uint64(nbits)].astype(np.int64)] = value
    return to_words(copied, dst_words), to_words(flags, dst_words), int(flags.sum()) - int(copied.sum())


def node_mask_model(labels, live, count, bitmap, nbits):
    """(the (count + 63) / 64 mask words, their set bits): bit i = live bit i && labels[i] < nbits && filter bit labels[i]"""
    labels = np.asarray(labels, np.uint64)[:count]
    ok = to_bool(live)[:count].copy()
    ok &= labels < np.uint64(nbits)
    idx = np.nonzero(ok)[0]
    ok[idx] = to_bool(bitmap)[labels[idx].astype(np.int64)]
    return to_words(ok, words_of(count)), int(ok.sum())


def scatter_model(dst, src, idx):
    out = dst.copy()
    out[np.asarray(idx, np.int64)] = src
    return out


def gather_model(src, idx):
    return src[np.asarray(idx, np.int64)].copy()


# ---- the per-block partial sums, where the contract plus the geometry decide them --------------------------------------------
def combine_partials(dst, blocks):
    """filter_combine: block b owns the words i with (i / 256) % blocks == b"""
    out = np.zeros(blocks, np.int64)
    if len(dst):
        np.add.at(out, (np.arange(len(dst)) // THREADS) % blocks, popcounts(dst))
    return out


def set_ids_partials(bits_in, nbits, ids, blocks):
    """filter_set_ids: block b counts the new bits its ids (i / 256) % blocks == b turn on -- decided only when no new bit is
    named from two blocks (else whichever block's atomic comes first counts it): None then"""
    ids = np.asarray(ids, np.uint64)
    blk = (np.arange(len(ids)) // THREADS) % blocks
    ok = ids < np.uint64(nbits)
    idv, blk = ids[ok].astype(np.int64), blk[ok]
    fresh = ~to_bool(bits_in)[idv]
    idv, blk = idv[fresh], blk[fresh]
    pairs = np.unique(np.stack([idv, blk], axis=1), axis=0) if len(idv) else np.zeros((0, 2), np.int64)
    if len(pairs) != len(np.unique(idv)):
        return None
    out = np.zeros(blocks, np.int64)
    np.add.at(out, pairs[:, 1], 1)
    return out


def set_runs_partials(bits_in, nbits, runs, blocks):
    """filter_set_runs: wave r % waves serves run r, four waves to a block -- decided only when no two runs share a bit"""
    edge = np.zeros(nbits + 1, np.int64)
    kept = []
    for r, (lo, hi) in enumerate(runs):
        lo, hi = int(lo), int(hi)
        if lo > hi or lo >= nbits:
            continue
        hi = min(hi, nbits - 1)
        edge[lo] += 1
        edge[hi + 1] -= 1
        kept.append((r, lo, hi))
    if nbits and np.cumsum(edge).max() > 1:
        return None
    fresh = np.concatenate([[0], np.cumsum(~to_bool(bits_in)[:nbits])])
    out = np.zeros(blocks, np.int64)
    for r, lo, hi in kept:
        out[(r % (blocks * 4)) // 4] += fresh[hi + 1] - fresh[lo]
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------
PAD = 2   # words the cases put behind a bitmap's slack word (filter_build_probe.hip's kPad)


def dirty_bitmap(rng, nbits, density=0.0):
    """words_of(nbits) + 1 + PAD words: the set itself (empty, or random at `density`), and random words wherever the
    launchers must not write -- above nbits in the last word, the slack word, the pad"""
    w = words_of(nbits)
    bits = rng.integers(0, 1 << 63, size=w + 1 + PAD, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=w + 1 + PAD, dtype=np.uint64)
    inside = to_bool(bits[:w])
    inside[:nbits] = rng.random(nbits) < density if density else False
    bits[:w] = to_words(inside, w)
    return bits


def set_ids_cases():
    rng = np.random.default_rng(7101)
    cases = {}
    big = 1_000_003
    perm = rng.permutation(big).astype(np.uint64)
    for n in (0, 1, 255, 256, 257, 524_288, 524_289, 600_000):
        cases["n_%d" % n] = dict(nbits=big, bits=dirty_bitmap(rng, big), ids=perm[:n].copy(), why="distinct ids: partial sums decided",
                                 reach=dict(blocks=set_ids_blocks(n), trips=trips(n, set_ids_blocks(n))), exact_partials=True)
    for nbits in (1, 63, 64, 65, 4097, big):
        ids = rng.integers(0, 2 * nbits + 2, size=300, dtype=np.uint64)
        cases["nbits_%d" % nbits] = dict(nbits=nbits, bits=dirty_bitmap(rng, nbits), ids=ids, why="ids on both sides of nbits, repeats")
    cases["all_equal"] = dict(nbits=4097, bits=dirty_bitmap(rng, 4097), ids=np.full(1000, 5, np.uint64), why="one bit named 1000 times, four blocks")
    cases["one_word"] = dict(nbits=4097, bits=dirty_bitmap(rng, 4097), ids=rng.integers(64, 128, size=1000, dtype=np.uint64), why="every atomic on one word")
    for nbits in (4097, 4096):
        cases["edges_%d" % nbits] = dict(nbits=nbits, bits=dirty_bitmap(rng, nbits),
                                         ids=np.array([nbits - 1, nbits, nbits + 1, nbits + 63, 1 << 40, (1 << 40) + 7, M64, 0, 1 << 32, (1 << 32) + 3], np.uint64),
                                         why="nbits - 1 is the last bit; nbits, 2^40, 2^32 + 3 and 2^64 - 1 are ignored")
    cases["extend"] = dict(nbits=100_003, bits=dirty_bitmap(rng, 100_003, density=0.5), ids=rng.integers(0, 100_003, size=70_000, dtype=np.uint64),
                           why="a half-full set extended: only the new bits are counted")
    return cases


def set_runs_cases():
    rng = np.random.default_rng(7102)
    cases = {}

    def add(name, nbits, runs, why, density=0.0, **reach):
        runs = np.array(runs, np.uint64).reshape(-1, 2)
        n = len(runs)
        cases[name] = dict(nbits=nbits, bits=dirty_bitmap(rng, nbits, density), runs=runs, why=why,
                           reach=dict(blocks=set_runs_blocks(n), wave_trips=trips(n, set_runs_blocks(n), 4), **reach))

    def lane_trips(runs, nbits):
        return max([ceil_div((min(hi, nbits - 1) >> 6) - (lo >> 6) + 1, 64) for lo, hi in runs if lo <= hi and lo < nbits] or [0])

    add("single_bits", 4097, [(0, 0), (63, 63), (64, 64)], "single-bit runs at a word's first and last bit")
    add("whole_words", 4097, [(64, 127), (0, 63), (4032, 4095)], "runs of exactly one word")
    add("ends_on_last_bit", 4096, [(4000, 4095)], "hi & 63 == 63 in the last word: no shift by 64, nothing in the slack word")
    add("ignored", 4097, [(10, 9), (4097, 5000), (1 << 40, 1 << 41), (M64, M64), (M64, 0), (20, 20)], "lo > hi and lo >= nbits are skipped")
    add("clamped", 4097, [(4090, 4097), (4000, M64), (100, 1 << 40)], "hi >= nbits and hi = 2^64 - 1 are clamped to nbits - 1")
    add("nbits_0", 0, [(0, 0), (0, M64), (5, 9)], "an empty label space: every run is ignored")
    r = [(3, 5000)]
    add("long_4096", 100_003, r, "more than 64 words: the lane loop's second trip", lane_trips=lane_trips(r, 100_003))
    r = [(100, 100 + 64 * 64 * 3 + 50)]
    add("long_12288", 100_003, r, "more than 3 * 64 words: the lane loop's fourth trip", lane_trips=lane_trips(r, 100_003))
    for n in (1, 4, 5, 8192, 8193, 9000):
        nbits = 1_000_003
        # disjoint runs in shuffled order, some touching their neighbour's word: the partial sums are decided
        starts = np.sort(rng.choice(nbits // 100, size=n, replace=False)) * 100
        lens = rng.integers(0, 100, size=n)
        order = rng.permutation(n)
        add("n_%d" % n, nbits, [(int(starts[i]), int(starts[i] + lens[i])) for i in order], "disjoint runs: partial sums decided", density=0.2)
        cases["n_%d" % n]["exact_partials"] = True
    nbits = 100_003
    lo = rng.integers(0, nbits, size=9000)
    r = [(int(a), int(a + l)) for a, l in zip(lo, rng.integers(0, 300, size=9000))]
    add("overlapping_9000", nbits, r, "thousands of runs sharing words and bits across waves and blocks: the count stays exact", lane_trips=lane_trips(r, nbits))
    return cases


def popcount_cases():
    rng = np.random.default_rng(7103)
    cases = {}
    for words in (0, 1, 255, 256, 257, 524_289):
        cases["words_%d" % words] = dict(bits=rng.integers(0, 1 << 63, size=words, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=words, dtype=np.uint64),
                                         start=(1 << 40) + 5 + words, why="added onto a non-zero start" if words else "no launch: the value stays",
                                         reach=dict(blocks=grid_for(words), trips=trips(words, grid_for(words))))
    return cases


def random_words(rng, n):
    return rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)


def combine_cases():
    rng = np.random.default_rng(7104)
    cases = {}
    for words in (0, 1, 64, 257, 524_289):
        a, b = random_words(rng, words), random_words(rng, words)
        if words >= 257:          # a block whose words give no bit at all: its partial sum is a written zero
            a[0:256] = 0
            b[0:256] = 0
        for op in (0, 1, 2):
            cases["op%d_words_%d" % (op, words)] = dict(a=a, b=b, op=op, why="and / or / and-not, slack word, every block's partial sum",
                                                        reach=dict(blocks=combine_blocks(words), trips=trips(words, combine_blocks(words))))
    return cases


def combine_batch_cases():
    rng = np.random.default_rng(7105)
    cases = {}

    def add(name, n, words, n_ops, why):
        ops = random_words(rng, n_ops * words).reshape(n_ops, words)
        table = np.stack([rng.integers(0, n_ops, size=n), rng.integers(0, n_ops, size=n), np.arange(n) % 3], axis=1).astype(np.uint32)
        table[0, 1] = table[0, 0]                       # a == b
        if n > 1:
            table[1, :2] = table[0, :2]                 # two items over the same operands
        cases[name] = dict(ops=ops, table=table, words=words, starts=rng.integers(1, 1 << 62, size=n, dtype=np.uint64), why=why,
                           reach=dict(gx=combine_batch_gx(words), trips=trips(words, combine_batch_gx(words))))

    for n in (1, 3, 97):
        for words in (0, 1, 1024, 1025):
            add("n%d_words_%d" % (n, words), n, words, 4, "shared operands, a == b, counts added onto non-zero starts")
    add("n3_words_65537", 3, 65_537, 3, "gx capped at 64 and a second trip")
    add("n_65536", 65_536, 1, 2, "more items than gridDim.y holds: hipErrorInvalidValue, nothing written")
    cases["n_65536"]["refused"] = True
    return cases


def rec(label, item):
    return (int(item) << LABEL_BITS) | int(label)


def delta_cases():
    """name -> dict(items = [(base words or None, nbits)], clr, set = record lists, starts, copy_only)"""
    rng = np.random.default_rng(7106)
    cases = {}

    def add(name, items, clr, sets, why, copy_only=False, **reach):
        n = len(items)
        mx = max(words_of(nb) for _, nb in items)
        cases[name] = dict(items=items, clr=np.array(clr, np.uint64), set=np.array(sets, np.uint64), copy_only=copy_only, max_dst_words=mx,
                           starts=rng.integers(1, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2), why=why,
                           reach=dict(gx=delta_copy_gx(mx, n), copy_trips=trips(mx, delta_copy_gx(mx, n)),
                                      apply_trips=max(trips(len(clr), grid_for(len(clr))), trips(len(sets), grid_for(len(sets)))), **reach))

    def stray(words, nbits):
        """a base whose last word carries bits above nbits % 64"""
        b = random_words(rng, words)
        if words:
            b[-1] |= np.uint64(M64 ^ tail_mask(nbits))
        return b

    # ---- the copy alone
    add("copy_no_base", [(None, 1000)], [], [], "no base: zeros", copy_only=True)
    add("copy_same_words_stray", [(stray(16, 1000), 1000)], [], [], "base_words == dst_words, stray bits above nbits % 64 in the base's last word", copy_only=True)
    add("copy_grow", [(stray(7, 448), 1000)], [], [], "base_words < dst_words: zeros behind the base", copy_only=True)
    add("copy_nbits_0", [(stray(3, 192), 0)], [], [], "dst_words = 0: only the slack word", copy_only=True)
    add("copy_nbits_mod64_0", [(stray(16, 1024), 1024)], [], [], "nbits % 64 == 0: the last word whole", copy_only=True)
    items = []
    for i in range(300):
        nb = int(rng.integers(0, 5000 * 64)) if i % 10 else (0, 5000 * 64 - 1, 64, 63, 65)[(i // 10) % 5]
        bw = int(rng.integers(0, words_of(nb) + 1))
        items.append((stray(bw, nb) if i % 4 else None, nb))
    add("copy_batch_300", items, [], [], "300 items of 0 - 5000 words under one max_dst_words: gx = 8, more trips for the long, idle blocks for the short",
        copy_only=True)

    # ---- copy, clears, sets
    nb = 100_003
    base = stray(words_of(nb), nb)
    lab = rng.integers(0, nb, size=5000)
    add("one_item", [(base, nb)], [rec(l, 0) for l in lab[:2500]], [rec(l, 0) for l in lab[2000:]],
        "every wave holds one item; labels in both lists end up set; clears of unset and sets of set bits leave the count alone")
    n = 2000
    items = [(stray(4, 256) if i % 3 else None, 256) for i in range(n)]
    clr, sets = [], []
    for i in range(n):
        for out in (clr, sets):
            for _ in range(int(rng.integers(1, 4))):
                out.append(rec(rng.integers(0, 300), i))          # (labels up to 299: some beyond nbits)
    add("many_items", items, clr, sets, "dozens of items per wave, 1 - 3 records each: the per-lane atomic", items_per_wave=64 // 3)
    # (the far labels below stay on the device only because the kernel tests them: they are not mixed into the near case)
    items = [(stray(4, 200), 200), (None, 256), (stray(2, 70), 70)]
    near = [rec(l, i) for i, (_, nbi) in enumerate(items) for l in range(nbi, words_of(nbi) * 64 + 64)]
    inside = [rec(rng.integers(0, nbi), i) for i, (_, nbi) in enumerate(items) for _ in range(40)]
    add("past_nbits_near", items, near + inside, inside[::2] + near, "labels from nbits to the end of the slack word: all ignored on the device")
    far = [rec(l, i) for i in range(3) for l in ((1 << 40) - 1, (1 << 32) + 5, 1 << 39, 100_000)]
    add("past_nbits_far", items, far + inside, inside[::2] + far, "labels up to 2^40 - 1, and 2^32 + 5 whose low word is inside: all ignored on the device")
    nb = 4097
    dup = [rec(l, 0) for l in (5, 5, 5, 4096, 4096, 70, 70)] * 20 + [rec(l, 1) for l in (5, 5, 9)] * 30
    add("duplicates_tail", [(stray(65, nb), nb), (stray(65, nb), nb)], dup[:64 * 3 + 5], dup[::-1][:64 * 3 + 5],
        "the same label within a wave and across waves; 197 records: the last wave's tail is past n")
    nb = 1_000_003
    items = [(stray(words_of(nb), nb), nb), (None, nb), (stray(100, 6400), nb)]
    big = [rec(l, i) for i, l in zip(np.sort(rng.integers(0, 3, size=600_000)), rng.integers(0, nb + 50, size=600_000))]
    add("records_600000", items, big[:300_000] + big[500_000:], big, "more than 524 288 records: the record loop's second trip")
    items = [(None, 0)] * 65_535
    items[0], items[40_000], items[65_534] = (stray(2, 100), 100), (None, 130), (stray(3, 130), 130)
    r = [rec(l, i) for i in (0, 40_000, 65_534) for l in rng.integers(0, 140, size=50)]
    add("item_65534", items, r[::2], r[1::2], "the largest item index a record can carry, in a table of empty items")
    return cases


UNIVERSE = 6000   # the node mask cases draw their ordinary labels below it


def node_mask_cases():
    """name -> dict(labels, live, count, filters = [(bitmap words, nbits)], starts)"""
    rng = np.random.default_rng(7107)
    cases = {}
    universe = UNIVERSE

    def bitmap(nbits):
        return random_words(rng, words_of(nbits) + 1)   # (random above nbits too: the kernel's label < nbits is what keeps those out)

    def add(name, count, n, live_kind, why):
        labels = rng.integers(0, universe, size=count).astype(np.uint64)              # any order, repeats
        k = max(1, count // 8)
        labels[rng.choice(count, size=min(k, count), replace=False)] = np.uint64(1 << 40) - rng.integers(1, 50, size=min(k, count)).astype(np.uint64)
        labels[rng.integers(0, count)] = np.uint64((1 << 32) + 7)                     # low word 7: inside every non-empty filter
        nbits = [(0, universe // 2, universe + 100)[f % 3] if f < 3 or f % 5 == 0 else int(rng.integers(1, universe + 200)) for f in range(n)]
        for f in range(min(n, 4)):                                                    # a label equal to nbits
            if nbits[f]:
                labels[rng.integers(0, count)] = nbits[f]
        w = words_of(count)
        live = {"ones": np.full(w, M64, np.uint64), "zero": np.zeros(w, np.uint64), "random": random_words(rng, w)}[live_kind]
        cases[name] = dict(labels=labels, live=live, count=count, filters=[(bitmap(nb), nb) for nb in nbits],
                           starts=rng.integers(1, 1 << 62, size=n, dtype=np.uint64), why=why,
                           reach=dict(blocks=node_mask_blocks(count), groups=ceil_div(n, 64)))

    for count in (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 5003):
        add("count_%d" % count, count, 3, "random", "word, wave (512) and block (2048) edges; nbits 0, below and above the largest label")
    for n in (1, 63, 64, 65, 130):
        add("filters_%d" % n, 2500, n, "random", "the group loop of 64 filters, its count slots and their re-zeroing")
    add("live_zero", 700, 5, "zero", "nothing live: zeros written, counts untouched")
    add("live_ones", 700, 5, "ones", "live bits set past count too: the tail of the last word stays zero")
    add("filters_130_ones", 2049, 130, "ones", "three groups, two blocks")
    return cases


def rows_cases():
    """name -> dict(src [n][stride] u32, idx [n] a permutation's head, rows)"""
    rng = np.random.default_rng(7108)
    cases = {}
    for n, stride in [(1, 1), (1, 17), (1, 33), (257, 1), (257, 17), (257, 33), (31_800, 33)]:
        rows = n + 3
        cases["n%d_stride%d" % (n, stride)] = dict(src=rng.integers(0, 1 << 32, size=(n, stride), dtype=np.uint32), rows=rows,
                                                   idx=rng.permutation(rows)[:n].astype(np.uint32), why="a permutation; three rows untouched",
                                                   reach=dict(blocks=rows_blocks(n * stride), trips=trips(n * stride, rows_blocks(n * stride))))
    return cases


ALL = dict(set_ids=set_ids_cases, set_runs=set_runs_cases, popcount=popcount_cases, combine=combine_cases, combine_batch=combine_batch_cases,
           delta=delta_cases, node_mask=node_mask_cases, rows=rows_cases)
