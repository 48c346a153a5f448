"""Models and inputs shared by tests/test_flat_select_kernels_gpu.py (which runs them on the device) and
tests/test_flat_select_model_cpu.py (which checks the model and counts which kernel path every input reaches).

The selection model is one numpy statement: the real entries (label != kNoLabel) ordered by (float value with -0 == +0,
label), the first min(k, real) of them.  The path models restate the documented branch conditions of
csrc/flat_scan.hip -- the 256-entry sample of merge_select_kernel, the solo / walking / 8-block split of
flat_rerank_kernel -- from its comments and constants, not from its arithmetic."""
import numpy as np

NO_LABEL = 0xFFFFFFFFFFFFFFFF
INF_BITS = 0x7F800000
FILLS = [0x00000000, 0xFFFFFFFF, 0x7F7FFFFF]          # the three patterns of tests/test_flat_filter_stages_gpu.py
SEL_MAX = 4096                                       # kMergeSelectMax: the selection serves e == 1 up to here
SEL_SURVIVORS = 256                                  # kSelSurvivors
SPILL_CHUNK, SPILL_PER_QUERY = 4096, 32              # kernels.hpp
RERANK_SOLO_MAX, RERANK_PARTS, RERANK_SLOTS = 2048, 8, 576


def order_key(d):
    """order-preserving u32 of a float, -0 == +0 (no NaN reaches a merge)"""
    u = np.ascontiguousarray(d, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def select_model(dist, label, k):
    """indices of the answer, in order: real entries by (value, label), the first min(k, real)"""
    real = np.flatnonzero(label != np.uint64(NO_LABEL))
    return real[np.lexsort((label[real], order_key(dist[real])))][:k]


# ---- merge inputs --------------------------------------------------------------------------------------------------------
VALUE_CLASSES = ["distinct", "equal", "tie_straddle", "zeros", "inf", "few_real", "none"]
PLACEMENTS = ["sample_smallest", "sample_largest", "sample_few_real", "survivors_256", "survivors_257"]


def sample_positions(total):
    """entries wave 0 of merge_select_kernel holds in its first four registers: 0..63, 256..319, 512..575, 768..831"""
    e = np.arange(min(total, 1024))
    return e[(e % 256) < 64]


def spread_labels(rng, n):
    """n distinct labels over all 64 bits: every combination of bits 63, 32 and 31 occurs, the low bits are random"""
    low = rng.choice(1 << 20, n, replace=False).astype(np.uint64)
    hi = np.arange(n, dtype=np.uint64) % np.uint64(8)
    lab = low | ((hi & np.uint64(1)) << np.uint64(31)) | (((hi >> np.uint64(1)) & np.uint64(1)) << np.uint64(32)) | (
        ((hi >> np.uint64(2)) & np.uint64(1)) << np.uint64(63))
    lab |= (rng.integers(0, 1 << 30, n).astype(np.uint64) << np.uint64(33)) & np.uint64(0x7FFFFFFE00000000)
    return rng.permutation(lab)


def merge_values(cls, total, k, rng):
    """(dist f32 [total], label u64 [total]) of one query's partial lists, in entry order"""
    lab = spread_labels(rng, total)
    d = np.unique(rng.standard_normal(2 * total + 8).astype(np.float32))          # distinct, negative ones among them
    d = rng.permutation(d)[:total].copy()
    assert d.size == total
    if cls == "distinct":
        pass
    elif cls == "equal":
        d[:] = np.float32(0.5)
    elif cls == "tie_straddle":                       # the entries around the k-th place share one value
        o = np.argsort(d)
        lo, hi = max(0, min(k, total) - 3), min(total, k + 4)
        d[o[lo:hi]] = d[o[lo]]
    elif cls == "zeros":                              # -0 and +0 are one value; a few entries on either side
        d = rng.choice(np.array([-0.0, 0.0, -0.0, 0.0, -1.5, 2.5], np.float32), total).astype(np.float32)
    elif cls == "inf":                                # real entries at +inf, the k-th place among them
        o = rng.permutation(total)
        d[o[max(0, min(k, total) - 3):]] = np.float32(np.inf)
    elif cls == "few_real":                           # fewer real entries than k, the empty ones scattered as K3 leaves them
        real = max(0, min(k, total) - 1 - int(rng.integers(0, 3)))
        o = rng.permutation(total)[real:]
        d[o] = np.float32(np.inf)
        lab[o] = np.uint64(NO_LABEL)
    elif cls == "none":
        d[:] = np.float32(np.inf)
        lab[:] = np.uint64(NO_LABEL)
    else:
        raise ValueError(cls)
    return d, lab


def placed_values(place, total, k, rng):
    """distinct values arranged against the sample; None where the arrangement does not exist at this size"""
    S = sample_positions(total)
    rest = np.setdiff1d(np.arange(total), S)
    d, lab = merge_values("distinct", total, k, rng)
    o = np.argsort(d)                                 # rank -> entry (values distinct)
    dv, lv = d[o], lab[o]                             # by rank
    n_s = S.size

    if place == "sample_smallest":                    # the k smallest are in the sample: U = the k-th smallest of all
        if n_s < k or rest.size == 0:
            return None
        ranks = np.concatenate([np.arange(k), k + rng.choice(total - k, n_s - k, replace=False)])
    elif place == "sample_largest":                   # the sample holds the largest values: nearly everything survives U
        if rest.size == 0:
            return None
        ranks = np.arange(total - n_s, total)
    elif place == "sample_few_real":                  # fewer than k real entries in the sample, k or more outside it
        if rest.size < k or n_s == 0:
            return None
        ranks = np.arange(total - n_s, total)
    elif place in ("survivors_256", "survivors_257"):
        # the sample's k-th smallest is the entry of rank 256 (257) of all: exactly that many entries have key <= U
        r = 255 if place == "survivors_256" else 256
        if n_s < k or total - (r + 1) < n_s - k:
            return None
        ranks = np.concatenate([np.arange(k - 1), [r], r + 1 + rng.choice(total - r - 1, n_s - k, replace=False)])
    else:
        raise ValueError(place)
    ranks = np.asarray(ranks, np.int64)
    other = np.setdiff1d(np.arange(total), ranks)
    out_d, out_l = np.empty_like(d), np.empty_like(lab)
    p = rng.permutation(ranks)
    out_d[S], out_l[S] = dv[p], lv[p]
    p = rng.permutation(other)
    out_d[rest], out_l[rest] = dv[p], lv[p]
    if place == "sample_few_real":                    # empty all of the sample but k - 1 entries
        gone = S[rng.permutation(n_s)[max(0, k - 1):]]
        out_d[gone] = np.float32(np.inf)
        out_l[gone] = np.uint64(NO_LABEL)
    return out_d, out_l


def merge_queries(total, k, seed=0, placements=True):
    """[(name, dist, label)]: one query per value class and per placement that exists at (total, k)"""
    rng = np.random.default_rng([total, k, seed])
    out = [(c, *merge_values(c, total, k, rng)) for c in VALUE_CLASSES]
    if placements:
        for p in PLACEMENTS:
            v = placed_values(p, total, k, rng)
            if v is not None:
                out.append((p, *v))
    return out


def select_path(dist, label, k):
    """what merge_select_kernel does with one query: (path, sample has fewer real entries than k, survivors of the sample's bound)

    real = entries with a label; k' = min(k, real); wave 0's sample = sample_positions; U = its k'-th smallest key when it
    has k' real entries, else 0xFFFFFFFF; survivors = real entries with key <= U; the fast path takes up to 256 of them."""
    real = label != np.uint64(NO_LABEL)
    kk = min(k, int(real.sum()))
    if kk == 0:
        return "empty", False, 0
    key = np.where(real, order_key(dist), np.uint32(0xFFFFFFFF))
    S = sample_positions(dist.size)
    skeys = np.sort(key[S][real[S]])
    few = skeys.size < kk
    U = 0xFFFFFFFF if few else int(skeys[kk - 1])
    survivors = int((real & (key <= U)).sum())
    return ("fast" if survivors <= SEL_SURVIVORS else "general"), few, survivors


SELECT_TOTALS = [1, 63, 64, 65, 255, 256, 257, 1024, 4095, 4096]
SELECT_KS = [1, 10, 15, 16, 63, 64]


# ---- re-rank inputs ------------------------------------------------------------------------------------------------------
def rerank_path(n, cand_cap, prune, spill=True):
    """the path flat_rerank_kernel takes for a list of n survivors: 'registers' (one block, the list in registers), 'walking'
    (one block walks a list longer than what the registers hold), 'blocks' (eight blocks, a partial list each); and whether
    a wave's kept entries can pass the 512 waiting slots so that flush() runs inside the walk (needs every entry kept)"""
    n = min(n, cand_cap + (SPILL_PER_QUERY * SPILL_CHUNK if spill else 0))
    n_sel = min(n, 2048, cand_cap)
    if n <= RERANK_SOLO_MAX:
        path = "registers" if n <= n_sel else "walking"
        waves = 4
    else:
        path, waves = "blocks", 4 * RERANK_PARTS
    per = -(-n // waves)
    flush = path != "registers" and per + 64 > RERANK_SLOTS and not prune
    return path, flush


def rerank_counts(k):
    return sorted({0, 1, max(k - 1, 0), k, k + 1, 16, 17, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 2100})


RERANK_SMALL_CAP = 256
RERANK_SMALL_CAP_COUNTS = [255, 256, 257, 1000, RERANK_SMALL_CAP + SPILL_CHUNK - 1, RERANK_SMALL_CAP + SPILL_CHUNK, RERANK_SMALL_CAP + SPILL_CHUNK + 1]
RERANK_LONG = 20000
