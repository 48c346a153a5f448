"""Cases and the numpy model of the select + emit stages of csrc/flat_large_k.hip (tests/test_flat_large_k_kernels_gpu.py runs
them on the device, tests/test_flat_large_k_model_cpu.py pins the model against plain Python and that every case reaches the
path it is named for).  The constants restate the kernel file's; the GPU test asks the probe for them."""
import numpy as np

SLICE = 4096            # entries per block of the histogram / emit launches
DIST_BLOCKS = 2048      # row blocks of the distance launch, four waves of 16 rows each per trip
BINS = 2048
STATE_WORDS = 8         # T | k left | n_less | n_eq | n_real | emit counter | overflow flag | 0
NAN_POS, NAN_NEG = 0x7FC00000, 0xFFC00001
NO_LABEL = np.uint64(0xFFFFFFFFFFFFFFFF)

COUNTS = {"one": 1, "slice-1": SLICE - 1, "slice": SLICE, "slice+1": SLICE + 1, "slices": 3 * SLICE + 5}
CLASSES = ("random", "negative", "all_equal", "tie_inside", "tie_past", "pm_zero", "plus_inf", "fewer", "none", "nan_ends", "low_digit",
           "high_digit")


def slack(k):
    return max(1024, k // 4)


def cap_of(k):
    return k + slack(k)


def plan(nq, count, k, budget):
    """large_k_plan of flat_large_k_host.hpp: (fits, ld, queries per chunk, chunks)"""
    ld = (count + 63) & ~63
    if nq == 0 or count == 0 or ld * 4 > budget:
        return False, ld, 0, 0
    c = max(1, budget // (ld * 4 + cap_of(k) * 12))
    c = min(c, nq, 65535)
    if c >= 8:
        c &= ~7
    return True, ld, c, (nq + c - 1) // c


def ks(count):
    return sorted({k for k in (1, 1025, count - 1, count, count + 1) if k >= 1})


def key_of(bits):
    """merge_key of flat_scan.hip over float bits: order-preserving u32, -0 and +0 sharing a key"""
    b = np.asarray(bits, np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def is_nan(bits):
    b = np.asarray(bits, np.uint32)
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def labels_for(count, seed):
    rng = np.random.default_rng([count, seed, 5])
    lab = rng.integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2) + (np.arange(count, dtype=np.uint64) & np.uint64(1))
    lab = np.unique(lab)
    while lab.size < count:      # (a collision among 64-bit draws: practically never)
        lab = np.unique(np.concatenate([lab, rng.integers(0, 1 << 63, count, dtype=np.uint64)]))
    return rng.permutation(lab[:count])


def values(cls, count, k, seed):
    """[count] float bits of one query's distances; None where the class cannot be made at this (count, k)"""
    rng = np.random.default_rng([count, k, seed, CLASSES.index(cls)])
    cap = cap_of(k)
    f = rng.standard_normal(count).astype(np.float32)
    if cls == "random":
        pass
    elif cls == "negative":
        f = -np.abs(f) - np.float32(1)
    elif cls == "all_equal":
        f[:] = 1.5
    elif cls in ("tie_inside", "tie_past"):
        n_less = min(k - 1, count - 1)
        n_eq = cap - n_less + (1 if cls == "tie_past" else 0)
        if n_less + n_eq > count:
            if cls == "tie_past":
                return None
            n_eq = count - n_less
        f = np.float32(2) + np.abs(f)                      # the rest: beyond the tie group
        f[:n_less] = np.float32(-1) - np.abs(f[:n_less])   # n_less entries below it
        f[n_less:n_less + n_eq] = 0.5
        f = rng.permutation(f)
    elif cls == "pm_zero":
        f = (f * np.float32(1e-3)).astype(np.float32)
        z = rng.random(count)
        f[z < 0.3] = 0.0
        f[z > 0.7] = -0.0
    elif cls == "plus_inf":
        f[rng.random(count) < 0.5] = np.inf
    elif cls == "fewer":
        want = min(count, k) // 2
        if want < 1 or want >= k:
            return None
        b = f.view(np.uint32).copy()
        dead = rng.permutation(count)[want:]
        b[dead] = np.where(rng.random(dead.size) < 0.5, NAN_POS, NAN_NEG).astype(np.uint32)
        return b
    elif cls == "none":
        return np.where(rng.random(count) < 0.5, NAN_POS, NAN_NEG).astype(np.uint32)
    elif cls == "nan_ends":
        b = f.view(np.uint32).copy()
        b[0], b[count // 2], b[count - 1] = NAN_NEG, NAN_POS, NAN_NEG
        return b
    elif cls == "low_digit":
        return (np.uint32(0x3F800000) + rng.integers(0, 1024, count).astype(np.uint32)).astype(np.uint32)
    elif cls == "high_digit":
        return (rng.integers(1, 1000, count).astype(np.uint32) << np.uint32(21)).astype(np.uint32)   # positive, finite
    return np.ascontiguousarray(f).view(np.uint32).copy()


def case(count, k, seed=0):
    """(classes made, dist bits [n][count], labels [count]) for one probe call: one query per class"""
    made, rows = [], []
    for cls in CLASSES:
        v = values(cls, count, k, seed)
        if v is not None:
            made.append(cls)
            rows.append(v)
    return made, np.stack(rows), labels_for(count, seed)


def model(bits, labels, k, cap):
    """what the select and the emit must leave for one query: the state words and the emitted (bits, label) pairs, sorted"""
    real = ~is_nan(bits)
    key, lab, b = key_of(bits)[real], labels[real], np.asarray(bits, np.uint32)[real]
    order = np.lexsort((lab, key))          # THE statement: by key, then label
    n_real = int(real.sum())
    if n_real == 0:
        return [0, 0, 0, 0, 0, 0, 0, 0], np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    want = min(k, n_real)
    T = int(key[order][want - 1])
    n_less, n_eq = int((key < T).sum()), int((key == T).sum())
    flag = int(n_less + n_eq > cap)
    take = order[:n_less + n_eq]
    state = [T, want - n_less, n_less, n_eq, n_real, 0 if flag else n_less + n_eq, flag, 0]
    if flag:
        return state, np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    return state, b[take], lab[take]


def canon(bits, labels):
    """an emitted list in a canonical order: by label (labels are distinct)"""
    o = np.argsort(labels, kind="stable")
    return np.asarray(bits)[o], np.asarray(labels)[o]
