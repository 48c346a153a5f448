"""The case table of the filter expansion kernels (csrc/filter_expand.hip), shared by tests/test_filter_expand_kernels_gpu.py
(which runs it on the device) and tests/test_filter_expand_model_cpu.py (which pins that every case crosses the threshold it
is named for).  The tile constants are restated here; the CPU test checks them against the source text and the GPU test
against what the probe exports."""
import numpy as np

THREADS = 256                       # kExpandThreads
ROWS = 4                            # kExpandRows
TILE_WORDS = THREADS * ROWS         # kExpandTileWords
TILE_BITS = TILE_WORDS * 64
SCAN_TRIP = 256                     # kExpandScanTrip: tiles per trip of the scan block


def tiles(nbits):
    return (((nbits + 63) // 64) + TILE_WORDS - 1) // TILE_WORDS


# name -> nbits
SIZES = {
    "one_bit": 1,
    "word_minus_1": 63,
    "word": 64,
    "word_plus_1": 65,
    "tile_minus_1": TILE_BITS - 1,
    "tile": TILE_BITS,
    "tile_plus_1": TILE_BITS + 1,
    "three_tiles_plus_5": 3 * TILE_BITS + 5,
    "second_scan_trip": SCAN_TRIP * TILE_BITS + 3 * 64 + 7,     # 257 tiles: 2 MiB of bitmap
}
PATTERNS = ("empty", "full", "bit0", "last_bit", "alt_words", "sparse", "half")


def words_of(nbits):
    return (nbits + 63) // 64


def make_bits(pattern, nbits, seed=0):
    """(nbits + 63) // 64 + 1 words (the slack word last), with RANDOM bits at or above nbits in the last word and in the
    slack word -- whatever the pattern: the kernels must ignore them."""
    rng = np.random.default_rng(seed * 1000003 + nbits % 999983)
    w = words_of(nbits)
    bits = np.zeros(w + 1, np.uint64)
    if pattern == "empty":
        pass
    elif pattern == "full":
        bits[:w] = ~np.uint64(0)
    elif pattern == "bit0":
        bits[0] = 1
    elif pattern == "last_bit":
        bits[(nbits - 1) // 64] = np.uint64(1) << np.uint64((nbits - 1) % 64)
    elif pattern == "alt_words":
        bits[0:w:2] = ~np.uint64(0)
    elif pattern in ("sparse", "half"):
        p = 1e-4 if pattern == "sparse" else 0.5
        flags = rng.random(w * 64) < p
        bits[:w] = np.packbits(flags, bitorder="little").view(np.uint64)
    else:
        raise ValueError(pattern)
    tail = nbits % 64
    stray = rng.integers(0, 2**63, 2, dtype=np.uint64) | np.uint64(1 << 63)
    if tail:
        low = (np.uint64(1) << np.uint64(tail)) - np.uint64(1)
        bits[w - 1] = (bits[w - 1] & low) | (stray[0] & ~low)
    bits[w] = stray[1]
    return bits


def expected(bits, nbits):
    """numpy.flatnonzero of the bits below nbits, as u64"""
    w = words_of(nbits)
    flags = np.unpackbits(bits[:w].view(np.uint8), bitorder="little")[:nbits]
    return np.flatnonzero(flags).astype(np.uint64)


def caps(total):
    return sorted({0, max(total - 1, 0), total, total + 1})


# the one case near 2^32: nbits just above 2^32, a handful of bits near both ends (a 512 MiB bitmap that exists on the
# device only: the probe writes these words into zeroed memory)
BIG_NBITS = (1 << 32) + 70
BIG_LABELS = [0, 1, 63, 64, 65535, 65536, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) + 69]
BIG_STRAY = [(1 << 32) + 70, (1 << 32) + 100, (1 << 32) + 127, (1 << 32) + 128 + 5]   # above nbits: last word, slack word


def big_words():
    """(word indices, word values, allocated words) of the 2^32 case"""
    words = {}
    for b in BIG_LABELS + BIG_STRAY:
        words[b // 64] = words.get(b // 64, 0) | (1 << (b % 64))
    idx = sorted(words)
    return np.array(idx, np.uint64), np.array([words[i] for i in idx], np.uint64), words_of(BIG_NBITS) + 1
