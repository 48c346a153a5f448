"""The case table of tests/test_filter_expand_kernels_gpu.py (tests/helpers/filter_expand_cases.py), without a device: the
restated tile constants equal the source text of csrc/filter_expand.hip, every size crosses the threshold it is named for,
and the patterns are what they say -- stray bits above nbits included -- so that the GPU test's expectation is the right one."""
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests" / "helpers"))
import filter_expand_cases as FE  # noqa: E402

SRC = (ROOT / "valkey-search_amd" / "csrc" / "filter_expand.hip").read_text()


def constant(name):
    m = re.search(r"constexpr uint32_t %s = ([^;]+);" % name, SRC)
    assert m, name
    return m.group(1).strip()


def test_restated_constants_equal_the_source():
    assert constant("kExpandThreads") == str(FE.THREADS)
    assert constant("kExpandRows") == str(FE.ROWS)
    assert constant("kExpandTileWords") == "kExpandThreads * kExpandRows"
    assert constant("kExpandScanTrip") == str(FE.SCAN_TRIP)
    assert FE.TILE_WORDS == FE.THREADS * FE.ROWS and FE.TILE_BITS == 64 * FE.TILE_WORDS


def test_every_size_crosses_its_threshold():
    S = FE.SIZES
    assert [S[n] for n in ("one_bit", "word_minus_1", "word", "word_plus_1")] == [1, 63, 64, 65]
    assert FE.words_of(S["word"]) == 1 and FE.words_of(S["word_plus_1"]) == 2
    assert FE.tiles(S["tile_minus_1"]) == 1 and S["tile_minus_1"] % 64 == 63          # a masked last word that fills the tile
    assert FE.tiles(S["tile"]) == 1 and S["tile"] % 64 == 0                           # no masked word, no second tile
    assert FE.tiles(S["tile_plus_1"]) == 2                                            # one bit in a second tile
    assert FE.tiles(S["three_tiles_plus_5"]) == 4 and S["three_tiles_plus_5"] % 64 == 5
    assert FE.tiles(S["second_scan_trip"]) == FE.SCAN_TRIP + 1                        # the scan block's second trip
    assert 2 << 20 <= FE.words_of(S["second_scan_trip"]) * 8 < 8 << 20                # "a few MB"
    assert FE.tiles(FE.BIG_NBITS) > FE.SCAN_TRIP * 255 and FE.BIG_NBITS > 1 << 32


def test_patterns_and_stray_bits():
    for name, nbits in FE.SIZES.items():
        if nbits > 4 * FE.TILE_BITS:
            continue
        w = FE.words_of(nbits)
        for pattern in FE.PATTERNS:
            bits = FE.make_bits(pattern, nbits, seed=1)
            assert len(bits) == w + 1 and bits[w] != 0                                # the slack word is dirty
            if nbits % 64:
                assert int(bits[w - 1]) >> (nbits % 64) != 0                          # ... and so is the last word's tail
            want = FE.expected(bits, nbits)
            assert want.dtype == np.uint64 and (len(want) == 0 or int(want[-1]) < nbits)
            assert np.all(np.diff(want.astype(np.int64)) > 0)
            if pattern == "empty":
                assert len(want) == 0
            elif pattern == "full":
                assert np.array_equal(want, np.arange(nbits, dtype=np.uint64))
            elif pattern == "bit0":
                assert want.tolist() == [0]
            elif pattern == "last_bit":
                assert want.tolist() == [nbits - 1]
            elif pattern == "alt_words":
                assert np.array_equal(want, np.array([i for i in range(nbits) if (i // 64) % 2 == 0], np.uint64))
    # densities of the random patterns, at a size where they mean something
    nbits = FE.SIZES["three_tiles_plus_5"]
    assert 0 < len(FE.expected(FE.make_bits("sparse", nbits), nbits)) < nbits * 5e-4
    assert 0.45 * nbits < len(FE.expected(FE.make_bits("half", nbits), nbits)) < 0.55 * nbits


def test_capacities_and_the_big_case():
    assert FE.caps(0) == [0, 1] and FE.caps(1) == [0, 1, 2] and FE.caps(10) == [0, 9, 10, 11]
    idx, val, n_words = FE.big_words()
    assert n_words == FE.words_of(FE.BIG_NBITS) + 1 and int(idx[-1]) == n_words - 1   # the slack word is written
    assert all(b < FE.BIG_NBITS for b in FE.BIG_LABELS) and all(b >= FE.BIG_NBITS for b in FE.BIG_STRAY)
    assert any(b // 64 == FE.words_of(FE.BIG_NBITS) - 1 for b in FE.BIG_STRAY)        # stray bits in the last word too
    assert min(FE.BIG_LABELS) == 0 and max(FE.BIG_LABELS) == FE.BIG_NBITS - 1
