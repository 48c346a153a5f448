"""The kernels that expand a device filter's bitmap into the ascending list of its labels (csrc/filter_expand.hip) on their
own, through tests/helpers/filter_expand_probe.hip -- a small library that includes that translation unit, built with the
library's flags, so the product's kernels and launcher run, on buffers the test owns.

Every case runs three times, from output and scratch buffers filled with 0x00000000, 0xFFFFFFFF and 0xEEEEEEEE, at the
capacities 0, total - 1, total and total + 1.  The WHOLE output buffer (cap + 3 entries) is held: its first min(total, cap)
entries equal numpy.flatnonzero of the bits below nbits, every entry behind them still holds the fill, and the total word is
exact.  Every bitmap carries random bits at or above nbits in its last word and in the slack word behind it.  The sizes and
patterns are tests/helpers/filter_expand_cases.py's (tests/test_filter_expand_model_cpu.py pins that each crosses the
threshold it is named for).  The probe polls the stream with a time limit: a kernel that spins is a failure."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "helpers"
CSRC = ROOT / "valkey-search_amd" / "csrc"
LIB = HERE / "libfilterexpandprobe.so"
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]      # csrc/Makefile's
FILLS = (0x00000000, 0xFFFFFFFF, 0xEEEEEEEE)
PAD = 3

sys.path.insert(0, str(HERE))
import filter_expand_cases as FE  # noqa: E402


def build_probe():
    src = HERE / "filter_expand_probe.hip"
    newest = max(p.stat().st_mtime for p in (src, CSRC / "filter_expand.hip", CSRC / "kernels.hpp", CSRC / "device_common.hpp"))
    if not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "-shared", "-fPIC", "-I", str(CSRC), str(src),
                               "-o", str(LIB)])
    return LIB


@pytest.fixture(scope="module")
def probe():
    lib = C.CDLL(str(build_probe()))
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    lib.fe_probe_run.argtypes = [u32, vp, u64, u64, u64, u64, vp, vp]
    lib.fe_probe_run.restype = C.c_int
    lib.fe_probe_run_sparse.argtypes = [u32, u64, vp, vp, u64, u64, u64, u64, vp, vp]
    lib.fe_probe_run_sparse.restype = C.c_int
    for f in (lib.fe_probe_tile_words, lib.fe_probe_scan_trip):
        f.restype = u32
    lib.fe_probe_tiles.argtypes = [u64]
    lib.fe_probe_tiles.restype = u32
    return lib


def check(out, total_word, want, cap, fill):
    fill64 = np.uint64(fill | (fill << 32))
    n = min(len(want), cap)
    assert total_word == len(want)
    assert np.array_equal(out[:n], want[:n])
    assert np.all(out[n:] == fill64), np.flatnonzero(out[n:] != fill64)[:8] + n


def test_the_probe_exports_the_restated_constants(probe):
    assert probe.fe_probe_tile_words() == FE.TILE_WORDS and probe.fe_probe_scan_trip() == FE.SCAN_TRIP
    for nbits in list(FE.SIZES.values()) + [0, FE.BIG_NBITS]:
        assert probe.fe_probe_tiles(nbits) == FE.tiles(nbits)


@pytest.mark.parametrize("pattern", FE.PATTERNS)
@pytest.mark.parametrize("size", list(FE.SIZES))
def test_expansion_equals_flatnonzero_from_dirty_buffers(probe, size, pattern):
    nbits = FE.SIZES[size]
    bits = FE.make_bits(pattern, nbits, seed=len(size) + len(pattern))
    want = FE.expected(bits, nbits)
    for cap in FE.caps(len(want)):
        for fill in FILLS:
            out = np.empty(cap + PAD, np.uint64)
            total = C.c_uint64(0xDEAD)
            rc = probe.fe_probe_run(fill, bits.ctypes.data, len(bits), nbits, cap, len(out), out.ctypes.data, C.byref(total))
            assert rc == 0, rc
            check(out, total.value, want, cap, fill)


def test_labels_near_two_to_the_32(probe):
    """nbits just above 2^32, a handful of bits near both ends and around 2^31 / 2^32, stray bits above nbits in the last word
    and in the slack word: the labels are u64 all the way (a 512 MiB bitmap, on the device only)."""
    idx, val, n_words = FE.big_words()
    want = np.array(sorted(FE.BIG_LABELS), np.uint64)
    for fill in FILLS:
        cap = len(want)
        out = np.empty(cap + PAD, np.uint64)
        total = C.c_uint64(0xDEAD)
        rc = probe.fe_probe_run_sparse(fill, n_words, idx.ctypes.data, val.ctypes.data, len(idx), FE.BIG_NBITS, cap, len(out),
                                       out.ctypes.data, C.byref(total))
        assert rc == 0, rc     # (3 = the device refused 512 MiB)
        check(out, total.value, want, cap, fill)
