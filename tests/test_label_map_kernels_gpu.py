"""The kernels of the device label map (csrc/label_map.hip; option prefilter-device-resolve) on their own, through
tests/helpers/label_map_probe.hip -- a small library that includes that translation unit, built with the library's flags, so
the product's kernels and launchers run, on buffers the test owns.

Every case runs three times: before the build the table, the outputs and the scratch are filled with 0x00000000, 0xFFFFFFFF
and 0x7F7FFFFF in turn, and only what the product's launchers initialise themselves is initialised.  The three results must be
equal, and equal to a Python dict (tests/helpers/label_map_cases.py; tests/test_label_map_model_cpu.py pins the restated hash
and checks that each case reaches the path it is there for).  Which bucket of its probe run a label ends in depends on the order
the threads claim buckets in, so the TABLE is compared as a mapping {label: slot} plus the linear-probing invariant (no empty
bucket between a label's first bucket and its place); everything the resolve writes is compared word for word: slots, kept
positions, segment offsets, tile offsets.  The probe polls the stream with a time limit: a kernel that spins is a failure."""
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
LIB = HERE / "liblabelmapprobe.so"
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]      # csrc/Makefile's
FILLS = (0x00000000, 0xFFFFFFFF, 0x7F7FFFFF)

sys.path.insert(0, str(HERE))
import label_map_cases as LM  # noqa: E402


def build_probe():
    src = HERE / "label_map_probe.hip"
    newest = max(p.stat().st_mtime for p in (src, CSRC / "label_map.hip", CSRC / "label_map_hash.hpp", CSRC / "kernels.hpp",
                                             CSRC / "device_common.hpp"))
    if not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "-shared", "-fPIC", "-I", str(CSRC), str(src),
                               "-o", str(LIB)])
    return LIB


class Probe:
    def __init__(self):
        lib = C.CDLL(str(build_probe()))
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        lib.lm_probe_run.argtypes = [u32, vp, u32, vp, u32, u64, vp, vp, vp, vp, u32, vp, u32, vp, vp, vp, vp]
        lib.lm_probe_run.restype = C.c_int
        lib.lm_probe_capacity.argtypes = [u64]
        lib.lm_probe_capacity.restype = u64
        lib.lm_probe_bucket.argtypes = [u64, u64]
        lib.lm_probe_bucket.restype = u64
        self.lib = lib

    def run(self, fill, labels, tomb, capacity, keys=None, list_begin=None):
        """one build (+ one resolve): (table keys, table vals, failure word[, seg, tile, slot, pos])"""
        n = len(labels)
        lab = np.array(labels, np.uint64)
        stride = 5
        links = None
        if tomb is not None:   # a level-0 table: word 0 = neighbour count | tombstone bit, the rest neighbour ids
            links = np.full((n, stride), 0xABCD, np.uint32)
            links[:, 0] = 3
            links[np.array(tomb, bool), 0] |= LM.TOMBSTONE
        tk, tv, tf = np.zeros(capacity, np.uint64), np.zeros(capacity, np.uint32), np.zeros(1, np.uint32)
        ns = 0 if keys is None else len(list_begin) - 1
        ky = np.array(keys if keys is not None else [], np.uint64)
        lb = np.array(list_begin if keys is not None else [0], np.uint32)
        seg, tile = np.zeros(ns + 1, np.uint32), np.zeros(ns + 1, np.uint32)
        slot, pos = np.zeros(max(ky.size, 1), np.uint32), np.zeros(max(ky.size, 1), np.uint32)
        rc = self.lib.lm_probe_run(fill, lab.ctypes.data, n, None if links is None else links.ctypes.data, stride, capacity, tk.ctypes.data,
                                   tv.ctypes.data, tf.ctypes.data, ky.ctypes.data, ky.size, lb.ctypes.data, ns, seg.ctypes.data, tile.ctypes.data,
                                   slot.ctypes.data, pos.ctypes.data)
        assert rc != 2, "a label map launch did not finish within the probe's time limit"
        assert rc == 0, "lm_probe_run refused its arguments" if rc == 1 else f"HIP error seen at label_map_probe.hip:{rc}"
        if keys is None:
            return tk, tv, int(tf[0])
        total = int(seg[ns])
        assert total <= ky.size
        return tk, tv, int(tf[0]), seg.tolist(), tile.tolist(), slot[:total].tolist(), pos[:total].tolist()


@pytest.fixture(scope="module")
def probe():
    return Probe()


def test_the_probe_runs_the_restated_hash(probe):
    for count in (0, 1, 8, 9, 63, 64, 65, 5000, 1 << 20):
        assert probe.lib.lm_probe_capacity(count) == LM.capacity_for(count)
    for label in (0, 1, LM.M64 - 1, 1 << 63, 0x123456789ABCDEF0):
        for cap in (16, 1 << 14, 1 << 32):
            assert probe.lib.lm_probe_bucket(label, cap) == LM.bucket(label, cap)


BUILD = LM.build_cases()


@pytest.mark.parametrize("name", sorted(BUILD))
def test_build(probe, name):
    case = BUILD[name]
    want, want_fails = LM.build_model(case["labels"], case["tomb"])
    assert want_fails == case.get("fails", 0)
    seen = []
    for fill in FILLS:
        tk, tv, fails = probe.run(fill, case["labels"], case["tomb"], case["capacity"])
        got, used = LM.table_as_dict(tk, tv)
        assert used == len(got), "a label is stored twice"
        assert fails == want_fails, hex(fill)
        if want_fails == 0:
            assert got == want, hex(fill)
        else:   # which slot of a repeated label wins is not defined: the labels, and a slot that carries the label
            assert sorted(got) == sorted(want), hex(fill)
            assert all(case["labels"][s] == l for l, s in got.items())
        longest, wraps = LM.longest_probe(tk, case["capacity"])
        assert longest >= case.get("min_probe", 0) and (wraps or not case.get("wraps", False))
        seen.append(sorted(got) if want_fails else got)
    assert seen[0] == seen[1] == seen[2]


RESOLVE = LM.resolve_cases()


@pytest.fixture(scope="module")
def world():
    labels, tomb, _ = LM.resolve_world()
    table, fails = LM.build_model(labels, tomb)
    assert fails == 0
    return labels, tomb, table


@pytest.mark.parametrize("name", sorted(RESOLVE))
def test_resolve(probe, world, name):
    labels, tomb, table = world
    keys, lb = RESOLVE[name]
    want = LM.resolve_model(table, keys, lb)
    seen = []
    for fill in FILLS:
        tk, tv, fails, seg, tile, slot, pos = probe.run(fill, labels, tomb, LM.capacity_for(len(labels)), keys, lb)
        assert fails == 0 and LM.table_as_dict(tk, tv)[0] == table
        assert (seg, tile, slot, pos) == want, hex(fill)
        seen.append((seg, tile, slot, pos))
    assert seen[0] == seen[1] == seen[2]


def test_resolve_against_a_table_with_long_runs(probe):
    """lookups that walk a 70-label run, and one that wraps the table's end: known labels at the run's far end, and unknown
    labels of the same bucket, which walk the whole run to the first empty bucket"""
    for name in ("collide_70", "wrap"):
        case = BUILD[name]
        table, _ = LM.build_model(case["labels"], None)
        cap = case["capacity"]
        b = LM.bucket(case["labels"][0], cap)
        strangers = LM.colliding_labels(cap, b, 5, start=1 << 45)
        assert not set(strangers) & set(table)
        keys = case["labels"][::-1] + strangers + case["labels"][:3]
        lb = [0, len(keys)]
        want = LM.resolve_model(table, keys, lb)
        for fill in FILLS:
            got = probe.run(fill, case["labels"], None, cap, keys, lb)
            assert tuple(got[3:]) == want, (name, hex(fill))
