"""The device label map's models on the CPU (-m "not gpu"): what tests/test_label_map_kernels_gpu.py compares the kernels with.

  * the hash and the sizing rule restated in tests/helpers/label_map_cases.py against csrc/label_map_hash.hpp itself, through
    tests/helpers/label_map_hash_main.cc -- a stand-alone program with its own main, built with -fsanitize=address,undefined
    (no Python process loads sanitized code);
  * the dict model's compaction against a second, independent statement of it;
  * the collision sets really collide, and each case reaches the path it is there for: a probe run longer than a wave, a run
    that wraps the table's end, the minimum capacity, every tile edge, unknown labels first / middle / last, ...
  * the option table and the header carry the option and the grown statistics struct.
"""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"
HELP = ROOT / "tests" / "helpers"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}

sys.path.insert(0, str(HELP))
import label_map_cases as LM  # noqa: E402

LABELS = [0, 1, 2, 63, 64, LM.M64 - 1, LM.M64, 1 << 31, 1 << 32, 1 << 63, (1 << 63) | (1 << 31), 0x123456789ABCDEF0, 0xDEADBEEF, 10 ** 19]
COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 5000, 8192, 8193, 10_000_000, 1 << 31]


@pytest.fixture(scope="module")
def host_values(tmp_path_factory):
    exe = tmp_path_factory.mktemp("label_map") / "label_map_hash_san"
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", str(CSRC), str(HELP / "label_map_hash_main.cc"), "-o", str(exe)])
    p = subprocess.run([str(exe), *map(str, LABELS), "-c", *map(str, COUNTS)], env={**os.environ, **ENV}, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0 and "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]
    return [l.split() for l in p.stdout.splitlines()]


def test_the_restated_hash_is_the_headers(host_values):
    mixes = {int(r[1]): int(r[2]) for r in host_values if r[0] == "mix"}
    buckets = {(int(r[1]), int(r[2])): int(r[3]) for r in host_values if r[0] == "bucket"}
    caps = {int(r[1]): int(r[2]) for r in host_values if r[0] == "capacity"}
    assert sorted(mixes) == sorted(LABELS) and sorted(caps) == sorted(COUNTS) and len(buckets) == 6 * len(LABELS)
    for l in LABELS:
        assert LM.mix(l) == mixes[l], l
    assert LM.mix_np(np.array(LABELS, np.uint64)).tolist() == [mixes[l] for l in LABELS]
    for (l, c), b in buckets.items():
        assert LM.bucket(l, c) == b < c
    for n in COUNTS:
        c = caps[n]
        assert LM.capacity_for(n) == c and c >= max(2 * n, LM.MIN_CAPACITY) and c & (c - 1) == 0 and (c == LM.MIN_CAPACITY or c < 4 * n)
    assert mixes[0] == 0 and LM.mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF     # splitmix64 seeded with 0: its first output


def test_the_header_is_shared_by_host_and_device():
    text = (CSRC / "label_map_hash.hpp").read_text()
    assert "#include <hip" not in text
    assert '#include "label_map_hash.hpp"' in (CSRC / "label_map.hip").read_text()
    assert "0xBF58476D1CE4E5B9" in text and "0x94D049BB133111EB" in text


def test_the_constants_are_the_kernels():
    hip = (CSRC / "label_map.hip").read_text()
    assert int(re.search(r"kKeyTile\s*=\s*(\d+)\s*;", hip).group(1)) == LM.KEY_TILE
    assert int(re.search(r"kDistTile\s*=\s*(\d+)\s*;", hip).group(1)) == LM.DIST_TILE
    assert int(re.search(r"kTombstone\s*=\s*(0x[0-9a-fA-F]+)u\s*;", hip).group(1), 16) == LM.TOMBSTONE
    sel = (CSRC / "prefilter_select.hip").read_text()
    assert int(re.search(r"kTileEntries\s*=\s*(\d+)\s*;", sel).group(1)) == LM.DIST_TILE
    graph = (CSRC / "hnsw_graph.hpp").read_text()
    assert int(re.search(r"kDeleteFlag\s*=\s*(0x[0-9a-fA-F]+)u\s*;", graph).group(1), 16) == LM.TOMBSTONE


def insert_sequentially(labels, tomb, capacity):
    """linear probing by the book, one slot after the other: the table a single thread would leave"""
    keys = np.full(capacity, LM.EMPTY, np.uint64)
    for i, l in enumerate(labels):
        if (tomb is not None and tomb[i]) or l == LM.EMPTY:
            continue
        h = LM.bucket(l, capacity)
        while keys[h] != np.uint64(LM.EMPTY) and keys[h] != np.uint64(l):
            h = (h + 1) % capacity
        keys[h] = l
    return keys


def test_build_cases_reach_their_paths():
    cases = LM.build_cases()
    assert {len(cases["count_%d" % n]["labels"]) for n in (0, 1, 63, 64, 65, 5000)} == {0, 1, 63, 64, 65, 5000}
    for name, c in cases.items():
        n = len(c["labels"])
        assert c["capacity"] >= LM.capacity_for(n), name
        table, fails = LM.build_model(c["labels"], c["tomb"])
        assert fails == c.get("fails", 0), name
        keys = insert_sequentially(c["labels"], c["tomb"], c["capacity"])
        longest, wraps = LM.longest_probe(keys, c["capacity"])
        assert longest >= c.get("min_probe", 0) and (wraps or not c.get("wraps", False)), (name, longest, wraps)
    assert sum(c["capacity"] == LM.capacity_for(len(c["labels"])) for c in cases.values()) >= 8      # the minimum capacity is there
    assert cases["roomy"]["capacity"] > LM.capacity_for(100)
    # the collision set really collides: 70 labels, one bucket
    c = cases["collide_70"]
    by_bucket = {}
    for l in c["labels"]:
        by_bucket.setdefault(LM.bucket(l, c["capacity"]), []).append(l)
    assert max(len(v) for v in by_bucket.values()) >= 70 and c["min_probe"] >= 64
    c = cases["wrap"]
    assert {LM.bucket(l, c["capacity"]) for l in c["labels"]} == {c["capacity"] - 3, c["capacity"] - 1}
    # extremes: 0, 2^64 - 2, and three pairs that differ in bit 63, 32, 31 only
    ex = cases["extremes"]["labels"]
    assert 0 in ex and LM.M64 - 1 in ex and len(set(ex)) == len(ex)
    for bit in (63, 32, 31):
        assert any(a ^ b == 1 << bit for a in ex for b in ex)
    # tombstones: some nodes out, one of them carrying a live node's label
    c = cases["tombstones"]
    table, fails = LM.build_model(c["labels"], c["tomb"])
    assert fails == 0 and len(table) == sum(not t for t in c["tomb"]) and table[c["labels"][100]] == 6
    assert cases["repeated"]["fails"] == 3


def resolve_by_hand(table, keys, lb):
    """a second statement of the compaction: per list, filter then count"""
    seg, tile, slot, pos = [0], [0], [], []
    for s in range(len(lb) - 1):
        kept = [(table[k], i) for i, k in enumerate(keys) if lb[s] <= i < lb[s + 1] and k in table and k != LM.EMPTY]
        slot += [a for a, _ in kept]
        pos += [b for _, b in kept]
        seg.append(seg[-1] + len(kept))
        tile.append(tile[-1] + -(-len(kept) // LM.DIST_TILE))
    return seg, tile, slot, pos


def test_resolve_cases_reach_their_paths_and_the_model_compacts():
    labels, tomb, unknown = LM.resolve_world()
    table, fails = LM.build_model(labels, tomb)
    assert fails == 0 and not set(unknown) & set(labels)
    cases = LM.resolve_cases()
    n_segs = set()
    for name, (keys, lb) in cases.items():
        assert lb[0] == 0 and lb[-1] == len(keys) and all(a <= b for a, b in zip(lb, lb[1:])), name
        got = LM.resolve_model(table, keys, lb)
        assert got == resolve_by_hand(table, keys, lb), name
        seg, tile, slot, pos = got
        assert all(keys[p] in table and table[keys[p]] == s for s, p in zip(slot, pos))
        assert pos == sorted(pos)                      # list order, list after list
        n_segs.add(len(lb) - 1)
    assert {1, 2, 257} <= n_segs
    keys, lb = cases["edges_csr"]
    lens = [b - a for a, b in zip(lb, lb[1:])]
    assert set(LM.SEG_LENGTHS) <= set(lens) and lens[1] == 0 and lens[3] == 0        # empty segments between full ones
    assert {len(cases["shared_%d" % n][0]) for n in LM.SEG_LENGTHS} == set(LM.SEG_LENGTHS)
    keys, lb = cases["unknown_places"]
    a = keys[lb[0]:lb[1]]
    assert a[0] not in table and a[150] not in table and a[-1] not in table and a[1] in table
    seg = LM.resolve_model(table, keys, lb)[0]
    assert seg[2] == seg[1]                                                      # the segment of unknown labels only
    c = keys[lb[2]:lb[3]]
    assert c.count(c[5]) >= 3 and LM.resolve_model(table, keys, lb)[2][seg[2]:seg[3]].count(table[c[5]]) >= 3   # duplicates kept
    assert keys[lb[4] - 1] == LM.EMPTY
    assert LM.resolve_model(table, *cases["all_unknown_shared"])[0] == [0, 0]
    # the kept counts hit both sides of a multiple of K8b's tile
    seg = LM.resolve_model(table, *cases["all_known_tiles"])[0]
    kept = [b - a for a, b in zip(seg, seg[1:])]
    assert kept == [63, 64, 65, 128, 129, 0, 64]
    assert {LM.resolve_model(table, *cases["all_known_shared_%d" % n])[0][1] for n in (63, 64, 65, 128, 129)} == {63, 64, 65, 128, 129}
    # a key tile (256) and a distance tile (64) both end inside, at and after a list somewhere
    assert any(n % LM.KEY_TILE == 1 for n in LM.SEG_LENGTHS) and any(n % LM.DIST_TILE == 63 for n in LM.SEG_LENGTHS)


def test_the_option_and_the_grown_struct_are_declared():
    assert '{"prefilter-device-resolve", nullptr, 0, 0, 1}' in (CSRC / "options.hpp").read_text()      # ships 0
    hdr = (ROOT / "include" / "vk_index.h").read_text()
    assert "prefilter-device-resolve" in hdr and "typedef struct vk_prefilter_stats_v2" in hdr
    for f in ("device_resolved_keys", "label_map_builds", "label_map_bytes"):
        assert f in hdr


def test_prefilter_stats_v2_layout_and_the_old_size(tmp_path):
    """vk_prefilter_stats_v2 against a C compiler (sizeof 80, every offset equal to the ctypes mirror's), its first 56 bytes the
    old struct field for field; and vk_index_prefilter_stats refuses every size but the two (no device needed)."""
    import ctypes as C
    import _pkg
    vsa = _pkg.vsa
    old = [f for f, _ in vsa.PrefilterStats._fields_]
    names = old + ["device_resolved_keys", "label_map_builds", "label_map_bytes"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vk_index.h"', 'int main(void){',
             'printf("size %zu %zu\\n", sizeof(vk_prefilter_stats), sizeof(vk_prefilter_stats_v2));']
    for f in names:
        lines.append(f'printf("{f} %zu\\n", offsetof(vk_prefilter_stats_v2, {f}));')
    for f in old:
        lines.append(f'printf("old.{f} %zu\\n", offsetof(vk_prefilter_stats, {f}));')
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    got = dict(l.split(None, 1) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert got["size"].split() == ["56", "80"] and C.sizeof(vsa.PrefilterStatsV2) == 80
    for f in names:
        assert int(got[f]) == getattr(vsa.PrefilterStatsV2, f).offset, f
    for f in old:
        assert int(got["old." + f]) == int(got[f]), f
    lib = vsa.lib()
    fake = C.create_string_buffer(256)
    s = vsa.PrefilterStatsV2()
    for size in (0, 8, 55, 57, 64, 79, 81, 88):
        s.struct_size = size
        assert lib.vk_index_prefilter_stats(C.cast(fake, C.c_void_p), C.cast(C.byref(s), C.POINTER(vsa.PrefilterStats))) == vsa.VK_ERR_INVALID, size
