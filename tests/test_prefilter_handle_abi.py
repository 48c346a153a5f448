"""The ABI of the exact kNN from a filter handle, without a device: the new symbols are exported, the Python binding's stats
mirror matches what a C compiler makes of include/vk_index.h (size and the offset of every field), the structs that must not
grow have not grown, the facade compiles, and the argument checks that need no device answer VK_ERR_INVALID."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = ("vk_index_search_filter_exact_batch", "vk_filter_read_labels", "vk_index_filter_exact_stats")


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    v = _pkg.vsa
    if not v.LIB_PATH.exists():
        v.build()
    return v


def test_the_new_symbols_are_declared_and_exported(vsa):
    text = (ROOT / "include" / "vk_index.h").read_text()
    lib = C.CDLL(str(vsa.LIB_PATH))
    for name in NEW:
        assert ("int %s(" % name) in text and hasattr(lib, name), name
    vsa.lib()      # (the binding resolves them too)


def test_stats_mirror_matches_the_header(vsa, tmp_path):
    mirrors = (("vk_filter_exact_stats", vsa.FilterExactStats), ("vk_prefilter_stats", vsa.PrefilterStats),
               ("vk_prefilter_stats_v2", vsa.PrefilterStatsV2), ("vk_index_stats", vsa.Stats), ("vk_index_params", vsa.Params))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vk_index.h"', 'int main(void){']
    for cname, mirror in mirrors:
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
    for fname, _ in vsa.FilterExactStats._fields_:
        lines.append(f'printf("f.{fname} %zu\\n", offsetof(vk_filter_exact_stats, {fname}));')
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for cname, mirror in mirrors:
        assert int(got[cname]) == C.sizeof(mirror), cname
    for fname, _ in vsa.FilterExactStats._fields_:
        assert int(got[f"f.{fname}"]) == getattr(vsa.FilterExactStats, fname).offset, fname
    assert [f for f, _ in vsa.FilterExactStats._fields_] == ["struct_size", "batches", "queries", "runs", "labels_expanded", "known_keys",
                                                             "candidates", "fallback_queries", "downloaded_runs"]
    # what must keep its size
    assert int(got["vk_index_stats"]) == 568 and int(got["vk_index_params"]) == 144
    assert int(got["vk_prefilter_stats"]) == 56 and int(got["vk_prefilter_stats_v2"]) == 80


def test_argument_validation_needs_no_device(vsa):
    lib = vsa.lib()
    q = np.zeros(4, np.float32)
    od, ol, on = np.full(2, 7.0, np.float32), np.full(2, 7, np.uint64), np.full(1, 7, np.uint64)
    tab = (C.c_void_p * 1)(None)
    assert lib.vk_index_search_filter_exact_batch(None, q.ctypes.data, 1, 2, tab, od.ctypes.data, ol.ctypes.data, on.ctypes.data) == vsa.VK_ERR_INVALID
    assert od.tolist() == [7.0, 7.0] and ol.tolist() == [7, 7] and on.tolist() == [7]
    n = C.c_uint64(7)
    assert lib.vk_filter_read_labels(None, ol.ctypes.data, 2, C.byref(n)) == vsa.VK_ERR_INVALID and n.value == 7
    s = vsa.FilterExactStats()
    s.struct_size = C.sizeof(vsa.FilterExactStats)
    assert lib.vk_index_filter_exact_stats(None, C.byref(s)) == vsa.VK_ERR_INVALID
    s.struct_size = 8
    assert lib.vk_index_filter_exact_stats(None, C.byref(s)) == vsa.VK_ERR_INVALID and b"struct_size" in lib.vk_last_error()
    assert lib.vk_index_filter_exact_stats(None, None) == vsa.VK_ERR_INVALID


def test_the_facade_method_compiles(vsa, tmp_path):
    src = tmp_path / "use.cc"
    src.write_text('#include "vk_algo.h"\n'
                   'template <class A> auto use(A &a, vk_filter *const *f) { return a.searchFilterExactBatch(nullptr, 0, 1, f); }\n'
                   'int main() { return 0; }\n')
    assert "searchFilterExactBatch" in (ROOT / "include" / "vk_algo.h").read_text()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)])
