"""The C ABI of the batched pre-filter search on the CPU (-m "not gpu"): vk_index_search_labels_batch and
vk_index_prefilter_stats are declared and exported, the ctypes mirror of vk_prefilter_stats matches what a C compiler makes
of the header, every argument error is reported before any device work (no device here), and the two structs whose sizes
other tests pin have not moved."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    v = _pkg.vsa
    if not v.LIB_PATH.exists():
        v.build()
    return v


def test_header_declares_and_library_exports_the_calls(vsa):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vk_index.h").read_text(), flags=re.S)
    lib = C.CDLL(str(vsa.LIB_PATH))
    for name in ("vk_index_search_labels_batch", "vk_index_prefilter_stats"):
        assert re.search(r"^\s*int\s+%s\s*\(" % name, text, flags=re.M), name
        assert hasattr(lib, name), name
    assert "typedef struct vk_prefilter_stats" in text


def test_prefilter_stats_layout_matches_header(vsa, tmp_path):
    names = ["struct_size", "batches", "queries", "keys", "candidates", "fallback_queries", "candidate_cap"]
    assert [f for f, _ in vsa.PrefilterStats._fields_] == names
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vk_index.h"', 'int main(void){',
             'printf("vk_prefilter_stats %zu\\n", sizeof(vk_prefilter_stats));']
    for f in names:
        lines.append(f'printf("vk_prefilter_stats.{f} %zu\\n", offsetof(vk_prefilter_stats, {f}));')
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["vk_prefilter_stats"]) == C.sizeof(vsa.PrefilterStats) == 56
    for f in names:
        assert int(got[f"vk_prefilter_stats.{f}"]) == getattr(vsa.PrefilterStats, f).offset, f


def test_the_pinned_struct_sizes_are_unchanged(vsa):
    lib = vsa.lib()
    assert lib.vk_abi_struct_size(0) == 144 and lib.vk_abi_struct_size(1) == 440 + 16 * 8


def test_argument_errors_need_no_device(vsa):
    """every argument error comes back before the index is used: the handle here is a block of zeros with no index behind it"""
    lib = vsa.lib()
    fn = lib.vk_index_search_labels_batch
    fake = C.create_string_buffer(256)
    ix = C.cast(fake, C.c_void_p)
    Q = np.zeros((2, 4), np.float32)
    lab = np.arange(6, dtype=np.uint64)
    od, ol, on = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.uint64), np.zeros(2, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ok_lb = np.array([0, 2, 6], np.uint64)
    INV = vsa.VK_ERR_INVALID
    assert fn(None, p(Q), 2, 3, p(lab), p(ok_lb), 6, p(od), p(ol), p(on)) == INV            # a NULL index
    assert fn(None, p(Q), 2, 3, p(lab), None, 6, p(od), p(ol), p(on)) == INV
    assert fn(ix, p(Q), 2, 3, p(lab), None, 6, None, p(ol), p(on)) == INV                  # NULL outputs
    assert fn(ix, p(Q), 2, 3, p(lab), None, 6, p(od), None, p(on)) == INV
    assert fn(ix, p(Q), 2, 3, p(lab), None, 6, p(od), p(ol), None) == INV
    assert fn(ix, None, 2, 3, p(lab), None, 6, p(od), p(ol), p(on)) == INV                 # nq > 0 with NULL queries
    assert fn(ix, p(Q), 2, 3, None, None, 6, p(od), p(ol), p(on)) == INV                   # NULL labels, n_labels != 0
    for bad in ([0, 4, 3], [3, 2, 6], [0, 2, 5], [0, 2, 7], [1, 7, 6]):                    # not ascending / not ending at n_labels
        lb = np.array(bad, np.uint64)
        assert fn(ix, p(Q), 2, 3, p(lab), p(lb), 6, p(od), p(ol), p(on)) == INV, bad
    assert b"list_begin" in lib.vk_last_error()
    s = vsa.PrefilterStats()
    s.struct_size = C.sizeof(vsa.PrefilterStats)
    assert lib.vk_index_prefilter_stats(None, C.byref(s)) == INV
    assert lib.vk_index_prefilter_stats(ix, C.byref(s)) == INV      # (no index behind the handle)
    assert lib.vk_index_prefilter_stats(ix, None) == INV
    s.struct_size = 8
    assert lib.vk_index_prefilter_stats(ix, C.byref(s)) == INV
    assert b"struct_size" in lib.vk_last_error()


def test_the_facade_member_compiles(vsa, tmp_path):
    """include/vk_algo.h: searchLabelsBatch beside searchLabels, built with a plain host compiler against libvkindex.so"""
    src = tmp_path / "algo_batch.cc"
    src.write_text('#include "vk_algo.h"\n#include <type_traits>\n'
                   'template <class A> auto probe(const A &a, const float *q, const uint64_t *l) -> decltype(a.searchLabelsBatch(q, 2, 3, l, nullptr, 4)) '
                   '{ return a.searchLabelsBatch(q, 2, 3, l, nullptr, 4); }\n'
                   'int main() { return 0; }\n')
    text = (ROOT / "include" / "vk_algo.h").read_text()
    assert "searchLabelsBatch" in text and "vk_index_search_labels_batch(ix_" in text
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)])
