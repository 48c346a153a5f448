"""The host half of the one-pass FLAT search for k > 1024 (csrc/flat_large_k_host.hpp) and its ABI, on the CPU (-m "not gpu").

The header makes no HIP call, so tests/helpers/san_flat_large_k_main.cc -- a stand-alone program with its own main -- drives it
under -fsanitize=address,undefined: the chunk plan over random (nq, count, k, budget), and the finish rule over a few thousand
random hand-backs with ties, +0 / -0 and short lists against std::partial_sort over the full list.  Any mismatch or sanitizer
report fails the test.

The ABI: vk_index_large_k_stats is declared and exported, the Python binding's mirror matches what a C compiler makes of
include/vk_index.h (size and the offset of every field), the structs that must not grow have not grown, the facade's
pass-through compiles, the argument checks that need no device answer VK_ERR_INVALID, and the two options are in the table
with the documented defaults."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"
HELP = ROOT / "tests" / "helpers"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
FIELDS = ["struct_size", "queries", "one_pass_queries", "fallback_queries", "chunks", "emitted_entries", "row_passes"]


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    v = _pkg.vsa
    if not v.LIB_PATH.exists():
        v.build()
    return v


def test_plan_and_finish_rule_under_sanitizers(tmp_path):
    exe = tmp_path / "flat_large_k_asan"
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", str(CSRC), str(HELP / "san_flat_large_k_main.cc"), "-o", str(exe)])
    p = subprocess.run([str(exe), "7", "2000", "4000"], env={**os.environ, **ENV}, capture_output=True, text=True, timeout=600)
    report = p.stdout[-2000:] + p.stderr[-6000:]
    assert p.returncode == 0 and "plans=2000 worlds=4000" in p.stdout and p.stdout.strip().endswith("bad=0"), report
    m = re.search(r"short=(\d+) zeros=(\d+)", p.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 1000, report       # short lists and both zeros were exercised
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, report


def test_the_symbol_is_declared_and_exported(vsa):
    text = (ROOT / "include" / "vk_index.h").read_text()
    lib = C.CDLL(str(vsa.LIB_PATH))
    assert "int vk_index_large_k_stats(" in text and hasattr(lib, "vk_index_large_k_stats")
    vsa.lib()      # (the binding resolves it too)
    assert hasattr(vsa.Index, "large_k_stats")


def test_stats_mirror_matches_the_header(vsa, tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vk_index.h"', 'int main(void){']
    for cname in ("vk_flat_large_k_stats", "vk_index_stats", "vk_index_params"):
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
    for fname in FIELDS:
        lines.append(f'printf("f.{fname} %zu\\n", offsetof(vk_flat_large_k_stats, {fname}));')
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [f for f, _ in vsa.FlatLargeKStats._fields_] == FIELDS
    assert int(got["vk_flat_large_k_stats"]) == C.sizeof(vsa.FlatLargeKStats) == 56
    for fname in FIELDS:
        assert int(got[f"f.{fname}"]) == getattr(vsa.FlatLargeKStats, fname).offset, fname
    assert int(got["vk_index_stats"]) == 568 and int(got["vk_index_params"]) == 144      # what must keep its size


def test_argument_validation_needs_no_device(vsa):
    lib = vsa.lib()
    s = vsa.FlatLargeKStats()
    s.struct_size = C.sizeof(vsa.FlatLargeKStats)
    assert lib.vk_index_large_k_stats(None, C.byref(s)) == vsa.VK_ERR_INVALID
    s.struct_size = 8
    assert lib.vk_index_large_k_stats(None, C.byref(s)) == vsa.VK_ERR_INVALID and b"struct_size" in lib.vk_last_error()
    assert lib.vk_index_large_k_stats(None, None) == vsa.VK_ERR_INVALID


def test_the_options_are_in_the_table():
    text = (CSRC / "options.hpp").read_text()
    assert re.search(r'\{"flat-large-k", nullptr, 0, 0, 1\}', text)                                  # ships 0
    assert re.search(r'\{"flat-large-k-bytes", nullptr, \(uint64_t\)1 << 30, 0, kMax\}', text)      # 1 GiB, the neighbours' range


def test_the_facade_method_compiles(tmp_path):
    src = tmp_path / "use.cc"
    src.write_text('#include "vk_algo.h"\n'
                   'template <class A> vk_flat_large_k_stats use(A &a) { return a.largeKStats(); }\n'
                   'int main() { return 0; }\n')
    assert "largeKStats" in (ROOT / "include" / "vk_algo.h").read_text()
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)])
