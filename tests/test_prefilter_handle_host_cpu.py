"""The host half of the exact kNN from a filter handle (csrc/prefilter_handle_host.hpp) on the CPU (-m "not gpu").  The header
makes no HIP call, so tests/helpers/san_prefilter_handle_main.cc -- a stand-alone program -- drives it under
-fsanitize=address,undefined: run splitting against a plain scan, and -- over ascending label lists spread over 1 to 8 shards,
with ties everywhere -- the union of the shards' hand-backs (a plain model of the select kernel per shard) finished by the heap
rule, against the heap rule over the whole list and against the k smallest by (distance, label); the fallback marks are
counted.  Any mismatch or sanitizer report fails the test.

The second program, tests/helpers/san_prefilter_handle_index_main.cc, links the REAL Index::search_filter_exact_batch and
filter_read_labels (csrc/prefilter_handle.cc), Index::search_labels_batch (csrc/prefilter_batch.cc), index_common.cc and
filter_set.cc against the virtual HIP layer (tests/helpers/hip_virtual.cc) with host models of the filter kernels and of the
expansion, and a fake index whose device stage marks none, all or some of a run's queries: the loop over runs, the download of
a run's list, the in-place and the gathered fallback, the scatter back, the padding and the counters, against the heap rule.
(The build lanes and the bitmap pool of filter_set.cc are never freed by design: no leak report, as in
tests/test_filter_delta_abi.py.)"""
import os
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"
HELP = ROOT / "tests" / "helpers"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def test_union_and_finish_equal_the_heap_over_the_whole_list(tmp_path):
    exe = tmp_path / "prefilter_handle_asan"
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", str(CSRC), str(HELP / "san_prefilter_handle_main.cc"), "-o", str(exe)])
    p = subprocess.run([str(exe), "6", "3000"], env={**os.environ, **ENV}, capture_output=True, text=True, timeout=600)
    report = p.stdout[-2000:] + p.stderr[-6000:]
    assert p.returncode == 0 and "worlds=3000" in p.stdout and "bad=0" in p.stdout, report
    assert "fell=0 " not in p.stdout, report      # the fallback mark was exercised
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, report


def test_the_real_host_half_over_the_virtual_hip_layer(tmp_path):
    exe = tmp_path / "prefilter_handle_index_asan"
    sources = [HELP / "san_prefilter_handle_index_main.cc", HELP / "hip_virtual.cc", CSRC / "prefilter_handle.cc", CSRC / "prefilter_batch.cc",
               CSRC / "index_common.cc", CSRC / "filter_set.cc"]
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I", str(CSRC), "-I", str(ROOT / "include"), "-I", str(HELP), "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", *[str(s) for s in sources], "-lpthread", "-ldl", "-o", str(exe)])
    env = {**os.environ, "ASAN_OPTIONS": "halt_on_error=1:detect_leaks=0", "UBSAN_OPTIONS": ENV["UBSAN_OPTIONS"]}
    p = subprocess.run([str(exe), "300"], env=env, capture_output=True, text=True, timeout=600)
    report = p.stdout[-2000:] + p.stderr[-6000:]
    assert p.returncode == 0 and "rounds=300" in p.stdout and p.stdout.strip().endswith("bad=0"), report
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr and "VIOLATION" not in p.stderr, report
    m = re.search(r"fell=(\d+) downloaded=(\d+) modes=(\d+)/(\d+)/(\d+) stage_calls=(\d+) list_batches=(\d+)", p.stdout)
    assert m and all(int(x) > 0 for x in m.groups()), report      # marks on none, all and some of a run; the list path taken
