"""The pre-filter lane of the dispatcher on the CPU (-m "not gpu"): vk_index_search_labels_submit's host side under the
sanitizers, and its place in the three bindings.

tests/helpers/san_prefilter_submit_main.cc -- a stand-alone program with its own main -- links the real csrc/dispatcher.hpp,
csrc/prefilter_batch.cc and csrc/index_common.cc against the virtual HIP layer (tests/helpers/hip_virtual.cc) and drives the
new lane from several threads: shared and own lists, callbacks and the bulk hook, a shallow queue, an index destroyed with
requests queued.  Built once with -fsanitize=address,undefined and once with -fsanitize=thread; no Python process loads
sanitized code."""
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"
HELP = ROOT / "tests" / "helpers"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
COMMON = ["-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
          "-I", str(CSRC), "-I", str(ROOT / "include"), "-I", str(HELP)]
SAN = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-fsanitize=thread"]}
ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
       "TSAN_OPTIONS": f"halt_on_error=1:second_deadlock_stack=1:suppressions={HELP / 'tsan_suppressions.txt'}"}
SOURCES = [HELP / "san_prefilter_submit_main.cc", HELP / "hip_virtual.cc", CSRC / "prefilter_batch.cc", CSRC / "index_common.cc"]


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_the_prefilter_lane_under_sanitizers(tmp_path, san):
    exe = tmp_path / f"prefilter_submit_{san}"
    subprocess.check_call([CXX, *COMMON, *SAN[san], *[str(s) for s in SOURCES], "-lpthread", "-ldl", "-o", str(exe)])
    p = subprocess.run([str(exe), "1"], env={**os.environ, **ENV}, capture_output=True, text=True, timeout=600)
    report = p.stdout[-2000:] + p.stderr[-6000:]
    assert p.returncode == 0, report
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, report
    assert p.stdout.strip().endswith("bad=0"), report
    busy = [int(m) for m in re.findall(r"busy=(\d+)", p.stdout)]
    shared = [int(m) for m in re.findall(r"shared_batches=(\d+)", p.stdout)]
    assert len(busy) == 5 and busy[2] > 0, report          # the shallow queue did refuse
    assert all(m <= b for m, b in zip([int(m) for m in re.findall(r"max_batch=(\d+)", p.stdout)], (8, 16, 4, 64, 64)))
    assert len(shared) == 5


def test_the_three_bindings_have_the_call():
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "vk_index.h").read_text(), flags=re.S)
    assert re.search(r"^\s*int\s+vk_index_search_labels_submit\s*\(", hdr, flags=re.M)
    assert "vk_index_search_labels_submit(ix_" in (ROOT / "include" / "vk_algo.h").read_text()
    assert "vk_index_search_labels_submit(ix_" in (CSRC / "host" / "vector_index.cc").read_text()
    assert "vsa_search_prefiltered_submit" in (CSRC / "host" / "host_capi.cc").read_text()
    assert "L.vk_index_search_labels_submit.argtypes" in (ROOT / "valkey-search_amd" / "__init__.py").read_text()


def test_the_facade_member_compiles(tmp_path):
    src = tmp_path / "algo_submit.cc"
    src.write_text('#include "vk_algo.h"\n'
                   'template <class A> auto probe(const A &a, const float *q, const uint64_t *l, float *d, uint64_t *o, uint64_t *n, vk_search_done_fn f)\n'
                   '    -> decltype(a.submitLabels(q, 3, l, 4, d, o, n, f, nullptr)) { return a.submitLabels(q, 3, l, 4, d, o, n, f, nullptr); }\n'
                   'int main() { return 0; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), str(src)])
