"""The host half of the batched pre-filter search (csrc/prefilter_host.hpp) on the CPU (-m "not gpu").  The header makes no
HIP call, so tests/helpers/san_prefilter_select_main.cc -- a stand-alone program -- drives it under
-fsanitize=address,undefined: a plain model of what the select kernel emits (everything at or below the k-th smallest
distance, in list order, up to the cap), then the reference's heap rule over that hand-back, against the heap rule over the
whole list; 20 000 random lists of 0 to 3 000 keys, k in {1, 2, 10, 64, 1000}, 3 to 50 distinct distances (ties everywhere),
duplicate labels, +-0, all-equal lists, NaNs, unknown keys, and the union of 1 to 8 shards.  Any mismatch or sanitizer report
fails the test."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"
HELP = ROOT / "tests" / "helpers"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def test_select_then_heap_equals_the_heap_over_the_whole_list(tmp_path):
    exe = tmp_path / "prefilter_select_asan"
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", str(CSRC), str(HELP / "san_prefilter_select_main.cc"), "-o", str(exe)])
    p = subprocess.run([str(exe), "6", "20000"], env={**os.environ, **ENV}, capture_output=True, text=True, timeout=600)
    report = p.stdout[-2000:] + p.stderr[-6000:]
    assert p.returncode == 0 and "lists=20000" in p.stdout and "bad=0" in p.stdout, report
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, report


def test_the_header_makes_no_hip_call():
    text = (CSRC / "prefilter_host.hpp").read_text()
    assert "#include <hip" not in text and "hipMalloc" not in text and "hipMemcpy" not in text and "hipStream" not in text


def test_the_single_call_and_the_batch_share_one_heap_rule():
    """prefilter_heap_select (the single call's host half) is the header's rule, not a second copy of it"""
    text = (CSRC / "flat_index.cc").read_text()
    body = text[text.index("void prefilter_heap_select("):]
    body = body[:body.index("\n}\n")]
    assert "prefilter_heap_rule(dist, labels, n, k, out_dist, out_label, out_n)" in body and "priority_queue" not in body
