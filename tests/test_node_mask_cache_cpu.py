"""The bookkeeping of the HNSW node masks (csrc/node_mask_cache.hpp) on the CPU (-m "not gpu"): the header makes no HIP call, so
tests/helpers/san_node_mask_main.cc drives it with host memory under -fsanitize={address,undefined} and -fsanitize=thread --
least-recently-used order, epoch invalidation, the byte budget, the fallback decision (no room = nothing evicted, nothing
built), holders that outlive an eviction, and get / reserve / put / drop_stale / clear from several threads.  Any sanitizer
report fails the test."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"
HELP = ROOT / "tests" / "helpers"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
SAN = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-fsanitize=thread"]}
ENV = {"ASAN_OPTIONS": "halt_on_error=1:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
       "TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1"}


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_node_mask_cache_under_sanitizers(tmp_path, san):
    exe = tmp_path / f"node_mask_{san}"
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", *SAN[san], "-I", str(CSRC),
                           str(HELP / "san_node_mask_main.cc"), "-lpthread", "-o", str(exe)])
    p = subprocess.run([str(exe), "6", "4000" if san == "asan" else "2000"], env={**os.environ, **ENV}, capture_output=True, text=True,
                       timeout=600)
    report = p.stdout[-2000:] + p.stderr[-6000:]
    assert p.returncode == 0 and "bad=0" in p.stdout, report
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, report


def test_the_header_makes_no_hip_call():
    text = (CSRC / "node_mask_cache.hpp").read_text()
    assert "#include <hip" not in text and "hipMalloc" not in text and "hipFree" not in text


def test_the_options_exist_with_their_defaults():
    """hnsw-node-mask (0 / 1) and hnsw-node-mask-bytes (1 GiB, like filter-cache-bytes) are in the option table"""
    text = (CSRC / "options.hpp").read_text()
    assert '{"hnsw-node-mask", "VK_HNSW_NODE_MASK", 0, 0, 1}' in text      # (off until the probe's gate says otherwise)
    assert '{"hnsw-node-mask-bytes", nullptr, (uint64_t)1 << 30, 0, kMax}' in text
