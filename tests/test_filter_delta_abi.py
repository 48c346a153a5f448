"""CPU-side checks of vk_filter_apply_delta[_batch] (include/vk_index.h): declared, exported, mirrored by the binding with the
layout a C compiler gives the struct, no change to the pinned struct sizes, refused without an index -- and the adaptor's
maintained predicates (include/vk_vector_adaptor.h) compile against the mocked interface as that mock is.  The host code
of FilterSet::apply_delta_batch (csrc/filter_delta.cc) runs under ASAN+UBSAN and TSAN over the virtual HIP runtime."""
import ctypes as C
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"
HELP = ROOT / "tests" / "helpers"


@pytest.fixture(scope="module")
def vsa():
    import _pkg
    v = _pkg.vsa
    if not v.LIB_PATH.exists():
        v.build()
    return v


def test_header_declares_the_delta_entry_points():
    text = (ROOT / "include" / "vk_index.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+vk_filter_apply_delta\s*\(\s*vk_index\s*\*\s*ix\s*,\s*const\s+vk_filter_delta\s*\*\s*item\s*,\s*vk_filter\s*\*\*\s*out\s*\)\s*;", text)
    assert re.search(r"int\s+vk_filter_apply_delta_batch\s*\(\s*vk_index\s*\*\s*ix\s*,\s*const\s+vk_filter_delta\s*\*\s*items\s*,\s*uint64_t\s+n\s*,"
                     r"\s*vk_filter\s*\*\*\s*out\s*\)\s*;", text)
    assert re.search(r"typedef\s+struct\s+vk_filter_delta\s*\{[^}]*\}\s*vk_filter_delta\s*;", text)


def test_library_exports_the_delta_entry_points(vsa):
    lib = C.CDLL(str(vsa.LIB_PATH))
    assert hasattr(lib, "vk_filter_apply_delta") and hasattr(lib, "vk_filter_apply_delta_batch")


def test_delta_struct_layout_matches_header_and_pinned_sizes_stay(vsa, tmp_path):
    """vsa.FilterDelta against what gcc makes of vk_filter_delta: size and the offset of every field; vk_index_params /
    vk_index_stats keep the sizes tests/test_abi_symbols.py pins (the feature adds no field to either)."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vk_index.h"', 'int main(void){',
             'printf("vk_filter_delta %zu\\n", sizeof(vk_filter_delta));',
             'printf("vk_index_params %zu\\n", sizeof(vk_index_params));',
             'printf("vk_index_stats %zu\\n", sizeof(vk_index_stats));']
    for fname, _ in vsa.FilterDelta._fields_:
        lines.append(f'printf("vk_filter_delta.{fname} %zu\\n", offsetof(vk_filter_delta, {fname}));')
    lines.append('return 0;}')
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["vk_filter_delta"]) == C.sizeof(vsa.FilterDelta) == 48
    assert [f for f, _ in vsa.FilterDelta._fields_] == ["base", "nbits", "clear_labels", "n_clear", "set_labels", "n_set"]
    for fname, _ in vsa.FilterDelta._fields_:
        assert int(got[f"vk_filter_delta.{fname}"]) == getattr(vsa.FilterDelta, fname).offset, fname
    assert int(got["vk_index_params"]) == C.sizeof(vsa.Params) == 144
    assert int(got["vk_index_stats"]) == C.sizeof(vsa.Stats) == 440 + 16 * 8
    lib = vsa.lib()
    assert lib.vk_abi_struct_size(0) == 144 and lib.vk_abi_struct_size(1) == 440 + 16 * 8


def test_without_an_index_both_calls_are_refused_before_any_device_work(vsa):
    lib = vsa.lib()
    item = vsa.FilterDelta(None, 64, None, 0, None, 0)
    out = (C.c_void_p * 1)()
    assert lib.vk_filter_apply_delta(None, item, out) == vsa.VK_ERR_INVALID
    assert b"index is NULL" in lib.vk_last_error()
    assert lib.vk_filter_apply_delta_batch(None, item, 1, out) == vsa.VK_ERR_INVALID
    assert lib.vk_filter_apply_delta_batch(None, None, 0, None) == vsa.VK_ERR_INVALID
    assert out[0] is None


def test_maintained_filters_of_the_adaptor_compile_against_the_mocked_interface(vsa, tmp_path):
    """tests/helpers/adaptor_filter_delta_check.cc drives MaintainFilter / ForgetFilter / NoteFilterChange / OnWritePhaseEnd
    (every member template is instantiated) with -Wall -Wextra -Werror against tests/helpers/mock_valkey_search.h."""
    exe = tmp_path / "adaptor_filter_delta_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-Wsuggest-override", "-I", str(ROOT / "include"),
                           "-I", str(HELP), str(HELP / "adaptor_filter_delta_check.cc"), "-o", str(exe),
                           "-L", str(vsa.LIB_PATH.parent), "-lvkindex", "-lpthread", f"-Wl,-rpath,{vsa.LIB_PATH.parent}"])
    assert exe.exists()


CXX = "/opt/rocm/lib/llvm/bin/clang++"
SAN = {"asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tsan": ["-fsanitize=thread"]}


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_apply_delta_host_code_under_sanitizers(tmp_path, san):
    """The real filter_set.cc + filter_delta.cc over the virtual HIP runtime (tests/helpers/hip_virtual.cc: several devices,
    asynchronous streams) with host models of the filter kernels (tests/helpers/san_filter_delta_main.cc): batches from
    several threads on 1 to 3 devices against a host model, error paths included.  Any sanitizer report, any violation
    the runtime model records (memory of another device, a staging block overwritten in flight) fails the test."""
    exe = tmp_path / f"filter_delta_{san}"
    subprocess.check_call([CXX, "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I", str(CSRC), "-I", str(ROOT / "include"), "-I", str(HELP), *SAN[san],
                           str(HELP / "san_filter_delta_main.cc"), str(HELP / "hip_virtual.cc"), str(CSRC / "filter_set.cc"),
                           str(CSRC / "filter_delta.cc"), "-lpthread", "-ldl", "-rdynamic", "-o", str(exe)])
    env = {**os.environ, "ASAN_OPTIONS": "halt_on_error=1:detect_leaks=0", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
           "TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1"}
    p = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=600)
    report = p.stdout[-2000:] + p.stderr[-6000:]
    assert p.returncode == 0 and "bad=0" in p.stdout, report
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr and "VIOLATION" not in p.stderr, report
