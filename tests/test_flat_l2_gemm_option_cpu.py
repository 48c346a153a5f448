"""Option flat-l2-gemm without a GPU: the options table row (ships 0), the header's struct and function, the vk_algo.h accessor, the
ctypes mirror against what gcc makes of the header, the argument checks of vk_index_l2_gemm_stats, and the truth table of the
decision function FlatIndex::scan and the launcher share (csrc/flat_l2_gemm_host.hpp) from a stand-alone host program under
ASAN / UBSAN."""
import ctypes as C
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"


def run_program(tmp_path, name, source, compiler, flags):
    (tmp_path / name).write_text(source)
    subprocess.check_call([compiler, *flags, str(tmp_path / name), "-o", str(tmp_path / "prog")])
    return subprocess.check_output([str(tmp_path / "prog")], text=True)


def test_the_option_ships_off_and_the_interface_is_the_headers(tmp_path):
    import _pkg
    assert '{"flat-l2-gemm", nullptr, 0, 0, 1},' in (CSRC / "options.hpp").read_text()
    header = (ROOT / "include" / "vk_index.h").read_text()
    assert "} vk_flat_l2_gemm_stats;" in header
    assert "int vk_index_l2_gemm_stats(vk_index *ix, vk_flat_l2_gemm_stats *out);" in header
    (tmp_path / "algo.cc").write_text('#include "vk_algo.h"\nauto p = &vkalgo::Algo<float>::l2GemmStats;\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", str(ROOT / "include"), str(tmp_path / "algo.cc")])
    S = _pkg.vsa.FlatL2GemmStats
    names = [f[0] for f in S._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "vk_index.h"\nint main(void) {\n  printf("%zu", sizeof(vk_flat_l2_gemm_stats));\n'
    src += "".join(f'  printf(" %zu", offsetof(vk_flat_l2_gemm_stats, {n}));\n' for n in names) + "  return 0;\n}\n"
    got = [int(v) for v in run_program(tmp_path, "layout.c", src, "gcc", ["-I", str(ROOT / "include")]).split()]
    assert names == ["struct_size", "launches", "queries", "rows", "evaluated", "declined"]
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n in names] == [48, 0, 8, 16, 24, 32, 40]
    # the checks that need no device: NULL out, a wrong struct_size, NULL ix
    f, s = _pkg.vsa.lib().vk_index_l2_gemm_stats, S()
    assert f(None, None) == _pkg.vsa.VK_ERR_INVALID
    for size in (C.sizeof(S) - 8, C.sizeof(S)):
        s.struct_size = size
        assert f(None, C.byref(s)) == _pkg.vsa.VK_ERR_INVALID


def test_the_decision_function(tmp_path):
    src = '#include <stdio.h>\n#include "flat_l2_gemm_host.hpp"\nint main() {\n  using namespace vk;\n'
    #        wanted l2 paged cancelled force nq stride k  taken
    table = [(0, 1, 0, 0, 0, 33, 768, 10, 0),        # the option is off
             (1, 0, 0, 0, 0, 33, 768, 10, 0),        # IP / COSINE: K4's
             (1, 1, 1, 0, 0, 33, 768, 10, 0),        # a pass of the k > 1024 pager
             (1, 1, 0, 1, 0, 33, 768, 10, 0),        # cancelled at entry
             (1, 1, 0, 0, 1, 33, 768, 10, 0),        # flat-force-scan
             (1, 1, 0, 0, 0, 4, 768, 10, 0),         # below kGemmMinQueries
             (1, 1, 0, 0, 0, 5, 768, 10, 1), (1, 1, 0, 0, 0, 65535, 64, 1, 1), (1, 1, 0, 0, 0, 33, 1856, 256, 1),
             (1, 1, 0, 0, 0, 33, 1920, 10, 0),       # no room for 16 queries beside the rest
             (1, 1, 0, 0, 0, 33, 96, 10, 0), (1, 1, 0, 0, 0, 33, 0, 10, 0),   # not whole pairs of stages
             (1, 1, 0, 0, 0, 33, 768, 0, 0), (1, 1, 0, 0, 0, 33, 768, 257, 0)]
    for r in table:
        b = ", ".join("true" if v else "false" for v in r[1:5]) + ", {}, {}, {}".format(*r[5:8])
        src += '  printf("%d ", (int)l2_gemm_takes({}, L2GemmBatch{{{}}}));\n'.format("true" if r[0] else "false", b)
    # queries per block by stride: 64 while the Q tile fits, then 32 / 24 / 16, then nothing
    strides = [(64, 64), (448, 64), (512, 32), (896, 32), (960, 24), (1216, 24), (1280, 16), (1856, 16), (1920, 0)]
    src += '  printf("\\n");\n' + "".join(f'  printf("%u ", l2_gemm_tile_q({s}));\n' for s, _ in strides)
    src += "  L2GemmCount c;\n  const L2GemmBatch ok{true, false, false, false, 37, 768, 10}, few{true, false, false, false, 4, 768, 10}, ip{false, false, false, false, 37, 768, 10};\n"
    src += "  int a = l2_gemm_decide(true, &c, ok, 1000), b = l2_gemm_decide(true, &c, few, 9), d = l2_gemm_decide(true, &c, ip, 9), e = l2_gemm_decide(false, &c, ok, 9);\n"
    src += '  printf("\\n%d %d %d %d %llu %llu %llu %llu\\n", a, b, d, e, (unsigned long long)c.launches, (unsigned long long)c.queries,\n'
    src += "         (unsigned long long)c.rows, (unsigned long long)c.declined);\n  return 0;\n}\n"
    out = run_program(tmp_path, "decide.cc", src, "g++", ["-std=c++17", "-fsanitize=address,undefined", "-I", str(CSRC)]).splitlines()
    assert [int(v) for v in out[0].split()] == [r[8] for r in table]
    assert [int(v) for v in out[1].split()] == [t for _, t in strides]
    assert out[2].split() == ["1", "0", "0", "0", "1", "37", "1000", "1"]   # an IP batch is not "declined": nothing wanted the path
