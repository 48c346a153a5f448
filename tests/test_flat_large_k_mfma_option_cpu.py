"""Option flat-large-k-mfma without a GPU: the options table row (ships 0), the header's struct and function, the vk_algo.h
accessor, the ctypes mirror against what gcc makes of the header, the argument checks of vk_index_large_k_mfma_stats, and the truth
table of the decision function FlatIndex::search_large_k and the launcher share (large_k_takes_mfma, csrc/flat_large_k_host.hpp)
from a stand-alone host program under ASAN / UBSAN."""
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
    assert '{"flat-large-k-mfma", nullptr, 0, 0, 1},' in (CSRC / "options.hpp").read_text()
    header = (ROOT / "include" / "vk_index.h").read_text()
    assert "} vk_flat_large_k_mfma_stats;" in header
    assert "int vk_index_large_k_mfma_stats(vk_index *ix, vk_flat_large_k_mfma_stats *out);" in header
    (tmp_path / "algo.cc").write_text('#include "vk_algo.h"\nauto p = &vkalgo::Algo<float>::largeKMfmaStats;\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", str(ROOT / "include"), str(tmp_path / "algo.cc")])
    S = _pkg.vsa.FlatLargeKMfmaStats
    names = [f[0] for f in S._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "vk_index.h"\nint main(void) {\n  printf("%zu", sizeof(vk_flat_large_k_mfma_stats));\n'
    src += "".join(f'  printf(" %zu", offsetof(vk_flat_large_k_mfma_stats, {n}));\n' for n in names) + "  return 0;\n}\n"
    got = [int(v) for v in run_program(tmp_path, "layout.c", src, "gcc", ["-I", str(ROOT / "include")]).split()]
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n in names] == [40, 0, 8, 16, 24, 32]
    # the checks that need no device: NULL out, a wrong struct_size, NULL ix
    f, s = _pkg.vsa.lib().vk_index_large_k_mfma_stats, S()
    assert f(None, None) == _pkg.vsa.VK_ERR_INVALID
    for size in (C.sizeof(S) - 8, C.sizeof(S)):
        s.struct_size = size
        assert f(None, C.byref(s)) == _pkg.vsa.VK_ERR_INVALID


def test_the_decision_function(tmp_path):
    src = '#include <stdio.h>\n#include "flat_large_k_host.hpp"\nint main() {\n  using namespace vk;\n'
    #        wanted l2 stride qc  taken
    table = [(0, 0, 768, 32, 0),      # the option is off
             (1, 1, 768, 32, 0),      # L2 is not a product of the inputs
             (1, 0, 768, 4, 0),       # below kGemmMinQueries
             (1, 0, 768, 5, 1), (1, 0, 64, 5, 1), (1, 0, 832, 5, 1), (1, 0, 1664, 65535, 1),
             (1, 0, 1728, 32, 0),     # no room for 16 queries beside the rings
             (1, 0, 96, 32, 0), (1, 0, 0, 32, 0)]   # not whole stage pairs
    for row in table:
        src += '  printf("%d ", (int)large_k_takes_mfma({}, {}, {}, {}));\n'.format(*("true" if v else "false" for v in row[:2]), *row[2:4])
    src += "  LargeKMfmaCount c;\n"
    src += "  int a = large_k_mfma_decide(true, &c, false, 768, 37, 1000), b = large_k_mfma_decide(true, &c, false, 768, 4, 9);\n"
    src += "  int d = large_k_mfma_decide(true, &c, true, 768, 37, 9), e = large_k_mfma_decide(false, &c, false, 768, 37, 9);\n"
    src += '  printf("\\n%d %d %d %d %llu %llu %llu %llu\\n", a, b, d, e, (unsigned long long)c.launches, (unsigned long long)c.queries,\n'
    src += "         (unsigned long long)c.rows, (unsigned long long)c.declined);\n  return 0;\n}\n"
    out = run_program(tmp_path, "decide.cc", src, "g++", ["-std=c++17", "-fsanitize=address,undefined", "-I", str(CSRC)]).splitlines()
    assert [int(v) for v in out[0].split()] == [r[4] for r in table]
    assert out[1].split() == ["1", "0", "0", "0", "1", "37", "1000", "2"]
