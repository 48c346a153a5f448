"""Option prefilter-shared-mfma without a GPU: the options table row (ships 0), the header's struct and function, the ctypes
mirror against what gcc makes of the header, and the truth table of the decision function the drivers and the launcher share
(prefilter_takes_mfma, csrc/prefilter_host.hpp) from a stand-alone host program."""
import ctypes as C
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "valkey-search_amd" / "csrc"


def run_program(tmp_path, name, source, compiler, flags):
    (tmp_path / name).write_text(source)
    subprocess.check_call([compiler, *flags, str(tmp_path / name), "-o", str(tmp_path / "prog")])
    return subprocess.check_output([str(tmp_path / "prog")], text=True)


def test_the_option_ships_off_and_the_header_declares_the_counters():
    assert '{"prefilter-shared-mfma", nullptr, 0, 0, 1},' in (CSRC / "options.hpp").read_text()
    header = (ROOT / "include" / "vk_index.h").read_text()
    assert "} vk_prefilter_mfma_stats;" in header
    assert "int vk_index_prefilter_mfma_stats(vk_index *ix, vk_prefilter_mfma_stats *out);" in header


def test_the_ctypes_mirror_is_the_headers_struct(tmp_path):
    import _pkg
    S = _pkg.vsa.PrefilterMfmaStats
    names = [f[0] for f in S._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "vk_index.h"\nint main(void) {\n  printf("%zu", sizeof(vk_prefilter_mfma_stats));\n'
    src += "".join(f'  printf(" %zu", offsetof(vk_prefilter_mfma_stats, {n}));\n' for n in names) + "  return 0;\n}\n"
    got = [int(v) for v in run_program(tmp_path, "layout.c", src, "gcc", ["-I", str(ROOT / "include")]).split()]
    assert got == [C.sizeof(S)] + [getattr(S, n).offset for n in names] == [40, 0, 8, 16, 24, 32]


def test_the_decision_function(tmp_path):
    src = '#include <stdio.h>\n#include "prefilter_host.hpp"\nint main() {\n  using namespace vk;\n'
    #        wanted shared l2  stride nq   taken
    table = [(0, 1, 0, 768, 32, 0),      # the option is off
             (1, 0, 0, 768, 32, 0),      # per-query (CSR) lists
             (1, 1, 1, 768, 32, 0),      # L2 is not a product of the inputs
             (1, 1, 0, 768, 4, 0),       # below kGemmMinQueries
             (1, 1, 0, 768, 5, 1),
             (1, 1, 0, 64, 5, 1), (1, 1, 0, 832, 5, 1), (1, 1, 0, 1664, 70000, 1),
             (1, 1, 0, 1728, 32, 0),     # no room for 16 queries beside the rings
             (1, 1, 0, 96, 32, 0), (1, 1, 0, 0, 32, 0)]   # not whole stage pairs
    for row in table:
        src += '  printf("%d ", (int)prefilter_takes_mfma({}, {}, {}, {}, {}));\n'.format(*("true" if v else "false" for v in row[:3]), *row[3:5])
    src += '  printf("%u %u %u %u\\n", prefilter_mfma_tile_q(832), prefilter_mfma_tile_q(896), prefilter_mfma_tile_q(1088), prefilter_mfma_tile_q(1152));\n'
    src += "  PrefilterMfmaCount c;\n"
    src += "  unsigned a = prefilter_mfma_decide(true, &c, true, false, 768, 37, 1000), b = prefilter_mfma_decide(true, &c, true, false, 768, 4, 9);\n"
    src += "  unsigned d = prefilter_mfma_decide(true, &c, false, false, 768, 37, 9), e = prefilter_mfma_decide(false, &c, true, false, 768, 37, 9);\n"
    src += '  printf("%u %u %u %u %llu %llu %llu %llu\\n", a, b, d, e, (unsigned long long)c.launches, (unsigned long long)c.queries,\n'
    src += "         (unsigned long long)c.entries, (unsigned long long)c.declined);\n  return 0;\n}\n"
    out = run_program(tmp_path, "decide.cc", src, "g++", ["-std=c++17", "-fsanitize=address,undefined", "-I", str(CSRC)]).splitlines()
    assert [int(v) for v in out[0].split()] == [r[5] for r in table] + [32, 24, 24, 16]
    assert out[1].split() == ["1", "0", "0", "0", "1", "37", "1000", "1"]
