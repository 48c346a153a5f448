"""The CPU side of tests/test_flat_select_kernels_gpu.py: the selection model it compares the kernels with, and a census of the
kernel paths its inputs reach (tests/helpers/flat_select_cases.py restates the branch conditions of csrc/flat_scan.hip)."""
import struct
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import flat_select_cases as FS  # noqa: E402


def test_selection_model_agrees_with_sorted():
    """select_model == Python's sorted on (float, label) -- float compare, so -0 == +0 -- over the real entries"""
    rng = np.random.default_rng(20)
    n_cases = 0
    for total in (1, 2, 3, 7, 16, 17, 63, 64, 65, 300):
        for k in (1, 3, 10, 16, 64):
            for cls in FS.VALUE_CLASSES:
                d, lab = FS.merge_values(cls, total, k, rng)
                real = [i for i in range(total) if int(lab[i]) != FS.NO_LABEL]
                want = sorted(real, key=lambda i: (float(d[i]), int(lab[i])))[:k]
                got = FS.select_model(d, lab, k).tolist()
                assert got == want, (cls, total, k)
                n_cases += 1
    assert n_cases >= 300
    # the key the model orders by: monotone in the float, the two zeros equal
    v = np.array([-np.inf, -3.0, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    key = FS.order_key(v).tolist()
    assert key == sorted(key) and key[3] == key[4] and len(set(key)) == 7
    assert struct.unpack("<I", struct.pack("<f", -0.0))[0] == 0x80000000


def test_tie_classes_have_ties_at_the_kth_place():
    rng = np.random.default_rng(21)
    for total, k in ((65, 10), (4096, 64), (257, 16)):
        for cls in ("equal", "tie_straddle", "zeros", "inf"):
            d, lab = FS.merge_values(cls, total, k, rng)
            o = FS.select_model(d, lab, total)
            key = FS.order_key(d[o])
            assert key[k - 1] == key[k], (cls, total, k)                 # the k-th and the (k+1)-th share a value: labels decide
        d, lab = FS.merge_values("equal", total, k, rng)
        bits = {(int(l) >> 63, (int(l) >> 32) & 1, (int(l) >> 31) & 1) for l in lab.tolist()}
        assert len(bits) == 8 or total < 8


def test_merge_select_path_census():
    """every path of merge_select_kernel the GPU test means to reach is reached by its inputs"""
    seen, few, survivors = set(), 0, set()
    by_placement = {}
    for total in FS.SELECT_TOTALS:
        for k in FS.SELECT_KS:
            for name, d, lab in FS.merge_queries(total, k):
                path, f, s = FS.select_path(d, lab, k)
                seen.add(path)
                few += int(f and path != "empty")
                survivors.add(s)
                by_placement.setdefault(name, set()).add(path)
    assert {"fast", "general", "empty"} <= seen
    assert few > 0, "no input whose sample has fewer than k real entries (U = 0xFFFFFFFF)"
    assert 256 in survivors and 257 in survivors
    assert by_placement["sample_smallest"] == {"fast"}
    assert "general" in by_placement["sample_largest"] and "general" in by_placement["survivors_257"]
    assert by_placement["survivors_256"] == {"fast"} and by_placement["survivors_257"] == {"general"}
    assert "general" in by_placement["sample_few_real"]
    for cls in ("equal", "tie_straddle", "zeros", "inf"):               # the label descent at a tied k-th key, on both paths
        assert {"fast", "general"} <= by_placement[cls], cls


def test_rerank_path_census():
    """solo in registers, solo walking, 8-block and the flush inside a walk are all among the GPU test's lists"""
    paths = set()
    for k in (1, 10, 64):
        for n in FS.rerank_counts(k):
            paths.add(FS.rerank_path(n, 4096, True))
    assert paths == {("registers", False), ("blocks", False)}
    small = {n: FS.rerank_path(n, FS.RERANK_SMALL_CAP, True) for n in FS.RERANK_SMALL_CAP_COUNTS}
    assert small[255][0] == small[256][0] == "registers"
    assert small[257][0] == small[1000][0] == "walking"
    assert small[FS.RERANK_SMALL_CAP + FS.SPILL_CHUNK + 1][0] == "blocks"
    assert FS.rerank_path(2048, 4096, True)[0] == "registers" and FS.rerank_path(2049, 4096, True)[0] == "blocks"
    assert FS.rerank_path(FS.RERANK_LONG, FS.RERANK_SMALL_CAP, False) == ("blocks", True)
    assert FS.rerank_path(2048, FS.RERANK_SMALL_CAP, False) == ("walking", False)   # 512 kept per wave: the slots just hold them
