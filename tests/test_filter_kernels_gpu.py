"""The device filter kernels on their own: csrc/filter_build.hip (set_ids, set_runs, popcount, combine, combine_batch, delta_copy,
delta_apply<set|clear>), csrc/node_mask.hip (launch_node_mask_build) and the two row kernels at the end of csrc/hnsw_search.hip
(launch_scatter_u32, launch_gather_u32), through tests/helpers/filter_build_probe.hip, node_mask_probe.hip and
hnsw_search_probe.hip's row entry -- small libraries that include those translation units, built with the library's flags, so
the product's kernels and launchers run, on buffers the test owns.

Every case runs three times: every buffer a kernel writes is filled with 0x00000000, 0xFFFFFFFF and 0xEEEEEEEE in turn before the
launch, except where the contract says "zeroed by the caller" or "holds the set to extend" -- there the case supplies random
words, also above nbits, in the slack word and behind it.  Every buffer comes back whole and is held, word for word, to the
boolean models of tests/helpers/filter_kernel_cases.py (pinned without a GPU by tests/test_filter_kernels_model_cpu.py, which
also checks that each case crosses the threshold it is named for): the bitmap, what lies above nbits and behind it, the slack
word, every per-block partial sum (exactly where contract and geometry decide them, else their sum and their range), the
entries no block owns, and counts added onto non-zero starts modulo 2^64.  The probes poll their stream with a time limit; a
launch that does not finish, or a HIP error, fails the test and every later test of this file without another launch."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "helpers"
CSRC = ROOT / "valkey-search_amd" / "csrc"
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]      # csrc/Makefile's

sys.path.insert(0, str(HERE))
import filter_kernel_cases as FK  # noqa: E402

FILLS = FK.FILLS
M64 = FK.M64
STOPPED = []          # why nothing more is launched from this file


def build_probe(src, lib, *deps):
    newest = max(p.stat().st_mtime for p in (HERE / src, CSRC / "kernels.hpp", *deps))
    if not (HERE / lib).exists() or (HERE / lib).stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", *FLAGS, "-shared", "-fPIC", "-I", str(CSRC), str(HERE / src),
                               "-o", str(HERE / lib)])
    return C.CDLL(str(HERE / lib))


def ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def u64(a):
    return np.ascontiguousarray(a, np.uint64)


class Probes:
    def __init__(self):
        vp, u32, q, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        fb = build_probe("filter_build_probe.hip", "libfilterbuildprobe.so", HERE / "probe_common.hpp", CSRC / "filter_build.hip", CSRC / "filter_lane.hpp")
        nm = build_probe("node_mask_probe.hip", "libnodemaskprobe.so", HERE / "probe_common.hpp", CSRC / "node_mask.hip")
        hs = build_probe("hnsw_search_probe.hip", "libhnswsearchprobe.so", CSRC / "hnsw_search.hip", CSRC / "device_common.hpp")
        for f in ("fb_probe_set_ids_blocks", "fb_probe_set_runs_blocks", "fb_probe_combine_blocks"):
            getattr(fb, f).argtypes, getattr(fb, f).restype = [q], u32
        fb.fb_probe_partials.restype = fb.fb_probe_pad.restype = nm.nm_probe_pad.restype = u32
        fb.fb_probe_set.argtypes = [u32, i32, vp, q, q, vp, q, vp]
        fb.fb_probe_popcount.argtypes = [u32, vp, q, q, vp]
        fb.fb_probe_combine.argtypes = [u32, vp, vp, q, u32, vp, vp]
        fb.fb_probe_combine_batch.argtypes = [u32, vp, u32, q, vp, u32, vp, vp]
        fb.fb_probe_delta.argtypes = [u32, i32, vp, q, vp, vp, vp, vp, u32, q, vp, q, vp, q, vp, vp]
        nm.nm_probe_run.argtypes = [u32, vp, vp, u32, vp, q, vp, vp, vp, u32, vp, vp]
        hs.hs_probe_rows.argtypes = [u32, i32, vp, vp, u32, u32, u32, vp]
        self.fb, self.nm, self.hs = fb, nm, hs
        assert fb.fb_probe_partials() == FK.PARTIALS and fb.fb_probe_pad() == FK.PAD
        self.nm_pad = nm.nm_probe_pad()

    @staticmethod
    def done(rc, what, allowed=(0,)):
        """a launch that did not finish (2) or a HIP error (a source line): nothing more is launched from this file"""
        if rc not in allowed and rc >= 2:
            STOPPED.append("%s: %s" % (what, "a launch did not finish within the probe's time limit" if rc == 2 else "HIP error seen at source line %d" % rc))
            pytest.fail(STOPPED[-1])
        assert rc != 1, what + " refused its arguments"
        assert rc in allowed, what + ": the launcher's answer"
        return rc


@pytest.fixture(scope="module")
def probes():
    return Probes()


@pytest.fixture(autouse=True)
def nothing_after_a_stop():
    if STOPPED:
        pytest.fail("not run: " + STOPPED[0])


def test_the_mirrored_geometry_is_the_launchers(probes):
    for n in (0, 1, 255, 256, 257, 524_288, 524_289, 600_000, 1 << 26):
        assert probes.fb.fb_probe_set_ids_blocks(n) == FK.set_ids_blocks(n)
        assert probes.fb.fb_probe_combine_blocks(n) == FK.combine_blocks(n)
    for n in (0, 1, 4, 5, 8191, 8192, 8193, 9000, 1 << 24):
        assert probes.fb.fb_probe_set_runs_blocks(n) == FK.set_runs_blocks(n)


def check_partials(got, want_exact, want_sum, blocks, fill, what):
    f64 = FK.fill64(fill)
    assert (got[blocks:] == np.uint64(f64)).all(), what + ": a partial sum no block owns was written"
    if want_exact is not None:
        assert got[:blocks].tolist() == want_exact.tolist(), what + ": per-block partial sums"
    assert int(got[:blocks].astype(object).sum()) == want_sum and int(got[:blocks].max()) <= want_sum, what + ": the partial sums' total"


# ---- set_ids / set_runs -------------------------------------------------------------------------------------------------------
def run_set(probes, fill, runs, case):
    bits = case["bits"].copy()
    data = u64(case["runs"] if runs else case["ids"])
    n = len(data)
    part = np.zeros(FK.PARTIALS, np.uint64)
    rc = probes.fb.fb_probe_set(fill, runs, ptr(bits), bits.size, case["nbits"], ptr(data), n, ptr(part))
    probes.done(rc, "fb_probe_set")
    return bits, part


SET_IDS = FK.set_ids_cases()


@pytest.mark.parametrize("name", sorted(SET_IDS))
def test_set_ids(probes, name):
    case = SET_IDS[name]
    want, added = FK.set_ids_model(case["bits"], case["nbits"], case["ids"])
    blocks = FK.set_ids_blocks(len(case["ids"]))
    exact = FK.set_ids_partials(case["bits"], case["nbits"], case["ids"], blocks)
    assert (exact is not None) or not case.get("exact_partials")
    for fill in FILLS:
        bits, part = run_set(probes, fill, 0, case)
        assert np.array_equal(bits, want), hex(fill)          # the set, the bits above nbits, the slack word and the pad
        check_partials(part, exact, added, blocks, fill, hex(fill))


SET_RUNS = FK.set_runs_cases()


@pytest.mark.parametrize("name", sorted(SET_RUNS))
def test_set_runs(probes, name):
    case = SET_RUNS[name]
    want, added = FK.set_runs_model(case["bits"], case["nbits"], case["runs"])
    blocks = FK.set_runs_blocks(len(case["runs"]))
    exact = FK.set_runs_partials(case["bits"], case["nbits"], case["runs"], blocks)
    assert (exact is not None) or not case.get("exact_partials")
    for fill in FILLS:
        bits, part = run_set(probes, fill, 1, case)
        assert np.array_equal(bits, want), hex(fill)
        check_partials(part, exact, added, blocks, fill, hex(fill))


# ---- popcount -----------------------------------------------------------------------------------------------------------------
POPCOUNT = FK.popcount_cases()


@pytest.mark.parametrize("name", sorted(POPCOUNT))
def test_popcount(probes, name):
    case = POPCOUNT[name]
    want = (case["start"] + FK.popcount(case["bits"])) & M64
    for fill in FILLS:
        out = np.zeros(4, np.uint64)
        probes.done(probes.fb.fb_probe_popcount(fill, ptr(case["bits"]), case["bits"].size, case["start"], ptr(out)), "fb_probe_popcount")
        assert out.tolist() == [want] + [FK.fill64(fill)] * 3, hex(fill)


# ---- combine ------------------------------------------------------------------------------------------------------------------
COMBINE = FK.combine_cases()


@pytest.mark.parametrize("name", sorted(COMBINE))
def test_combine(probes, name):
    case = COMBINE[name]
    words = case["a"].size
    want, count = FK.combine_model(case["a"], case["b"], case["op"])
    blocks = FK.combine_blocks(words)
    exact = FK.combine_partials(want, blocks)
    assert int(exact.sum()) == count
    for fill in FILLS:
        dst, part = np.zeros(words + 1 + FK.PAD, np.uint64), np.zeros(FK.PARTIALS, np.uint64)
        probes.done(probes.fb.fb_probe_combine(fill, ptr(case["a"]), ptr(case["b"]), words, case["op"], ptr(dst), ptr(part)), "fb_probe_combine")
        assert np.array_equal(dst[:words], want), hex(fill)
        assert dst[words:].tolist() == [0] + [FK.fill64(fill)] * FK.PAD, hex(fill) + ": the slack word is cleared, nothing behind it is written"
        check_partials(part, exact, count, blocks, fill, hex(fill))


COMBINE_BATCH = FK.combine_batch_cases()


@pytest.mark.parametrize("name", sorted(COMBINE_BATCH))
def test_combine_batch(probes, name):
    case = COMBINE_BATCH[name]
    ops, table, words, starts = case["ops"], case["table"], case["words"], case["starts"]
    n, per = len(table), words + 1 + FK.PAD
    refused = case.get("refused", False)
    assert refused == (n > FK.BATCH_MAX_N)
    models = {}
    for a, b, op in {tuple(r) for r in table.tolist()}:
        models[(a, b, op)] = FK.combine_model(ops[a], ops[b], op)
    for fill in FILLS:
        f64 = FK.fill64(fill)
        counts = np.concatenate([starts, np.zeros(FK.PAD, np.uint64)])
        dst = np.zeros((n, per), np.uint64)
        rc = probes.done(probes.fb.fb_probe_combine_batch(fill, ptr(ops), len(ops), words, ptr(table), n, ptr(counts), ptr(dst)), "fb_probe_combine_batch",
                         allowed=(-1,) if refused else (0,))
        assert counts[n:].tolist() == [f64] * FK.PAD, hex(fill)
        if refused:   # hipErrorInvalidValue, and nothing written
            assert rc == -1 and np.array_equal(counts[:n], starts) and (dst == np.uint64(f64)).all(), hex(fill)
            continue
        for i, key in enumerate(map(tuple, table.tolist())):
            want, count = models[key]
            assert np.array_equal(dst[i, :words], want), (hex(fill), i)
            assert dst[i, words:].tolist() == [0] + [f64] * FK.PAD, (hex(fill), i)
            assert int(counts[i]) == (int(starts[i]) + count) & M64, (hex(fill), i)


# ---- delta_copy, delta_apply clear, delta_apply set -------------------------------------------------------------------------------
DELTA = FK.delta_cases()


@pytest.mark.parametrize("name", sorted(DELTA))
def test_delta(probes, name):
    case = DELTA[name]
    items, starts = case["items"], case["starts"]
    n = len(items)
    nbits = u64([nb for _, nb in items])
    dst_words = u64([FK.words_of(nb) for _, nb in items])
    base_words = u64([0 if b is None else len(b) for b, _ in items])
    base_off = np.full(n, M64, np.uint64)
    at, parts = 0, []
    for i, (b, _) in enumerate(items):
        if b is not None:
            base_off[i] = at
            parts.append(b)
            at += len(b)
    bases = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
    off = np.concatenate([[0], np.cumsum(dst_words.astype(np.int64) + 1 + FK.PAD)])
    # the model, item by item (only the items that carry records, a base or bits need one)
    by_item = [{}, {}]
    for k, recs in enumerate((case["clr"], case["set"])):
        if len(recs):
            it = (recs >> np.uint64(FK.LABEL_BITS)).astype(np.int64)
            lab = recs & np.uint64((1 << FK.LABEL_BITS) - 1)
            order = np.argsort(it, kind="stable")
            cuts = np.flatnonzero(np.diff(it[order])) + 1
            for grp in np.split(order, cuts):
                by_item[k][int(it[grp[0]])] = lab[grp]
    none = np.zeros(0, np.uint64)
    want_dst, want_cnt = np.zeros(int(off[n]), np.uint64), starts.copy()
    for i, (b, nb) in enumerate(items):
        if nb == 0:             # no word, and no label is below nbits: only the slack word, and the count as it was
            continue
        copied, final, change = FK.delta_model(b, int(dst_words[i]), nb, by_item[0].get(i, none), by_item[1].get(i, none))
        want_dst[off[i]:off[i] + int(dst_words[i])] = copied if case["copy_only"] else final
        if not case["copy_only"]:
            want_cnt[i] = (int(starts[i]) + change) & M64
    for fill in FILLS:
        f64 = FK.fill64(fill)
        want = want_dst.copy()
        for i in range(n):      # the slack word cleared, the pad untouched
            want[off[i] + int(dst_words[i]) + 1:off[i + 1]] = f64
        counts = np.concatenate([starts, np.zeros(FK.PAD, np.uint64)])
        dst = np.zeros(int(off[n]), np.uint64)
        rc = probes.fb.fb_probe_delta(fill, int(case["copy_only"]), ptr(bases), bases.size, ptr(base_off), ptr(base_words), ptr(dst_words), ptr(nbits), n,
                                      case["max_dst_words"], ptr(case["clr"]), len(case["clr"]), ptr(case["set"]), len(case["set"]), ptr(counts), ptr(dst))
        probes.done(rc, "fb_probe_delta")
        assert np.array_equal(dst, want), hex(fill)
        assert np.array_equal(counts[:n], want_cnt) and counts[n:].tolist() == [f64] * FK.PAD, hex(fill)


# ---- node masks ---------------------------------------------------------------------------------------------------------------
NODE_MASK = FK.node_mask_cases()


@pytest.mark.parametrize("name", sorted(NODE_MASK))
def test_node_mask(probes, name):
    case = NODE_MASK[name]
    count, filters, starts = case["count"], case["filters"], case["starts"]
    n, words, pad = len(filters), FK.words_of(case["count"]), probes.nm_pad
    bm_words = u64([len(b) for b, _ in filters])
    bm_off = u64(np.concatenate([[0], np.cumsum(bm_words.astype(np.int64))[:-1]]))
    bitmaps = np.concatenate([b for b, _ in filters])
    nbits = u64([nb for _, nb in filters])
    want = [FK.node_mask_model(case["labels"], case["live"], count, b, nb) for b, nb in filters]
    for fill in FILLS:
        f64 = FK.fill64(fill)
        counts = np.concatenate([starts, np.zeros(pad, np.uint64)])
        dst = np.zeros((n, words + pad), np.uint64)
        rc = probes.nm.nm_probe_run(fill, ptr(case["labels"]), ptr(case["live"]), count, ptr(bitmaps), bitmaps.size, ptr(bm_off), ptr(bm_words), ptr(nbits), n,
                                    ptr(counts), ptr(dst))
        probes.done(rc, "nm_probe_run")
        assert (dst[:, words:] == np.uint64(f64)).all(), hex(fill) + ": words past (count + 63) / 64 were written"
        assert (counts[n:] == np.uint64(f64)).all(), hex(fill)
        for f, (mask, cnt) in enumerate(want):
            assert np.array_equal(dst[f, :words], mask), (hex(fill), f)
            assert int(counts[f]) == (int(starts[f]) + cnt) & M64, (hex(fill), f)


# ---- scatter_u32 / gather_u32 -------------------------------------------------------------------------------------------------
ROWS = FK.rows_cases()


@pytest.mark.parametrize("name", sorted(ROWS))
def test_scatter_then_gather(probes, name):
    case = ROWS[name]
    src, idx, rows = case["src"], case["idx"], case["rows"]
    n, stride = src.shape
    for fill in FILLS:
        dirty = np.full((rows, stride), fill, np.uint32)
        out = np.zeros(rows * stride + 2, np.uint32)
        probes.done(probes.hs.hs_probe_rows(fill, 0, ptr(src), ptr(idx), n, stride, rows, ptr(out)), "hs_probe_rows (scatter)")
        table = out[:rows * stride].reshape(rows, stride)
        assert np.array_equal(table, FK.scatter_model(dirty, src, idx)) and out[rows * stride:].tolist() == [fill, fill], hex(fill)
        back = np.zeros(n * stride + 2, np.uint32)
        probes.done(probes.hs.hs_probe_rows(fill, 1, ptr(table), ptr(idx), n, stride, rows, ptr(back)), "hs_probe_rows (gather)")
        assert np.array_equal(back[:n * stride].reshape(n, stride), src) and back[n * stride:].tolist() == [fill, fill], hex(fill)
        # ... and a gather that repeats rows and reads the untouched ones
        again = np.concatenate([idx[::-1], np.arange(rows, dtype=np.uint32)])
        back = np.zeros(again.size * stride + 2, np.uint32)
        probes.done(probes.hs.hs_probe_rows(fill, 1, ptr(table), ptr(again), again.size, stride, rows, ptr(back)), "hs_probe_rows (gather)")
        assert np.array_equal(back[:again.size * stride].reshape(-1, stride), FK.gather_model(table, again)), hex(fill)
