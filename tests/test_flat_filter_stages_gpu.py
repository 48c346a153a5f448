"""Every stage of the candidate filter (K4h, csrc/flat_filter.hip) against float64 arithmetic, from a dirty workspace.

tests/helpers/filter_probe.hip includes the product's translation unit and runs its launchers -- row_stats + tile cap,
qprep, the sample pass, the bound selection, the early pass, the tighten step, the main pass -- on buffers the probe owns,
each filled with a 32-bit pattern before the first launch and handed back whole.  No assertion here has a tolerance: each
is an inequality against exact (float64) arithmetic over the values the index holds (bf16-rounded rows for bf16; for L2 the
accumulator space dot - |x|^2 / 2), or an equality of bits.

  row_stats   tile_norm >= the exact largest norm of the tile, +inf exactly for tiles the f16 pipe cannot carry; stats[3]
              from the device's own tile norms; hn16 within the split's 2^-21; rows16 == np.float16(x); ranges [lo, hi)
  qprep       q16 un-permuted == the query rounded to nearest even (f16; bf16 on the bf16 matrix-core path); every counter
              zero; closed columns; qwit == the polynomial at the cap with the kernel's fma order
  sample      every smax[q][g < groups] written, <= the exact best score of the group's rows or -inf; groups disjoint
  select      key(qbound) == the k-th largest smax key with its low 12 bits cleared; qbound <= the exact k-th best
  filter      survivors (private list + spill chunks): no duplicates, rows < n_rows and allowed, a superset of every
              allowed row with exact score >= the exact k-th best; counts; |cand_val - exact| <= E_q(R_t)
  two passes  early + tighten + main with 4 and 7 blocks: bound still valid, union a superset, no row twice, the tiles of
              the two passes partition the index
  fills       the whole chain three times over 0x00000000, 0xFFFFFFFF, 0x7F7FFFFF: everything a later stage or the host
              reads is identical, and no such word still holds its fill

Inputs: the seeds of chunks 12, 14 and 15 of test_thousand_seeds_of_small_adversarial_indexes whose draw is bf16 rows with IP
or COSINE (the cases that test has failed on), built by its own _small_case, plus plain random cases at the shapes where the
kernels change path.

Which `fn` branch of launch_flat_filter a variant selects (filter_probe_symbol repeats its branches; the test prints it):

  variant               sample pass                          main pass                              early pass
  f32_ip_reg            flat_filter_sample_kernel<f32,ip>    flat_filter_kernel<f32,ip>             (same symbol)
  f32_ip_bdma           flat_filter_sample_kernel<f32,ip>    flat_filter_bdma_kernel<f32,ip>        flat_filter_early_kernel<f32,ip>
  f32_ip_image          flat_filter_sample_kernel<f32,ip>    flat_filter_bdma_kernel<f32,ip,image>  flat_filter_early_kernel<f32,ip,image>
  bf16_ip_f16pipe       flat_filter_sample_kernel<bf16,ip>   flat_filter_kernel<bf16,ip>            (same symbol)
  bf16_ip_f16pipe_bdma  flat_filter_sample_kernel<bf16,ip>   flat_filter_bdma_kernel<bf16,ip>       flat_filter_early_kernel<bf16,ip>
  bf16_ip_bfmma         flat_filter_bfmma_sample_kernel      flat_filter_bfmma_kernel               (same symbol)
  bf16_ip_bfmma_bdma    flat_filter_bfmma_sample_kernel      flat_filter_bdma_kernel<bf16,ip,bfmma> flat_filter_early_kernel<bf16,ip,bfmma>
  bf16_ip_bfmma_dma     flat_filter_bfmma_sample_kernel      flat_filter_bfmma_dma_kernel           flat_filter_early_bfmma_dma_kernel
  f32_l2_reg            flat_filter_sample_kernel<f32,l2>    flat_filter_kernel<f32,l2>             (same symbol)
  f32_l2_bdma           flat_filter_sample_kernel<f32,l2>    flat_filter_bdma_kernel<f32,l2>        flat_filter_early_kernel<f32,l2>
  bf16_l2_reg           flat_filter_sample_kernel<bf16,l2>   flat_filter_kernel<bf16,l2>            (same symbol)
  bf16_l2_bdma          flat_filter_sample_kernel<bf16,l2>   flat_filter_bdma_kernel<bf16,l2>       flat_filter_early_kernel<bf16,l2>
"""
import ctypes as C
import subprocess
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HERE = ROOT / "tests" / "helpers"
CSRC = ROOT / "valkey-search_amd" / "csrc"
LIB = HERE / "libfilterprobe.so"
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(ROOT / "tests"))

QPREP, SAMPLE, SELECT, EARLY, TIGHTEN, MAIN = 1, 2, 4, 8, 16, 32
ONE_PASS = QPREP | SAMPLE | SELECT | MAIN
TWO_PASS = QPREP | SAMPLE | SELECT | EARLY | TIGHTEN | MAIN
FILLS = [0x00000000, 0xFFFFFFFF, 0x7F7FFFFF]
NAN_FILL = 0xFFFFFFFF
SPILL_CHUNK, SPILL_PER_QUERY = 4096, 32        # kernels.hpp: kSpillChunk, kSpillPerQuery
INF_BITS = 0x7F800000

# (bf16, l2, qbf16, dma, bdma, image)
VARIANTS = {
    "f32_ip_reg": (0, 0, 0, 0, 0, 0),
    "f32_ip_bdma": (0, 0, 0, 0, 1, 0),
    "f32_ip_image": (0, 0, 0, 0, 1, 1),
    "bf16_ip_f16pipe": (1, 0, 0, 0, 0, 0),
    "bf16_ip_f16pipe_bdma": (1, 0, 0, 0, 1, 0),
    "bf16_ip_bfmma": (1, 0, 1, 0, 0, 0),
    "bf16_ip_bfmma_bdma": (1, 0, 1, 0, 1, 0),
    "bf16_ip_bfmma_dma": (1, 0, 1, 1, 1, 0),
    "f32_l2_reg": (0, 1, 0, 0, 0, 0),
    "f32_l2_bdma": (0, 1, 0, 0, 1, 0),
    "bf16_l2_reg": (1, 1, 0, 0, 0, 0),
    "bf16_l2_bdma": (1, 1, 0, 0, 1, 0),
}


def build_probe():
    src = HERE / "filter_probe.hip"
    newest = max(p.stat().st_mtime for p in (src, CSRC / "flat_filter.hip", CSRC / "kernels.hpp", CSRC / "device_common.hpp"))
    if not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", "-I", str(CSRC), str(src),
                               "-o", str(LIB)])
    return LIB


class Cfg(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_rows", "stride", "nq", "k", "bf16", "l2", "qbf16", "dma", "bdma", "image", "fill", "cap",
                                          "n_chunks", "sample_rows", "blocks", "early_tiles", "stages", "allow_nbits")]


class IO(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rows", "queries", "labels", "allow_bits", "tile_norm", "stats", "q16", "thr", "words", "smax",
                                          "cand", "spill", "qbound_select", "cnt_early")]


def bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(x):
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Out:
    pass


class Probe:
    def __init__(self):
        lib = C.CDLL(str(build_probe()))
        u32, vp = C.c_uint32, C.c_void_p
        lib.filter_probe_layout.argtypes = [C.POINTER(Cfg), vp]
        lib.filter_probe_layout.restype = C.c_int
        lib.filter_probe_sample_row.argtypes = [u32] * 5
        lib.filter_probe_sample_row.restype = C.c_uint64
        lib.filter_probe_symbol.argtypes = [u32] * 8
        lib.filter_probe_symbol.restype = C.c_char_p
        lib.filter_probe_row_stats.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32, u32, vp, vp, vp, vp]
        lib.filter_probe_row_stats.restype = C.c_int
        lib.filter_probe_chain.argtypes = [C.POINTER(Cfg), C.POINTER(IO)]
        lib.filter_probe_chain.restype = C.c_int
        self.lib = lib

    def symbols(self, variant, two_pass):
        v = VARIANTS[variant]
        s = [self.lib.filter_probe_symbol(*v, 1, 0).decode(), self.lib.filter_probe_symbol(*v, 0, 0).decode()]
        if two_pass:
            s.append(self.lib.filter_probe_symbol(*v, 0, 1).decode())
        return s

    def row_stats(self, X, bf16, l2, lo, hi, image, fill):
        n, stride = X.shape
        n_tiles = (n + 127) // 128
        alloc = n_tiles * 128 + 256
        rows = bf16_bits(X) if bf16 else np.ascontiguousarray(X, np.float32)
        o = Out()
        o.tile_norm = np.zeros(n_tiles + 2, np.uint32)
        o.stats = np.zeros(16, np.uint32)
        o.hn16 = np.zeros(alloc, np.uint32)
        o.rows16 = np.zeros((alloc, stride) if image else (1, 1), np.uint16)
        rc = self.lib.filter_probe_row_stats(ptr(rows), bf16, l2, stride, n, lo, hi, image, fill, ptr(o.tile_norm), ptr(o.stats), ptr(o.hn16),
                                             ptr(o.rows16))
        assert rc == 0, "filter_probe_row_stats -> %d" % rc
        return o

    def chain(self, case, variant, *, stages, fill=NAN_FILL, cap=8192, n_chunks=8, sample_rows=1024, blocks=256, early_tiles=0, k=None):
        bf16, l2, qbf16, dma, bdma, image = VARIANTS[variant]
        assert bool(bf16) == case.bf16 and bool(l2) == case.l2, (variant, case.bf16, case.l2)
        n, stride = case.X.shape
        nq = case.Q.shape[0]
        k = case.k if k is None else k
        nbits = 0 if case.allow is None else n
        blocks = min(blocks, (n + 127) // 128)                  # scan_filter's filter_grid: min(CUs, tiles)
        cfg = Cfg(n, stride, nq, k, bf16, l2, qbf16, dma, bdma, image, fill, cap, n_chunks, sample_rows, blocks, early_tiles, stages, nbits)
        lay = np.zeros(8, np.uint32)
        assert self.lib.filter_probe_layout(C.byref(cfg), ptr(lay)) == 0
        n_s, gap, fine, groups, smax_ld, nqt, n_tiles, _alloc = (int(v) for v in lay)
        rows = bf16_bits(case.X) if bf16 else np.ascontiguousarray(case.X, np.float32)
        queries = np.ascontiguousarray(case.Q, np.float32)
        labels = np.arange(n, dtype=np.uint64)
        allow_bits = None
        if case.allow is not None:
            allow_bits = np.packbits(case.allow.astype(np.uint8), bitorder="little")
            allow_bits = np.concatenate([allow_bits, np.zeros((-len(allow_bits)) % 8 + 8, np.uint8)]).view(np.uint64)
        w_chunk, w_done = 3 * nq + 4, 3 * nq + 4 + nq * SPILL_PER_QUERY
        tile_norm = np.zeros(n_tiles + 2, np.uint32)
        stats = np.zeros(16, np.uint32)
        q16 = np.zeros(nqt * 32 * stride, np.uint16)
        thr = np.zeros(nqt * 32 * 6, np.float32)
        words = np.zeros(w_done + 2 * nq, np.uint32)
        smax = np.zeros((nq, smax_ld), np.float32)
        cand = np.zeros(2 * nq * cap, np.uint32)
        spill = np.zeros(2 * max(n_chunks, 1) * SPILL_CHUNK, np.uint32)
        qsel = np.full(nqt * 32, np.nan, np.float32)
        cnt_early = np.zeros(nq, np.uint32)
        io = IO(ptr(rows), ptr(queries), ptr(labels), None if allow_bits is None else ptr(allow_bits), ptr(tile_norm), ptr(stats), ptr(q16),
                ptr(thr), ptr(words), ptr(smax), ptr(cand), ptr(spill), ptr(qsel), ptr(cnt_early))
        rc = self.lib.filter_probe_chain(C.byref(cfg), C.byref(io))
        assert rc == 0, "filter_probe_chain -> %d (1 refused, 2 qprep left a counter unwritten, else a source line) %s" % (rc, variant)
        o = Out()
        o.n_s, o.gap, o.fine, o.groups, o.smax_ld, o.nqt, o.n_tiles = n_s, gap, fine, groups, smax_ld, nqt, n_tiles
        o.cap, o.n_chunks, o.k, o.nq, o.fill, o.qbf16, o.bf16 = cap, n_chunks, k, nq, fill, qbf16, bf16
        o.tile_norm, o.stats, o.smax = tile_norm, stats, smax
        # fragment order -> [column][element]: (jt, ks, g, jj, t) holds element ks * 16 + g * 8 + t of column jt * 32 + jj
        o.q16 = q16.reshape(nqt, stride // 16, 2, 32, 8).transpose(0, 3, 1, 2, 4).reshape(nqt * 32, stride)
        o.qcoef = thr[:nqt * 32 * 4].reshape(nqt * 32, 4)
        o.qbound = thr[nqt * 32 * 4:nqt * 32 * 5]
        o.qwit = thr[nqt * 32 * 5:]
        o.qbound_select = qsel
        o.cnt, o.ovf, o.misc = words[:nq], words[nq:2 * nq], words[2 * nq:2 * nq + 4]
        o.qchunk = words[w_chunk:w_done].reshape(nq, SPILL_PER_QUERY)
        o.done, o.rerank = words[w_done:w_done + nq], words[w_done + nq:]
        o.cand_row = cand[:nq * cap].reshape(nq, cap)
        o.cand_val = cand[nq * cap:].view(np.float32).reshape(nq, cap)
        o.spill = spill[:n_chunks * SPILL_CHUNK].reshape(n_chunks, SPILL_CHUNK)
        o.spill_val = spill[max(n_chunks, 1) * SPILL_CHUNK:][:n_chunks * SPILL_CHUNK].view(np.float32).reshape(n_chunks, SPILL_CHUNK)
        o.cnt_early = cnt_early
        return o

    def group_rows(self, o):
        """[groups][rows per group] index rows of every group of the sample (sample_row() and sample_max's register map)"""
        kR = 16 if o.bf16 else 8
        t = np.arange(o.n_s)[:, None]
        i = np.arange(128)[None, :]
        row = (((i // kR) * o.n_s + t) * kR + i % kR) * o.gap                                   # [n_s][128]
        assert int(row[o.n_s - 1, 127]) == self.lib.filter_probe_sample_row(o.bf16, o.n_s, o.gap, o.n_s - 1, 127)
        assert int(row[0, 77]) == self.lib.filter_probe_sample_row(o.bf16, o.n_s, o.gap, 0, 77)
        r = np.arange(16)
        out = np.zeros((o.groups, 16 if o.fine else 64), np.int64)
        for tile in range(o.n_s):
            for g in range(2):
                loc = [rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * g for rt in range(4)]               # local rows of (rt, g)
                if o.fine:
                    for rt in range(4):
                        out[(tile * 4 + rt) * 2 + g] = row[tile, loc[rt]]
                else:
                    out[tile * 2 + g] = row[tile, np.concatenate(loc)]
        return out


@pytest.fixture(scope="module")
def probe():
    return Probe()


# ---- cases and their float64 references ------------------------------------------------------------------------------------
class Case:
    def __init__(self, X, Q, bf16, l2, k, allow=None):
        self.bf16, self.l2, self.k, self.allow = bool(bf16), bool(l2), int(k), allow
        self.X = bf16_value(X) if bf16 else np.ascontiguousarray(X, np.float32)      # the values the index holds
        self.Q = np.ascontiguousarray(Q, np.float32)
        self._ref = None

    def ref(self):
        """exact scores [n][nq] in accumulator space, exact row norms [n]; computed once"""
        if self._ref is None:
            Xd, Qd = self.X.astype(np.float64), self.Q.astype(np.float64)
            ok = np.isfinite(Qd).all(1)
            with np.errstate(all="ignore"):
                S = Xd @ np.where(ok[:, None], Qd, 0.0).T
                n2 = (Xd * Xd).sum(1)
                if self.l2:
                    S = S - 0.5 * n2[:, None]
            self._ref = (S, np.sqrt(n2), n2)
        return self._ref

    def kth(self, k):
        """exact k-th best score per query over the allowed rows (-inf when there are fewer than k)"""
        S = self.ref()[0]
        if self.allow is not None:
            S = np.where(self.allow[:, None], S, -np.inf)
        if k > S.shape[0]:
            return np.full(S.shape[1], -np.inf)
        return np.partition(S, S.shape[0] - k, axis=0)[S.shape[0] - k]


_CASES = {}


def plain_case(kind, n, dim, nq, k, l2, bf16, allow):
    key = (kind, n, dim, nq, k, l2, bf16, allow)
    if key not in _CASES:
        rng = np.random.default_rng(abs(hash(key[1:6])) % (1 << 32))
        if kind == "same":            # every row the same vector: every row has the same score, so every row survives any bound
            X = np.repeat(rng.standard_normal((1, dim)).astype(np.float32), n, 0)
            Q = rng.standard_normal((nq, dim)).astype(np.float32)
        else:                         # clustered rows, queries near rows: neighbours that are near
            cen = rng.standard_normal((16, dim)).astype(np.float32)
            X = (cen[rng.integers(0, 16, n)] + 0.5 * rng.standard_normal((n, dim))).astype(np.float32) / np.float32(np.sqrt(dim))
            Q = (X[rng.integers(0, n, nq)] + 0.05 * rng.standard_normal((nq, dim)).astype(np.float32)).astype(np.float32)
        a = (rng.random(n) < 0.4) if allow else None
        _CASES[key] = Case(X, Q, bf16, l2, k, a)
        if len(_CASES) > 24:
            _CASES.pop(next(iter(_CASES)))
    return _CASES[key]


def _seed_head(seed):
    """the first draws of _small_case (tests/test_flat_filter_adversarial_gpu.py), to name the cases at collection time"""
    rng = np.random.default_rng(770000 + seed)
    dim = int(rng.choice([64, 128, 192, 256, 320]))
    dtype = "bf16" if rng.random() < 0.3 else "f32"
    metric = str(rng.choice(["IP", "IP", "L2", "COSINE"]))
    return dim, dtype, metric


# chunks 12, 14 and 15 of test_thousand_seeds_of_small_adversarial_indexes, the draws with bf16 rows and IP or COSINE
BF16_SEEDS = [s for s in list(range(768, 832)) + list(range(896, 1024)) if _seed_head(s)[1] == "bf16" and _seed_head(s)[2] != "L2"]


def seed_case(seed):
    key = ("seed", seed)
    if key not in _CASES:
        import test_flat_filter_adversarial_gpu as adv
        dim, dtype, metric, k, X, Q = adv._small_case(np.random.default_rng(770000 + seed))
        assert (dim, dtype, metric) == _seed_head(seed)
        _CASES[key] = Case(X, Q, dtype == "bf16", metric == "L2", k)
        if len(_CASES) > 24:
            _CASES.pop(next(iter(_CASES)))
    return _CASES[key]


def product_sample_rows(k):
    """filter_prepass_rows(k) under the sweep's options (filter-prepass-rows 1024): 1024 per ten of k"""
    return 1024 * ((k + 9) // 10)


# ---- the properties -----------------------------------------------------------------------------------------------------------
def key_of(f32):
    u = np.ascontiguousarray(f32, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def margins(o, R):
    """E_q(R) in float64 from the device's coefficients: [len(R)][nq]"""
    c = o.qcoef[:o.nq].astype(np.float64)
    R = np.asarray(R, np.float64)[:, None]
    with np.errstate(all="ignore"):
        return c[None, :, 0] * R * R + c[None, :, 1] * R + c[None, :, 2]


def f32_round(fr):
    """a non-negative Fraction rounded to nearest even float32 (normal range; beyond it +inf)"""
    if fr == 0:
        return np.float32(0)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1
    e = max(e, -126)
    m = fr / Fraction(2) ** (e - 23)
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    v = Fraction(n) * Fraction(2) ** (e - 23)
    return np.float32(np.inf) if v >= Fraction(2) ** 128 else np.float32(float(v))


def fma32(a, b, c):
    return f32_round(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def check_qprep(case, o, counters=True):
    nq, Q = o.nq, case.Q
    ok = np.isfinite(Q).all(1) & (np.abs(np.where(np.isfinite(Q), Q, 0)).max(1) <= 32768.0)
    with np.errstate(all="ignore"):
        want = bf16_bits(Q) if o.qbf16 else Q.astype(np.float16).view(np.uint16)
    want = np.where(ok[:, None], want, 0).astype(np.uint16)
    assert (o.q16[:nq] == want).all(), "q16: column %d differs from the query rounded to nearest even" % int(np.argmax((o.q16[:nq] != want).any(1)))
    # columns behind the batch replicate the last query (flat_qprep_kernel) and are CLOSED: nothing of them reaches a list
    assert (o.q16[nq:] == want[nq - 1]).all(), "q16: a padding column is neither the last query nor written"
    assert (o.qcoef[nq:, 3] == 1).all() and (o.qcoef[nq:, :3] == 0).all(), "qcoef: padding columns are closed"
    assert (o.qcoef[:nq, 3] == np.where(ok, 0, 1)).all(), "qcoef.w: closed exactly for the queries outside f16"
    assert (o.ovf[:nq] == np.where(ok, 0, 1)).all(), "ovf_q: raised exactly for the queries outside f16"
    for name, a in (("cand_cnt", o.cnt), ("qchunk", o.qchunk), ("spill_next", o.misc[:1]), ("redo_cnt", o.misc[1:2]), ("done_cnt", o.done),
                    ("rerank_cnt", o.rerank))[:6 if counters else 0]:      # (behind the passes the first three count)
        assert not a.any(), "%s[%d] is not zero behind qprep" % (name, int(np.flatnonzero(a.ravel())[0]))
    Rc = o.stats[3:4].view(np.float32)[0]
    for j in range(o.nqt * 32):
        c = o.qcoef[j]
        if np.isfinite(c[:3]).all():
            w = fma32(fma32(c[0], Rc, c[1]), Rc, c[2])
            assert o.qwit[j].view(np.uint32) == w.view(np.uint32), "qwit[%d] = %r, the polynomial at the cap gives %r" % (j, o.qwit[j], w)
    assert (o.qcoef[:nq][ok][:, 1:3] > 0).all() and np.isfinite(o.qcoef[:nq][ok]).all()


def check_sample_select(case, o, probe, k):
    S = case.ref()[0]
    nq = o.nq
    sm = o.smax[:, :o.groups]
    if o.fill != 0:
        bad = np.argwhere(sm.view(np.uint32) == o.fill)
        assert len(bad) == 0, "smax[%d][%d] still holds the fill behind the sample pass" % tuple(bad[0])
    assert not np.isnan(sm).any(), "smax holds a NaN"
    gr = probe.group_rows(o)
    flat = gr.ravel()
    assert len(np.unique(flat)) == len(flat), "two groups of the sample share a row"
    assert flat.max() < case.X.shape[0]
    Sg = S[gr]                                                  # [groups][rows per group][nq]
    if case.allow is not None:
        Sg = np.where(case.allow[gr][:, :, None], Sg, -np.inf)
    best = Sg.max(1).T                                          # [nq][groups]
    closed = o.qcoef[:nq, 3] != 0
    bad = np.argwhere((sm.astype(np.float64) > best) & ~np.isneginf(sm))
    assert len(bad) == 0, "smax[%d][%d] = %r is above the group's exact best score %r" % (
        bad[0][0], bad[0][1], sm[tuple(bad[0])], best[tuple(bad[0])])
    assert np.isneginf(sm[closed]).all(), "a closed column has a group bound"
    # the bound selection: the k-th largest key to 20 bits from below
    keys = key_of(sm)
    want = np.full(nq, -np.inf, np.float32)
    if k <= o.groups:
        T = (np.sort(keys, axis=1)[:, o.groups - k] & np.uint32(0xFFFFF000)).astype(np.uint32)
        b = np.where(T & 0x80000000, T & 0x7FFFFFFF, ~T).astype(np.uint32).view(np.float32)
        want = np.where(np.isnan(b) | (T == 0), np.float32(-np.inf), b).astype(np.float32)
    got = o.qbound_select[:nq]
    assert (got.view(np.uint32) == want.view(np.uint32)).all(), "qbound[%d] = %r, the k-th largest group bound to 20 bits is %r" % (
        int(np.argmax(got.view(np.uint32) != want.view(np.uint32))), got[np.argmax(got.view(np.uint32) != want.view(np.uint32))],
        want[np.argmax(got.view(np.uint32) != want.view(np.uint32))])
    kth = case.kth(k)
    bad = np.flatnonzero(got.astype(np.float64) > kth)
    assert len(bad) == 0, "query %d: the selected bound %r is above the exact k-th best score %r" % (bad[0], got[bad[0]], kth[bad[0]])


def survivors(o, q, lo=0):
    """(rows, scores) of query q's stored survivors from list position lo on: the private list, then its spill chunks"""
    cnt = int(o.cnt[q])
    rows, vals = [o.cand_row[q, lo:min(cnt, o.cap)]], [o.cand_val[q, lo:min(cnt, o.cap)]]
    stored = min(cnt, o.cap)
    for c in range(SPILL_PER_QUERY):
        left = cnt - o.cap - c * SPILL_CHUNK
        if left <= 0:
            break
        cid = int(o.qchunk[q, c])
        if cid < 2 or cid == 0xFFFFFFFF:
            break
        assert cid - 2 < o.n_chunks, "qchunk[%d][%d] = %d names no chunk of the pool" % (q, c, cid)
        m = min(left, SPILL_CHUNK)
        rows.append(o.spill[cid - 2, :m])
        vals.append(o.spill_val[cid - 2, :m])
        stored += m
    return np.concatenate(rows).astype(np.int64), np.concatenate(vals), stored


def check_survivors(case, o, k, ovf_allowed=False, need_superset=True):
    S, norm, _ = case.ref()
    n = case.X.shape[0]
    kth = case.kth(k)
    tile_R = o.tile_norm[:o.n_tiles].view(np.float32).astype(np.float64)
    tiles = np.arange(n) >> 7
    assert (tile_R[tiles] >= norm).all(), "tile_norm below a row's exact norm"
    E = margins(o, tile_R)                                       # [n_tiles][nq]
    closed = o.qcoef[:o.nq, 3] != 0
    if not ovf_allowed:
        assert (o.ovf[~closed] == 0).all(), "ovf_q raised for query %d: the case was not built for that" % int(np.flatnonzero(o.ovf)[0])
        # the test's own inputs: the rows within two margins of the k-th best fit the private list
        with np.errstate(all="ignore"):
            near = (S >= (kth - 2 * margins(o, [tile_R[np.isfinite(tile_R)].max()])[0])[None, :]).sum(0)
        assert (near[~closed] < o.cap).all(), "precondition: %d rows within 2 E of the k-th best, cap %d" % (near.max(), o.cap)
    sets = []
    for q in range(o.nq):
        rows, vals, stored = survivors(o, q)
        sets.append(rows)
        if closed[q]:
            assert len(rows) == 0, "query %d is closed and has survivors" % q
            continue
        assert len(np.unique(rows)) == len(rows), "query %d: a row is listed twice" % q
        assert len(rows) == 0 or rows.max() < n, "query %d: row slot %d >= n_rows" % (q, rows.max())
        if case.allow is not None:
            assert case.allow[rows].all(), "query %d: a row the filter does not allow survived" % q
        assert int(o.cnt[q]) == stored or (int(o.cnt[q]) > stored and o.ovf[q] != 0), "query %d: cand_cnt %d, %d stored, ovf %d" % (
            q, o.cnt[q], stored, o.ovf[q])
        err = np.abs(vals.astype(np.float64) - S[rows, q])
        e = E[rows >> 7, q]
        with np.errstate(all="ignore"):
            bad = np.flatnonzero(np.isfinite(e) & ~(err <= e))
        assert len(bad) == 0, "query %d row %d: |approx - exact| = %.4g exceeds E_q(R_t) = %.4g (%.2f E)" % (
            q, rows[bad[0]], err[bad[0]], e[bad[0]], err[bad[0]] / e[bad[0]])
        if need_superset and not (ovf_allowed and o.ovf[q] != 0):
            must = S[:, q] >= kth[q]
            if case.allow is not None:
                must &= case.allow
            lost = np.setdiff1d(np.flatnonzero(must), rows)
            assert len(lost) == 0, "query %d lost row %d: exact score %r >= the exact k-th best %r; bound %r, E %r" % (
                q, lost[0], S[lost[0], q], kth[q], o.qbound[q], E[lost[0] >> 7, q])
    return sets


def half_norm_f32(X):
    """|x|^2 / 2 as row_stats_kernel's lane 0 of a quad gets it, in float32: lane j owns the 4-element pieces c * 4 + j, each
    taken up as fma(x, x, fma(y, y, fma(z, z, fma(w, w, n2)))), then (n0 + n1) + (n2 + n3).  (x * x is exact in float64, so
    float32(x * x + n2) is the fused result but for a double rounding that needs a tie in the 29 bits between the formats.)"""
    m, d = X.shape
    P = np.ascontiguousarray(X, np.float32).reshape(m, d // 16, 4, 4).astype(np.float64)
    acc = np.zeros((m, 4), np.float32)
    for c in range(d // 16):
        for e in (3, 2, 1, 0):
            acc = (P[:, c, :, e] * P[:, c, :, e] + acc.astype(np.float64)).astype(np.float32)
    return np.float32(0.5) * ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3]))


# ---- row statistics -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16,l2,dim,n,lo,hi", [
    (0, 0, 64, 128 * 24 + 1, 0, None), (0, 0, 320, 128 * 30 - 1, 0, 128 * 20 + 37), (0, 0, 192, 128 * 30, 128 * 7 + 77, 128 * 19 + 5),
    (0, 1, 192, 128 * 24 + 1, 0, None), (0, 1, 64, 128 * 30, 128 * 3 + 41, 128 * 29 + 127), (1, 0, 320, 128 * 24 - 1, 0, None),
    (1, 1, 64, 128 * 24 + 1, 128 * 2, 128 * 20 + 1), (0, 1, 320, 128 * 24, 128 * 2 + 127, 128 * 22 + 1)])
def test_row_stats_and_tile_cap(probe, bf16, l2, dim, n, lo, hi):
    hi = n if hi is None else hi
    lo_eff = lo & ~127        # launch_row_stats starts at the tile edge below lo: rows [lo_eff, lo) are read and written again
    rng = np.random.default_rng(n * 7 + dim + l2)
    X = (rng.standard_normal((n, dim)) * np.exp2(rng.integers(-3, 4, (n, 1)))).astype(np.float32)
    bad_rows = {lo + 200: np.inf, lo + 700: -np.inf, lo + 1300: 40000.0}            # values the f16 pipe cannot carry
    if l2:
        X[lo + 1700] = 400.0 / np.sqrt(dim) * 2                                     # half norm 320 000: beyond f16 (60 000)
    if not bf16:
        for r, v in bad_rows.items():
            X[r, dim // 3] = v
    else:
        X[lo + 200, 5] = np.inf
        X[lo + 1300, 7] = 65536.0
    X = bf16_value(X) if bf16 else X
    image = int(not bf16 and not l2)
    for fill in (NAN_FILL, 0x7F7FFFFF):
        o = probe.row_stats(X, bf16, l2, lo, hi, image, fill)
        n_tiles = (n + 127) // 128
        Xd = X.astype(np.float64)
        with np.errstate(all="ignore"):
            n2 = (Xd * Xd).sum(1)
            cannot = ~np.isfinite(Xd).all(1) | (np.abs(Xd).max(1) > 32768) | (bool(l2) & (0.5 * n2 > 60000 * 1.01))
        tn = o.tile_norm[:n_tiles]
        for t in range(n_tiles):
            a, b = max(t * 128, lo_eff), min(t * 128 + 128, hi)
            if a >= b:
                assert tn[t] == 0, "tile %d outside [lo, hi) was written" % t
                continue
            if cannot[a:b].any():
                assert tn[t] == INF_BITS, "tile %d holds a value outside f16 and is not +inf (%#x)" % (t, tn[t])
            else:
                assert tn[t] < INF_BITS and float(tn[t:t + 1].view(np.float32)[0]) >= np.sqrt(n2[a:b].max()), "tile_norm[%d]" % t
        assert o.tile_norm[n_tiles:].tolist() == [0, 0]
        # the norm cap from the device's own tile norms (tile_cap_kernel)
        fin = tn[tn < INF_BITS]
        hist = np.bincount(fin >> 20, minlength=2048)
        want = len(fin) - len(fin) // 32
        b = int(np.argmax(np.cumsum(hist) >= want))
        assert int(o.stats[3]) == (0 if len(fin) == 0 else 0x7F7FFFFF if b >= 2039 else (b + 1) << 20)
        assert int(o.stats[2]) == int((tn == INF_BITS).sum())
        if l2:
            with np.errstate(all="ignore"):
              hv = (o.hn16 & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64) + (o.hn16 >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
            good = np.flatnonzero(~cannot[lo_eff:hi]) + lo_eff
            half = 0.5 * n2[good]
            h32 = half_norm_f32(X[good]).astype(np.float64)
            # the split (hi = f16(hn), lo = f16(hn - hi)) keeps 2^-21 of the f32 half norm it is given ...
            worst = (np.abs(hv[good] - h32) / h32).max()
            print("hn16: worst |hi + lo - hn| / hn = 2^%.2f" % np.log2(max(worst, 2.0 ** -60)))
            assert (np.abs(hv[good] - h32) <= 2.0 ** -21 * h32).all(), "hn16: hi + lo off the f32 half norm by more than 2^-21"
            # ... and that f32 value is a sum of dim / 4 fused multiply-adds per lane and two additions, all terms positive:
            # at most (dim / 4 + 2) roundings of 2^-24 each away from the exact sum (first order; 1 % for the higher ones)
            assert (np.abs(h32 - half) <= 1.01 * (dim / 4 + 2) * 2.0 ** -24 * half).all(), "the f32 half norm is off |x|^2 / 2"
            outside = np.r_[np.arange(0, lo_eff), np.arange(hi, len(o.hn16))]
            assert (o.hn16[outside] == fill).all(), "hn16 written outside [lo, hi)"
        if image:
            with np.errstate(all="ignore"):
                want16 = X[lo_eff:hi].astype(np.float16).view(np.uint16)
            assert (o.rows16[lo_eff:hi] == want16).all(), "rows16 != np.float16(x)"
            assert (o.rows16[:lo_eff].view(np.uint32) == fill).all() and (o.rows16[hi:].view(np.uint32) == fill).all(), "rows16 written outside [lo, hi)"


# ---- qprep ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,dim,nq", [("f32_ip_reg", 64, 1), ("f32_ip_bdma", 320, 31), ("bf16_ip_bfmma_dma", 192, 33), ("f32_l2_reg", 192, 32),
                                            ("bf16_l2_bdma", 64, 257), ("bf16_ip_f16pipe", 320, 257), ("bf16_ip_bfmma", 64, 33)])
def test_qprep(probe, variant, dim, nq):
    bf16, l2 = VARIANTS[variant][:2]
    case = plain_case("near", 128 * 24 + 1, dim, nq, 10, l2, bf16, False)
    Q = case.Q.copy()
    # rounding midpoints of both formats, f16 subnormals, the largest value that goes through, and queries that do not
    Q[0, :8] = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 + 2.0 ** -40, 32768.0]
    if nq > 2:
        Q[1, 3] = np.inf
        Q[nq - 2, 0] = 32769.0
        Q[nq // 2, dim - 1] = np.nan
    c2 = Case(case.X, Q, bf16, l2, 10)
    for fill in FILLS:
        o = probe.chain(c2, variant, stages=QPREP, fill=fill)
        check_qprep(c2, o)


# ---- one pass, every variant -------------------------------------------------------------------------------------------------------
#        dim  n_rows         nq   k  allow sample_rows blocks
SHAPES = [(64, 128 * 40 - 1, 33, 10, False, 1024, 256),
          (192, 128 * 40 + 1, 31, 1, True, 384, 7),         # groups = 24: smax_ld = 64 > groups
          (320, 128 * 36, 257, 32, False, 4096, 64),        # a second launch of 256 queries, nq % 32 != 0
          (64, 128 * 48 + 1, 1, 100, True, 2048, 256),      # k > 64
          (192, 128 * 200 - 1, 32, 10, False, 1024, 256)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_n%d_q%d_k%d_%s" % (s[0], s[1], s[2], s[3], "allow" if s[4] else "all"))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_one_pass_every_variant(probe, variant, shape):
    dim, n, nq, k, allow, sample_rows, blocks = shape
    bf16, l2 = VARIANTS[variant][:2]
    case = plain_case("near", n, dim, nq, k, l2, bf16, allow)
    print(variant, "->", probe.symbols(variant, False))
    o = probe.chain(case, variant, stages=ONE_PASS, sample_rows=sample_rows, blocks=blocks, cap=max(8192, 64 * k))
    check_qprep_light(case, o)
    check_sample_select(case, o, probe, k)
    assert (o.qbound[:nq].view(np.uint32) == o.qbound_select[:nq].view(np.uint32)).all()
    check_survivors(case, o, k)


def check_qprep_light(case, o):
    ok = np.isfinite(case.Q).all(1)
    want = bf16_bits(case.Q) if o.qbf16 else case.Q.astype(np.float16).view(np.uint16)
    assert (o.q16[:o.nq][ok] == want[ok]).all()


def test_coarse_groups(probe):
    """n_s * 8 > 4096: two groups of 64 rows per sample tile, and the 64-values-per-thread selection"""
    n, dim, nq, k = 128 * 2100 + 1, 64, 33, 10
    case = plain_case("near", n, dim, nq, k, 0, 1, False)
    for variant in ("bf16_ip_bfmma_dma", "bf16_ip_f16pipe"):
        o = probe.chain(case, variant, stages=ONE_PASS, sample_rows=128 * 2100, blocks=256)
        assert not o.fine and o.groups == 4200 and o.groups > 4096
        check_sample_select(case, o, probe, k)
        check_survivors(case, o, k)


def test_spill_chunks_and_a_pool_that_runs_out(probe):
    """cap 64: the lists continue in spill chunks; with one chunk for all queries the pool runs out and ovf_q is raised"""
    n, dim, nq, k = 128 * 80 + 1, 64, 33, 1
    case = plain_case("same", n, dim, nq, k, 0, 0, False)
    for variant in ("f32_ip_bdma", "f32_ip_image", "f32_ip_reg"):
        o = probe.chain(case, variant, stages=ONE_PASS, cap=64, n_chunks=33 * 3, sample_rows=1024)
        sets = check_survivors_same(o)
        assert all(len(s) == n for s in sets) and int(o.misc[0]) == 33 * 3 and not o.ovf.any()
        o = probe.chain(case, variant, stages=ONE_PASS, cap=64, n_chunks=2, sample_rows=1024)
        assert int(o.ovf.sum()) >= nq - 2 and int(o.misc[0]) >= 2
        check_survivors(case, o, k, ovf_allowed=True)


def check_survivors_same(o):
    """every row has the same exact score, so every row must survive: the near-the-k-th precondition does not apply"""
    sets = []
    for q in range(o.nq):
        rows, vals, stored = survivors(o, q)
        assert len(np.unique(rows)) == len(rows) and stored == int(o.cnt[q])
        sets.append(rows)
    return sets


# ---- two passes ------------------------------------------------------------------------------------------------------------------
TWO = [("f32_ip_bdma", 64, 128 * 70 + 1, 7, 4), ("f32_ip_image", 192, 128 * 128, 4, 8), ("bf16_ip_bfmma_dma", 320, 128 * 112 - 1, 7, 3),
       ("bf16_ip_bfmma_bdma", 64, 128 * 130, 4, 6), ("bf16_ip_bfmma", 192, 128 * 70 + 1, 4, 4), ("f32_l2_bdma", 64, 128 * 126, 7, 4),
       ("bf16_l2_bdma", 192, 128 * 70 - 1, 4, 5), ("f32_l2_reg", 320, 128 * 72, 4, 4), ("bf16_l2_reg", 64, 128 * 101, 7, 3),
       ("f32_ip_reg", 320, 128 * 70 + 1, 7, 2), ("bf16_ip_f16pipe_bdma", 64, 128 * 129, 7, 4)]


@pytest.mark.parametrize("k,nq", [(10, 33), (100, 31)])
@pytest.mark.parametrize("variant,dim,n,blocks,early", TWO)
def test_early_tighten_main(probe, variant, dim, n, blocks, early, k, nq):
    bf16, l2 = VARIANTS[variant][:2]
    case = plain_case("near", n, dim, nq, k, l2, bf16, k == 100)
    print(variant, "->", probe.symbols(variant, True), "tiles %d blocks %d remainder %d" % ((n + 127) // 128, blocks, ((n + 127) // 128) % blocks))
    o = probe.chain(case, variant, stages=TWO_PASS, sample_rows=1024, blocks=blocks, early_tiles=early, cap=max(8192, 64 * k))
    check_sample_select(case, o, probe, k)
    kth = case.kth(k)
    bad = np.flatnonzero(o.qbound[:nq].astype(np.float64) > kth)
    assert len(bad) == 0, "query %d: the tightened bound %r is above the exact k-th best %r" % (bad[0], o.qbound[bad[0]], kth[bad[0]])
    assert (o.qbound[:nq] >= o.qbound_select[:nq]).all(), "tighten lowered a bound"
    rose = int((o.qbound[:nq] > o.qbound_select[:nq]).sum())
    print("tighten raised %d of %d bounds" % (rose, nq))
    assert rose > 0, "the tighten step raised no bound: its kernel did nothing"
    if k > o.groups:       # the selection had fewer than k group bounds (-inf): every bound comes from the early pass's survivors
        assert np.isneginf(o.qbound_select[:nq]).all() and np.isfinite(o.qbound[:nq]).all()
    sets = check_survivors(case, o, k)                       # union of both passes: a superset, and no row twice
    # the early pass's survivors are the head of every list and lie in the early tiles of their block
    n_tiles = (n + 127) // 128
    t_base, t_rem = divmod(n_tiles, blocks)
    first = [b * t_base + min(b, t_rem) for b in range(blocks + 1)]
    early_tile = np.zeros(n_tiles, bool)
    for b in range(blocks):
        early_tile[first[b]:min(first[b] + early, first[b + 1])] = True
    for q in range(nq):
        ce = int(o.cnt_early[q])
        assert ce <= o.cap and ce <= int(o.cnt[q])
        assert early_tile[sets[q][:ce] >> 7].all() and not early_tile[sets[q][ce:] >> 7].any(), "query %d: a survivor from the other pass's tiles" % q


@pytest.mark.parametrize("variant,dim,n,blocks,early", TWO)
def test_the_two_passes_partition_the_tiles(probe, variant, dim, n, blocks, early):
    """every row the same vector and no tighten step: every row survives, so the survivor rows are arange(n), each once"""
    bf16, l2 = VARIANTS[variant][:2]
    nq, k = 2, 10
    case = plain_case("same", n, dim, nq, k, l2, bf16, False)
    o = probe.chain(case, variant, stages=QPREP | SAMPLE | SELECT | EARLY | MAIN, sample_rows=128, blocks=blocks, early_tiles=early,
                    cap=n + 64, n_chunks=0)
    assert np.isneginf(o.qbound[:nq]).all()                  # k = 10 > 8 groups: no bound, the gate is open
    for q in range(nq):
        rows, _, stored = survivors(o, q)
        assert stored == int(o.cnt[q])
        assert np.array_equal(np.sort(rows), np.arange(n)), "query %d: %d survivors of %d rows; first missing %s, first twice %s" % (
            q, len(rows), n, np.setdiff1d(np.arange(n), rows)[:1], rows[np.flatnonzero(np.diff(np.sort(rows)) == 0)[:1]])
    assert not o.ovf.any()


# ---- the adversarial seeds, and independence from what the workspace held -----------------------------------------------------------
def read_state(o):
    """everything a later stage (re-rank, merge) or the host reads, in a comparable form; asserts that none of it is the fill"""
    nq = o.nq
    st = {"qcoef": o.qcoef.view(np.uint32).ravel(), "qwit": o.qwit.view(np.uint32), "qbound": o.qbound[:nq].view(np.uint32),
          "q16": o.q16.ravel().astype(np.uint32), "smax": o.smax[:, :o.groups].view(np.uint32).ravel(), "cand_cnt": o.cnt, "ovf_q": o.ovf,
          "spill_next": o.misc[:1], "redo_cnt": o.misc[1:2], "done_cnt": o.done, "rerank_cnt": o.rerank,
          "cnt_early": o.cnt_early, "qchunk_used": (o.qchunk != 0).astype(np.uint32).ravel(), "tile_norm": o.tile_norm, "norm_cap": o.stats[3:4]}
    if o.fill != 0:
        for name, a in st.items():
            if name in ("qchunk_used", "tile_norm", "norm_cap"):
                continue
            hit = np.flatnonzero((a == (o.fill & 0xFFFF)) | (a == (o.fill >> 16)) if name == "q16" else a == o.fill)
            assert len(hit) == 0, "%s[%d] still holds the fill %#x" % (name, hit[0], o.fill)
        hit = np.argwhere(o.qchunk == o.fill)
        assert len(hit) == 0 or o.fill == 0xFFFFFFFF and o.ovf[hit[0][0]], "qchunk[%d][%d] still holds the fill" % tuple(hit[0])
    sets = []
    for q in range(nq):
        rows, vals, _ = survivors(o, q)
        order = np.argsort(rows, kind="stable")
        sets.append((rows[order], vals[order].view(np.uint32)))
        if o.fill != 0:
            assert not (vals.view(np.uint32) == o.fill).any() and not (rows == o.fill).any(), "query %d: a stored survivor is the fill" % q
    return st, sets


def same_state(a, b, what):
    (sa, la), (sb, lb) = a, b
    for name in sa:
        d = np.flatnonzero(sa[name] != sb[name])
        assert len(d) == 0, "%s: %s[%d] = %#x / %#x" % (what, name, d[0], sa[name][d[0]], sb[name][d[0]])
    for q, ((ra, va), (rb, vb)) in enumerate(zip(la, lb)):
        assert np.array_equal(ra, rb), "%s: query %d has other survivors (%d / %d)" % (what, q, len(ra), len(rb))
        assert np.array_equal(va, vb), "%s: query %d, other scores for the same survivors" % (what, q)


@pytest.mark.parametrize("seed", BF16_SEEDS)
def test_adversarial_bf16_seeds_stage_by_stage_over_three_fills(probe, seed):
    """The product's configuration for these indexes (bf16 matrix cores, rows by DMA, 256 blocks, one pass), every stage checked,
    from three different workspaces."""
    case = seed_case(seed)
    k = case.k
    states = []
    for fill in FILLS:
        o = probe.chain(case, "bf16_ip_bfmma_dma", stages=ONE_PASS, fill=fill, sample_rows=product_sample_rows(k), blocks=256,
                        cap=max(8192, 64 * k))
        check_qprep(case, o, counters=False)
        assert not o.done.any() and not o.rerank.any() and int(o.misc[1]) == 0
        check_sample_select(case, o, probe, k)
        check_survivors(case, o, k)
        states.append(read_state(o))
    same_state(states[0], states[1], "fill 0 / 0xFFFFFFFF")
    same_state(states[0], states[2], "fill 0 / 0x7F7FFFFF")


@pytest.mark.parametrize("seed", BF16_SEEDS[::6])
@pytest.mark.parametrize("variant", ["bf16_ip_bfmma", "bf16_ip_bfmma_bdma", "bf16_ip_f16pipe"])
def test_adversarial_bf16_seeds_other_variants(probe, seed, variant):
    case = seed_case(seed)
    o = probe.chain(case, variant, stages=ONE_PASS, sample_rows=product_sample_rows(case.k), blocks=256, cap=max(8192, 64 * case.k))
    check_sample_select(case, o, probe, case.k)
    check_survivors(case, o, case.k)


@pytest.mark.parametrize("variant,dim,n,blocks,early", TWO[:8])
def test_two_pass_chain_does_not_depend_on_the_workspace(probe, variant, dim, n, blocks, early):
    bf16, l2 = VARIANTS[variant][:2]
    nq, k = 33, 10
    case = plain_case("near", n, dim, nq, k, l2, bf16, False)
    states = []
    for fill in FILLS:
        o = probe.chain(case, variant, stages=TWO_PASS, fill=fill, sample_rows=1024, blocks=blocks, early_tiles=early)
        states.append(read_state(o))
        assert (o.cnt_early <= o.cnt).all() and o.cnt_early.any()
    same_state(states[0], states[1], "fill 0 / 0xFFFFFFFF")
    same_state(states[0], states[2], "fill 0 / 0x7F7FFFFF")


def test_spilled_lists_do_not_depend_on_the_workspace(probe):
    n, dim, nq, k = 128 * 80 + 1, 64, 33, 1
    case = plain_case("same", n, dim, nq, k, 0, 0, False)
    states = []
    for fill in FILLS:
        o = probe.chain(case, "f32_ip_bdma", stages=ONE_PASS, fill=fill, cap=64, n_chunks=33 * 3, sample_rows=1024)
        states.append(read_state(o))
    same_state(states[0], states[1], "fill 0 / 0xFFFFFFFF")
    same_state(states[0], states[2], "fill 0 / 0x7F7FFFFF")


def test_a_tile_outside_f16_lets_every_pair_through(probe):
    """one +inf element: its tile's norm is +inf, all 128 rows of the tile survive for every open query, nothing else changes"""
    n, dim, nq, k = 128 * 40 + 1, 64, 33, 10
    base = plain_case("near", n, dim, nq, k, 0, 0, False)
    X = base.X.copy()
    X[128 * 17 + 5, 3] = np.inf
    case = Case(X, base.Q, 0, 0, k)
    for variant in ("f32_ip_bdma", "f32_ip_image"):
        o = probe.chain(case, variant, stages=ONE_PASS, sample_rows=1024)
        assert o.tile_norm[17] == INF_BITS and int(o.stats[2]) == 1
        for q in range(nq):
            rows, _, _ = survivors(o, q)
            assert np.isin(np.arange(128 * 17, 128 * 18), rows).all(), "query %d: a row of the tile outside f16 was dropped" % q
