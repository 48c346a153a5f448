#!/usr/bin/env python3
"""Timing probe of option flat-l2-gemm: L2 batches the candidate filter does not take, answered by flat_l2_gemm_kernel (K4e,
csrc/flat_l2_gemm.hip: a matrix-core bound, exact distances for the pairs it leaves) against the scan kernel (K3), on one index
per shape in one process.

f32: 100 000 x 128 (BASELINE config 1's shape), 200 000 x 768 and 20 000 x 768 at 16 / 64 / 256 queries, k = 10; 200 000 x 768 with
flat-filter = 0 at k = 100; bf16: 200 000 x 768.  Per point: the shape warmed up under both values, then the option alternating
call by call, --reps whole calls per value on the host clock (search_batch ends in a stream synchronise); median and extremes
per value, how many option-1 calls were slower than the option-0 median, the share of (row, query) pairs that got an exact
distance, and whether the answers are byte-identical.

    python scripts/flat_l2_gemm_probe.py [--reps R] > profiles/r20_flat_l2_gemm_probe.log
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import _pkg  # noqa: E402

vsa = _pkg.vsa
OPT = "flat-l2-gemm"


def index(rows, dim, dtype, k, nqs, reps, options=()):
    rng = np.random.default_rng(20)
    ix = vsa.Index("FLAT", dim, "L2", initial_cap=rows, device_id=0, dtype=dtype)
    t0 = time.perf_counter()
    for lo in range(0, rows, 100_000):   # (in pieces: the host never holds more than 100 000 rows)
        ix.add_batch(rng.standard_normal((min(100_000, rows - lo), dim)).astype(np.float32), np.arange(lo, min(rows, lo + 100_000), dtype=np.uint64))
    ix.flush()
    for name, v in options:
        ix.set_option(name, v)
    print(f"FLAT {rows} x {dim} {dtype} L2 built in {time.perf_counter() - t0:.1f} s; k = {k}; {dict(options)}; {reps} whole calls per value", flush=True)
    ok = True
    for nq in nqs:
        Q = rng.standard_normal((nq, dim)).astype(np.float32)
        times, answers = {0: [], 1: []}, {}
        for v in (0, 1):   # warm-up of this shape under both values
            ix.set_option(OPT, v)
            ix.search_batch(Q, k)
        s0 = ix.l2_gemm_stats()
        for _ in range(reps):
            for v in (0, 1):
                ix.set_option(OPT, v)
                t0 = time.perf_counter()
                answers[v] = ix.search_batch(Q, k)
                times[v].append((time.perf_counter() - t0) * 1e3)
        s1 = ix.l2_gemm_stats()
        same = all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(answers[0], answers[1]))
        ok &= same
        med = {v: statistics.median(times[v]) for v in (0, 1)}
        pairs = max(1, s1.rows - s0.rows) * nq
        print(f"nq {nq:>3}: option 0 median {med[0]:9.3f} ms (min {min(times[0]):9.3f} max {max(times[0]):9.3f})  "
              f"option 1 median {med[1]:9.3f} ms (min {min(times[1]):9.3f} max {max(times[1]):9.3f})  0 / 1 x{med[0] / med[1]:.2f}  "
              f"option-1 calls slower than the option-0 median: {sum(t > med[0] for t in times[1])} of {reps}  "
              f"evaluated / (rows x queries) {(s1.evaluated - s0.evaluated) / pairs:.5f}  launches {s1.launches - s0.launches} "
              f"declined {s1.declined - s0.declined}  byte-identical: {'yes' if same else 'NO'}", flush=True)
    ix.set_option(OPT, 0)
    ix.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nqs", default="16,64,256")
    a = ap.parse_args()
    nqs = [int(v) for v in a.nqs.split(",")]
    ok = index(100_000, 128, "f32", 10, nqs, a.reps)
    ok &= index(200_000, 768, "f32", 10, nqs, a.reps)
    ok &= index(20_000, 768, "f32", 10, nqs, a.reps)
    ok &= index(200_000, 768, "f32", 100, nqs, a.reps, (("flat-filter", 0),))
    ok &= index(200_000, 768, "bf16", 10, nqs, a.reps)
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
