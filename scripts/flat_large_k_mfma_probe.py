#!/usr/bin/env python3
"""Timing probe of option flat-large-k-mfma: a chunk's dense distances from flat_dense_mfma_kernel (the matrix cores) against
flat_dense_distance_kernel (the vector ALUs), csrc/flat_large_k.hip, on one index in one process.

The index of the earlier large-k probes: FLAT 400 000 x 256 f32 COSINE, flat-large-k = 1 and flat-large-k-device-sort = 1,
k 2 500 / 10 000 / 100 000 at 16 / 64 / 256 queries; then one bf16 index of the same shape and one f32 index of stride 768 at
k 10 000.  Per point: every shape warmed up under both values, then the option alternating call by call, --reps whole calls per
value on the host clock (search_batch ends in a stream synchronise); median and extremes per value, how many option-1 calls were
slower than the option-0 median, and whether the answers are byte-identical.  Then, in a run of its own with kernel-timing =
1, three calls per value: the device time of a chunk (vk_flat_large_k_sort_stats.device_ns / timed_chunks: distances, select,
emit and sort between two events).

    python scripts/flat_large_k_mfma_probe.py [--rows N] [--reps R] > profiles/r19_flat_large_k_mfma_probe.log
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
OPT = "flat-large-k-mfma"


def chunk_ms(ix, call):
    ix.set_option("kernel-timing", 1)
    s0 = ix.large_k_sort_stats()
    for _ in range(3):
        call()
    s1 = ix.large_k_sort_stats()
    ix.set_option("kernel-timing", 0)
    return (s1.device_ns - s0.device_ns) / max(1, s1.timed_chunks - s0.timed_chunks) / 1e6


def index(rows, dim, dtype, ks, nqs, reps):
    rng = np.random.default_rng(13)
    ix = vsa.Index("FLAT", dim, "COSINE", initial_cap=rows, device_id=0, dtype=dtype)
    t0 = time.perf_counter()
    for lo in range(0, rows, 100_000):   # (in pieces: the host never holds more than 100 000 rows)
        x = rng.standard_normal((min(100_000, rows - lo), dim)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        ix.add_batch(x, np.arange(lo, lo + x.shape[0], dtype=np.uint64))
    ix.flush()
    ix.set_option("flat-large-k", 1)
    ix.set_option("flat-large-k-device-sort", 1)
    print(f"FLAT {rows} x {dim} {dtype} COSINE built in {time.perf_counter() - t0:.1f} s; flat-large-k = 1, flat-large-k-device-sort = 1, "
          f"{reps} whole calls per value", flush=True)
    ok = True
    for k in ks:
        for nq in nqs:
            Q = rng.standard_normal((nq, dim)).astype(np.float32)
            Q /= np.linalg.norm(Q, axis=1, keepdims=True)
            call = lambda: ix.search_batch(Q, k)
            times, answers = {0: [], 1: []}, {}
            for v in (0, 1):   # warm-up of this shape under both values
                ix.set_option(OPT, v)
                call()
            s0 = ix.large_k_mfma_stats()
            for _ in range(reps):
                for v in (0, 1):
                    ix.set_option(OPT, v)
                    t0 = time.perf_counter()
                    answers[v] = call()
                    times[v].append((time.perf_counter() - t0) * 1e3)
            s1 = ix.large_k_mfma_stats()
            dev = {}
            for v in (0, 1):
                ix.set_option(OPT, v)
                dev[v] = chunk_ms(ix, call)
            same = all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(answers[0], answers[1]))
            ok &= same
            med = {v: statistics.median(times[v]) for v in (0, 1)}
            print(f"k {k:>6} nq {nq:>3}: option 0 median {med[0]:9.3f} ms (min {min(times[0]):9.3f} max {max(times[0]):9.3f})  "
                  f"option 1 median {med[1]:9.3f} ms (min {min(times[1]):9.3f} max {max(times[1]):9.3f})  0 / 1 x{med[0] / med[1]:.2f}  "
                  f"option-1 calls slower than the option-0 median: {sum(t > med[0] for t in times[1])} of {reps}  "
                  f"chunk device time {dev[0]:.3f} -> {dev[1]:.3f} ms  launches {s1.launches - s0.launches} declined {s1.declined - s0.declined}  "
                  f"byte-identical: {'yes' if same else 'NO'}", flush=True)
    ix.set_option(OPT, 0)
    ix.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=400_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nqs", default="16,64,256")
    a = ap.parse_args()
    nqs = [int(v) for v in a.nqs.split(",")]
    ok = index(a.rows, 256, "f32", (2500, 10000, 100000), nqs, a.reps)
    ok &= index(a.rows, 256, "bf16", (10000,), nqs, a.reps)
    ok &= index(a.rows // 2, 768, "f32", (10000,), nqs, a.reps)
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
