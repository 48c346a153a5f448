"""Timing probe of option prefilter-shared-mfma: a shared list's distances from K8m (prefilter_mfma_kernel) against K8b.

One FLAT f32 COSINE index of --rows x 768, k = 10.  Shared lists of 20 000 / 200 000 / 1 000 000 labels, 8 / 32 / 256 queries;
two legs per size: vk_index_search_labels_batch over the list, vk_index_search_filter_exact_batch over one handle admitting the
same labels.  Option 0 and 1 alternate in one process; every shape is warmed up under both values; medians and extremes of
--reps timed repetitions each; the answers of the two values are compared byte for byte at every timed size.  The calls are
timed whole (resolve, upload, distances, select, download, heap): the distance kernel is one part of them.

    python scripts/prefilter_mfma_probe.py [--rows N] [--reps R] > profiles/r18_prefilter_mfma_probe.log
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
OPT = "prefilter-shared-mfma"


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=24)
    ap.add_argument("--lists", default="20000,200000,1000000")
    ap.add_argument("--nqs", default="8,32,256")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    g = vsa.Index("FLAT", a.dim, "COSINE", initial_cap=a.rows, device_id=0)
    t0 = time.perf_counter()
    for lo in range(0, a.rows, 100_000):   # (in pieces: the host never holds more than 100 000 rows)
        x = rng.standard_normal((min(100_000, a.rows - lo), a.dim)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        g.add_batch(x, np.arange(lo, lo + x.shape[0], dtype=np.uint64))
    print(f"FLAT {a.rows} x {a.dim} f32 COSINE built in {time.perf_counter() - t0:.1f} s; k = 10, {a.reps} repetitions per leg and value", flush=True)
    k = 10
    for m in (int(v) for v in a.lists.split(",")):
        if m > a.rows:
            print(f"list {m:>8}: not timed (more labels than rows)")
            continue
        keys = np.sort(rng.choice(a.rows, size=m, replace=False)).astype(np.uint64)
        f = g.make_filter(a.rows, labels=keys)
        for nq in (int(v) for v in a.nqs.split(",")):
            Q = rng.standard_normal((nq, a.dim)).astype(np.float32)
            Q /= np.linalg.norm(Q, axis=1, keepdims=True)
            legs = {"labels_batch": lambda: g.search_labels_batch(Q, k, keys), "filter_exact_batch": lambda: g.search_filter_exact_batch(Q, k, f)}
            for name, fn in legs.items():
                times, answers = {0: [], 1: []}, {}
                for v in (0, 1):   # warm-up of this shape under both values
                    g.set_option(OPT, v)
                    fn()
                s0 = g.prefilter_mfma_stats()
                for _ in range(a.reps):
                    for v in (0, 1):
                        g.set_option(OPT, v)
                        t, answers[v] = timed(fn)
                        times[v].append(t)
                s1 = g.prefilter_mfma_stats()
                same = all(u.tobytes() == w.tobytes() for u, w in zip(answers[0], answers[1]))
                med = {v: statistics.median(times[v]) for v in (0, 1)}
                print(f"list {m:>8} nq {nq:>4} {name:<19}: option 0 median {med[0]:9.3f} ms (min {min(times[0]):9.3f} max {max(times[0]):9.3f})  "
                      f"option 1 median {med[1]:9.3f} ms (min {min(times[1]):9.3f} max {max(times[1]):9.3f})  0 / 1 x{med[0] / med[1]:.2f}  "
                      f"K8m launches {s1.launches - s0.launches}  byte-identical: {'yes' if same else 'NO'}", flush=True)
        f.release()
    g.set_option(OPT, 0)


if __name__ == "__main__":
    main()
