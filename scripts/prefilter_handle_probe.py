"""Timing probe of the exact kNN from a filter handle (vk_index_search_filter_exact_batch) against the list path
(vk_index_search_labels_batch over the same keys as a shared host list, with prefilter-device-resolve 0 and 1).

FLAT and HNSW, 400 000 x 256 f32 COSINE, k = 10, 256 queries, one shared filter admitting 200 / 2 000 / 20 000 / 200 000 labels
out of nbits = 400 000 and out of nbits = 10 000 000.  The legs alternate in one process, one untimed call follows every
switch, medians of five repetitions, answers compared byte for byte.  The handle leg's expansion share is timed apart through
vk_filter_read_labels with cap 0 (the count and scan launches, which read every word of the bitmap; no emit, no download).

    python scripts/prefilter_handle_probe.py [--rows N] [--kinds FLAT,HNSW] > profiles/r12_prefilter_handle_probe.log
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


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=400_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--kinds", default="FLAT,HNSW")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((a.rows, a.dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    Q = rng.standard_normal((a.nq, a.dim)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    k = 10
    for kind in a.kinds.split(","):
        kw = dict(m=16, ef_construction=100) if kind == "HNSW" else {}
        g = vsa.Index(kind, a.dim, "COSINE", initial_cap=a.rows, device_id=0, **kw)
        t, _ = timed(lambda: g.add_batch(x))
        print(f"{kind}: {a.rows} x {a.dim} f32 COSINE built in {t / 1e3:.1f} s", flush=True)
        for nbits in (a.rows, 10_000_000):
            for admitted in (200, 2_000, 20_000, 200_000):
                if admitted > a.rows:
                    continue
                keys = np.sort(rng.choice(a.rows, size=admitted, replace=False)).astype(np.uint64)
                f = g.make_filter(nbits, labels=keys)
                assert f.read_labels().tolist() == keys.tolist()
                legs = {
                    "handle": lambda: g.search_filter_exact_batch(Q, k, f),
                    "list, host resolve": lambda: (g.set_option("prefilter-device-resolve", 0), g.search_labels_batch(Q, k, keys))[1],
                    "list, device resolve": lambda: (g.set_option("prefilter-device-resolve", 1), g.search_labels_batch(Q, k, keys))[1],
                    "expansion alone": lambda: f.read_labels(cap=0),
                }
                times = {n: [] for n in legs}
                answers = {}
                for _ in range(a.reps):
                    for name, fn in legs.items():
                        fn()                                   # one untimed call behind every switch
                        t, out = timed(fn)
                        times[name].append(t)
                        answers[name] = out
                ref = answers["handle"]
                for name in ("list, host resolve", "list, device resolve"):
                    assert all(u.tobytes() == v.tobytes() for u, v in zip(ref, answers[name])), name
                med = {n: statistics.median(v) for n, v in times.items()}
                s = g.filter_exact_stats()
                print(f"  nbits {nbits:>10} admitted {admitted:>7}: " + "  ".join(f"{n} {m:.3f} ms" for n, m in med.items()) +
                      f"  | handle / best list x{min(med['list, host resolve'], med['list, device resolve']) / med['handle']:.2f}"
                      f"  expansion share {med['expansion alone'] / med['handle']:.2f}  fallback_queries {s.fallback_queries}", flush=True)
                f.release()
        g.set_option("prefilter-device-resolve", 0)


if __name__ == "__main__":
    main()
