#!/usr/bin/env python3
"""FLAT k > 1024: option flat-large-k = 1 (one row pass + device select, csrc/flat_large_k.hip), with the hand-back ordered by
the host and by the device (option flat-large-k-device-sort = 1), against option 0 (the paged path) on the same device in the
same process.

FLAT 400 000 x 256 f32 COSINE (the project's reduced shape), k 2 500 / 10 000 / 100 000, nq 1 / 16.  Per point the three legs
alternate, one untimed call behind every switch, five timed calls per leg; the medians, their ratios, the large-k counters and
whether the answers are byte-identical go out as one JSON line -- behind, per one-pass leg, how a call splits into device
stages (events around the launches), download and host finish (option kernel-timing, three calls outside the medians).  Every point runs in a child process of its
own under its own time limit; the driver stops at the first child that does not end cleanly.

  python scripts/flat_large_k_probe.py [--rows 400000] [--dim 256] [--out profiles/r16_flat_large_k_sort_probe.log]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
KS = (2500, 10000, 100000)
NQS = (1, 16)
REPS = 5


def point(rows, dim, k, nq):
    import numpy as np
    sys.path.insert(0, str(ROOT))
    import _pkg
    vsa = _pkg.vsa
    rng = np.random.default_rng(13)
    X = rng.standard_normal((rows, dim)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    ix = vsa.Index("FLAT", dim, "COSINE", initial_cap=rows, device_id=0)
    ix.add_batch(X)
    ix.flush()
    legs = {"paged": (0, 0), "one_pass": (1, 0), "device_sort": (1, 1)}      # (flat-large-k, flat-large-k-device-sort)

    def switch(leg):
        ix.set_option("flat-large-k", legs[leg][0])
        ix.set_option("flat-large-k-device-sort", legs[leg][1])
        return ix.search_batch(Q, k)                     # untimed: the first call behind the switch

    # where a call of the one-pass legs goes (kernel-timing = 1: the launches end before the download starts), three calls each
    split = {}
    for leg in ("one_pass", "device_sort"):
        switch(leg)
        ix.set_option("kernel-timing", 1)
        s0 = ix.large_k_sort_stats()
        for _ in range(3):
            ix.search_batch(Q, k)
        s1 = ix.large_k_sort_stats()
        ix.set_option("kernel-timing", 0)
        split[leg] = {f: round((getattr(s1, f + "_ns") - getattr(s0, f + "_ns")) / 3e6, 3) for f in ("device", "download", "finish")}
    times = {leg: [] for leg in legs}
    answers = {}
    for rep in range(REPS):
        for leg in legs:
            answers[leg] = switch(leg)
            t0 = time.perf_counter()
            ix.search_batch(Q, k)
            times[leg].append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
               for leg in ("one_pass", "device_sort") for a, b in zip(answers["paged"], answers[leg]))
    s, ss = ix.large_k_stats(), ix.large_k_sort_stats()
    med = {leg: statistics.median(t) for leg, t in times.items()}
    print(json.dumps({"rows": rows, "dim": dim, "metric": "COSINE", "k": k, "nq": nq, "paged_ms_median": round(med["paged"], 3),
                      "one_pass_ms_median": round(med["one_pass"], 3), "device_sort_ms_median": round(med["device_sort"], 3),
                      "speedup": round(med["paged"] / med["one_pass"], 2), "device_sort_over_one_pass": round(med["one_pass"] / med["device_sort"], 2),
                      "one_pass_split_ms": split["one_pass"], "device_sort_split_ms": split["device_sort"],
                      **{leg + "_ms": [round(t, 3) for t in ts] for leg, ts in times.items()}, "identical": bool(same),
                      "one_pass_queries": s.one_pass_queries, "fallback_queries": s.fallback_queries, "chunks": s.chunks, "row_passes": s.row_passes,
                      "sorted_queries": ss.sorted_queries, "merge_passes": ss.merge_passes}), flush=True)
    ix.close()
    return 0 if same else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=400000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r13_flat_large_k_probe.log"))
    ap.add_argument("--limit", type=int, default=150, help="seconds per point")
    ap.add_argument("--point", nargs=2, type=int, metavar=("K", "NQ"))
    a = ap.parse_args()
    if a.point:
        return point(a.rows, a.dim, a.point[0], a.point[1])
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        log.write("# scripts/flat_large_k_probe.py: paged / one pass (host sort) / one pass (device sort) alternating in one process, medians of %d\n" % REPS)
        for k in KS:
            for nq in NQS:
                try:
                    p = subprocess.run([sys.executable, __file__, "--rows", str(a.rows), "--dim", str(a.dim), "--point", str(k), str(nq)],
                                       capture_output=True, text=True, timeout=a.limit)
                except subprocess.TimeoutExpired:
                    log.write("# k=%d nq=%d: no answer within %d s -- stopped here\n" % (k, nq, a.limit))
                    return 2
                log.write(p.stdout)
                log.flush()
                sys.stdout.write(p.stdout)
                if p.returncode != 0:      # (a point that ended badly: nothing more is started on the device)
                    log.write("# k=%d nq=%d: exit status %d -- stopped here\n%s\n" % (k, nq, p.returncode, p.stderr[-2000:]))
                    return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
