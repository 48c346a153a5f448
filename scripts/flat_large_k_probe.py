#!/usr/bin/env python3
"""FLAT k > 1024: option flat-large-k = 1 (one row pass + device select, csrc/flat_large_k.hip) against option 0 (the paged
path) on the same device in the same process.

FLAT 400 000 x 256 f32 COSINE (the project's reduced shape), k 2 500 / 10 000 / 100 000, nq 1 / 16.  Per point the option
alternates 0 / 1, one untimed call behind every switch, five timed calls per setting; the medians, their ratio, the large-k
counters and whether the two answers are byte-identical go out as one JSON line.  Every point runs in a child process of its
own under its own time limit; the driver stops at the first child that does not end cleanly.

  python scripts/flat_large_k_probe.py [--rows 400000] [--dim 256] [--out profiles/r13_flat_large_k_probe.log]
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
    times = {0: [], 1: []}
    answers = {}
    for rep in range(REPS):
        for opt in (0, 1):
            ix.set_option("flat-large-k", opt)
            answers[opt] = ix.search_batch(Q, k)          # untimed: the first call behind the switch
            t0 = time.perf_counter()
            ix.search_batch(Q, k)
            times[opt].append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
               for a, b in zip(answers[0], answers[1]))
    s = ix.large_k_stats()
    m0, m1 = statistics.median(times[0]), statistics.median(times[1])
    print(json.dumps({"rows": rows, "dim": dim, "metric": "COSINE", "k": k, "nq": nq, "paged_ms_median": round(m0, 3),
                      "one_pass_ms_median": round(m1, 3), "speedup": round(m0 / m1, 2), "paged_ms": [round(t, 3) for t in times[0]],
                      "one_pass_ms": [round(t, 3) for t in times[1]], "identical": bool(same), "one_pass_queries": s.one_pass_queries,
                      "fallback_queries": s.fallback_queries, "chunks": s.chunks, "row_passes": s.row_passes}), flush=True)
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
        log.write("# scripts/flat_large_k_probe.py: option flat-large-k 0 (paged) / 1 (one pass) alternating in one process, medians of %d\n" % REPS)
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
