"""256 pre-filter searches: 256 calls of search_labels against ONE search_labels_batch, inside one process on one device lease.

    python scripts/prefilter_batch_probe.py [--rows 400000] [--dim 256] [--reps 5] [--out profiles/r09_prefilter_batch_probe.log]

A FLAT index (no graph to build) of rows x dim f32, COSINE, k = 10, 256 queries; key lists of 200 (= rows / 2000, the ratio of
bench.py's pre_filter leg), 2 000 and 20 000 keys, each length once as ONE list shared by all queries and once as 256 distinct
lists.  Per case the two legs alternate, --reps repetitions each (leases differ by a few percent, so nothing is compared
across runs), and the medians are compared:
  single  256 calls of vk_index_search_labels -- the per-query path, which this build leaves as it was
  batch   one vk_index_search_labels_batch
Every answer of the batch leg is compared with the single leg's (ids and distance bits); a mismatch ends the run.  Every
measured step runs under an alarm of its own that ends the process (a hung device call cannot be waited out), and the first
failure stops the script."""
import argparse
import json
import signal
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _pkg  # noqa: E402

vsa = _pkg.vsa
STEP_LIMIT_S = 120


def limited(fn, *a):
    """one GPU step under its own time limit: SIGALRM's default action ends the process, inside a native call too"""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(STEP_LIMIT_S)
    try:
        return fn(*a)
    finally:
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=400_000)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r09_prefilter_batch_probe.log"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least five repetitions per leg"
    N, D, K, NQ = a.rows, a.dim, 10, 256
    rng = np.random.default_rng(9)
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def unit(n):
        x = rng.standard_normal((n, D), dtype=np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        return x

    g = vsa.Index("FLAT", D, "COSINE", initial_cap=N)
    for lo in range(0, N, 100_000):
        limited(g.add_batch, unit(min(100_000, N - lo)), np.arange(lo, min(lo + 100_000, N), dtype=np.uint64))
    limited(g.flush)
    Q = unit(NQ)
    say({"index": {"algo": "FLAT", "rows": N, "dim": D, "metric": "COSINE", "dtype": "f32", "k": K, "queries": NQ}})

    def single(lists):
        out = []
        for q in range(NQ):
            out.append(g.search_labels(Q[q], K, lists[q]))
        return out

    for m in (N // 2000, 2000, 20000):
        for mode in ("shared", "distinct"):
            if mode == "shared":
                one = rng.choice(N, size=m, replace=False).astype(np.uint64)
                lists, labels, lb = [one] * NQ, one, None
            else:
                lists = [rng.choice(N, size=m, replace=False).astype(np.uint64) for _ in range(NQ)]
                labels = np.concatenate(lists)
                lb = np.arange(NQ + 1, dtype=np.uint64) * np.uint64(m)
            # warm both legs (scratch buffers grow once), and check every answer of the batch against the single calls
            ref = limited(single, lists)
            before = g.prefilter_stats()
            Db, Lb, Nb = limited(g.search_labels_batch, Q, K, labels, lb)
            for q in range(NQ):
                n = int(Nb[q])
                if Lb[q, :n].tolist() != ref[q][1].tolist() or Db[q, :n].view(np.uint32).tolist() != ref[q][0].view(np.uint32).tolist():
                    say({"keys": m, "lists": mode, "mismatch_at_query": q})
                    Path(a.out).write_text("\n".join(lines) + "\n")
                    sys.exit(1)
            after = g.prefilter_stats()
            ts, tb = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                limited(single, lists)
                ts.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                limited(g.search_labels_batch, Q, K, labels, lb)
                tb.append(time.perf_counter() - t0)
            s_med, b_med = statistics.median(ts), statistics.median(tb)
            say({"keys": m, "lists": mode, "single_ms": round(s_med * 1e3, 3), "batch_ms": round(b_med * 1e3, 3),
                 "single_qps": round(NQ / s_med), "batch_qps": round(NQ / b_med), "ratio": round(s_med / b_med, 2),
                 "single_all_ms": [round(t * 1e3, 3) for t in ts], "batch_all_ms": [round(t * 1e3, 3) for t in tb],
                 "answers_equal": True, "fallback_queries": int(after.fallback_queries - before.fallback_queries),
                 "candidates": int(after.candidates - before.candidates)})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
