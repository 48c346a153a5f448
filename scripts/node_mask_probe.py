"""A/B of the option hnsw-node-mask on the shapes of bench.py's config4_hnsw_tag leg, inside ONE process on one device lease.

    python scripts/node_mask_probe.py [--rows 1250000] [--dim 768] [--reps 5] [--out profiles/r08_node_mask_probe.log]

One HNSW graph (COSINE, M = 16, efConstruction = 200), k = 10, ef = 256, TAG filters of 10 % selectivity as device filter
handles.  Measured points, each with the option alternating 0 / 1 (--reps repetitions each, medians compared; leases differ by
2-6 %, so nothing here is compared across runs):
  shared_tags         4096 queries over 16 cached handles (the masks are built once, then hit)
  distinct_per_query  1024 queries, each with a handle nobody shares, NEW every step (tag_a OR tag_b combined on the device
                      inside the step, as bench.py does): every step builds 1024 masks in one launch
  tombstones_only     4096 unfiltered queries, 1 % of the rows deleted (the live bitmap against the strided tombstone word)
Printed per point and option: QPS, useful bytes over the HBM peak (evals x (row + 4) + hops x 132 B, like bench.py), and for
option 1 the time of the mask launch per batch (the step's first repetition after a release of the masks minus the median
warm step, where the masks are cached; for distinct_per_query the masks are rebuilt in every step, so the figure is the step's
difference to option 0).  The last line is the gate: `default_on_supported` is true only if no point's option-1 median is
below its option-0 median."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _pkg  # noqa: E402

vsa = _pkg.vsa
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_250_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r08_node_mask_probe.log"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least five repetitions per option"
    N, D, K, EF, T = a.rows, a.dim, 10, 256, 16
    rng = np.random.default_rng(8)
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def rows_block(n):
        x = rng.standard_normal((n, D), dtype=np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        return x

    t0 = time.perf_counter()
    h = vsa.Index("HNSW", D, "COSINE", initial_cap=N, m=16, ef_construction=200, ef_runtime=EF)
    for lo in range(0, N, 250_000):
        h.add_batch(rows_block(min(250_000, N - lo)), np.arange(lo, min(lo + 250_000, N), dtype=np.uint64))
    h.flush()
    say({"graph": {"rows": N, "dim": D, "M": 16, "ef": EF, "k": K, "build_s": round(time.perf_counter() - t0, 1)}})
    Q = rows_block(4096)
    tags = [h.make_filter(N, labels=np.flatnonzero(np.random.default_rng(4000 + t).random(N) < 0.1).astype(np.uint64)) for t in range(T)]
    shared = [tags[i % T] for i in range(4096)]
    nd = 1024
    pairs = [(i % T, (i // T + 1 + i) % T) for i in range(nd)]
    pairs = [(x, y if y != x else (y + 1) % T) for x, y in pairs]

    def step_shared():
        h.search_batch_filter_handles(Q, K, shared, ef=EF)
        return 4096

    def step_distinct():
        fl = h.combine_filters_batch([(tags[x], tags[y]) for x, y in pairs], "or")
        h.search_batch_filter_handles(Q[:nd], K, fl, ef=EF)
        return nd

    def step_plain():
        h.search_batch(Q, K, ef=EF)
        return 4096

    def timed(step):
        st0 = h.stats()
        t = time.perf_counter()
        n = step()
        dt = time.perf_counter() - t
        st1 = h.stats()
        useful = (st1.total_n_eval - st0.total_n_eval) * (D * 4 + 4) + (st1.total_n_hops - st0.total_n_hops) * 132
        return n / dt, useful / dt / 1e9 / HBM_PEAK_GBS, dt

    def point(name, step):
        res = {0: [], 1: []}
        first_on = []
        step()                                                   # warm-up: contexts, scratch
        for _ in range(a.reps):
            for opt in (0, 1):                                   # 0 releases the masks: the first step of every 1-run builds them
                h.set_option("hnsw-node-mask", opt)
                if opt == 1:
                    first_on.append(timed(step)[2])
                res[opt].append(timed(step))
        med = {o: (statistics.median(r[0] for r in res[o]), statistics.median(r[1] for r in res[o]), statistics.median(r[2] for r in res[o])) for o in res}
        ms = h.node_mask_stats()
        if name == "distinct_per_query":
            mask_ms = (med[1][2] - med[0][2]) * 1e3
        else:
            mask_ms = (statistics.median(first_on) - med[1][2]) * 1e3
        say({"point": name, "reps": a.reps,
             "off": {"qps": round(med[0][0], 1), "frac_of_hbm_peak": round(med[0][1], 4)},
             "on": {"qps": round(med[1][0], 1), "frac_of_hbm_peak": round(med[1][1], 4), "mask_launch_ms_per_batch": round(mask_ms, 3),
                    "masks_built": ms.masks_built, "cache_hits": ms.cache_hits, "served_last_batch": ms.last_batch_served},
             "on_over_off": round(med[1][0] / med[0][0], 4)})
        return med[1][0] >= med[0][0]

    ok = [point("shared_tags", step_shared), point("distinct_per_query", step_distinct)]
    dead = rng.choice(N, N // 100, replace=False)
    for lab in dead:
        h.remove(int(lab))
    h.flush()
    ok.append(point("tombstones_only", step_plain))
    say({"default_on_supported": all(ok)})
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
