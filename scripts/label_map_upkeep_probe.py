#!/usr/bin/env python3
"""The device label map behind a write phase: option prefilter-label-map-upkeep = 1 (the touched labels applied on the device,
label_map_apply_kernel) against option 0 (the map rebuilt from every published label) on the same index in the same process.

FLAT f32 L2, rows x 64 (the map's cost does not depend on the dimension).  50 write phases of 100 adds plus 100 removes; behind
each a flush (untimed), then one vk_index_search_labels_batch (16 queries, one shared list of 2 000 keys, prefilter-device-resolve
1) -- the batch that meets the new publication and pays for the map -- and one vk_index_search_filter_exact_batch over a filter
of the same keys, which finds the map current.  The option alternates phase by phase; the first five phases are discarded.  Per
size one JSON line: the median, the extremes and the deciles of the first batch under either option, the second batch's
medians, and the label map's counters.  Every size runs in a child process of its own under its own time limit; the driver
stops at the first child that does not end cleanly.

  python scripts/label_map_upkeep_probe.py [--rows 1000000 10000000] [--out profiles/r15_label_map_upkeep_probe.log]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
DIM, K, NQ, KEYS = 64, 10, 16, 2000
PHASES, DISCARD, ADDS, REMOVES = 50, 5, 100, 100


def summary(ms):
    ms = sorted(ms)
    return {"median": round(statistics.median(ms), 3), "min": round(ms[0], 3), "p10": round(ms[len(ms) // 10], 3),
            "p90": round(ms[len(ms) * 9 // 10], 3), "max": round(ms[-1], 3), "n": len(ms)}


def point(rows):
    import numpy as np
    sys.path.insert(0, str(ROOT))
    import _pkg
    vsa = _pkg.vsa
    rng = np.random.default_rng(15)
    ix = vsa.Index("FLAT", DIM, "L2", initial_cap=rows + PHASES * ADDS, device_id=0)
    step = 1 << 20
    for at in range(0, rows, step):      # (in pieces: the host never holds more than 256 MiB of rows)
        n = min(step, rows - at)
        ix.add_batch(rng.standard_normal((n, DIM)).astype(np.float32), np.arange(at, at + n, dtype=np.uint64))
    ix.flush()
    ix.set_option("prefilter-device-resolve", 1)
    Q = rng.standard_normal((NQ, DIM)).astype(np.float32)
    live = np.ones(rows + PHASES * ADDS, bool)
    live[rows:] = False
    nxt = rows
    first = {0: [], 1: []}
    second = {0: [], 1: []}
    ix.search_labels_batch(Q, K, np.arange(KEYS, dtype=np.uint64))      # the first build, untimed
    for ph in range(PHASES):
        opt = ph & 1
        ix.set_option("prefilter-label-map-upkeep", opt)
        ix.add_batch(rng.standard_normal((ADDS, DIM)).astype(np.float32), np.arange(nxt, nxt + ADDS, dtype=np.uint64))
        live[nxt:nxt + ADDS] = True
        nxt += ADDS
        for l in rng.choice(np.nonzero(live)[0], size=REMOVES, replace=False):
            ix.remove(int(l))
            live[l] = False
        ix.flush()
        keys = rng.choice(nxt, size=KEYS, replace=False).astype(np.uint64)      # (some of them removed by now: unknown keys)
        f = ix.make_filter(nxt, keys)
        t0 = time.perf_counter()
        ix.search_labels_batch(Q, K, keys)
        t1 = time.perf_counter()
        ix.search_filter_exact_batch(Q, K, f)
        t2 = time.perf_counter()
        if ph >= DISCARD:
            first[opt].append((t1 - t0) * 1e3)
            second[opt].append((t2 - t1) * 1e3)
    s = ix.label_map_stats()
    a, b = summary(first[0]), summary(first[1])
    print(json.dumps({"rows": rows, "dim": DIM, "phases": PHASES, "discarded": DISCARD, "adds": ADDS, "removes": REMOVES, "nq": NQ, "keys": KEYS,
                      "first_batch_ms_upkeep0": a, "first_batch_ms_upkeep1": b, "speedup_median": round(a["median"] / b["median"], 2),
                      "second_batch_ms_median_upkeep0": round(statistics.median(second[0]), 3),
                      "second_batch_ms_median_upkeep1": round(statistics.median(second[1]), 3),
                      "builds": s.builds, "delta_batches": s.delta_batches, "delta_records": s.delta_records, "claimed": s.claimed,
                      "killed": s.killed, "moved": s.moved, "dead_entries": s.dead_entries, "used_entries": s.used_entries,
                      "capacity": s.capacity, "delta_mismatches": s.delta_mismatches, "rebuilds_forced": s.rebuilds_forced}), flush=True)
    ix.close()
    return 0 if s.delta_mismatches == 0 else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1000000])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r15_label_map_upkeep_probe.log"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per size")
    ap.add_argument("--point", type=int, metavar="ROWS")
    a = ap.parse_args()
    if a.point:
        return point(a.point)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        log.write("# scripts/label_map_upkeep_probe.py: option prefilter-label-map-upkeep 0 (rebuild) / 1 (apply) alternating phase by phase "
                  "in one process; the first batch behind each flush, ms\n")
        for rows in a.rows:
            try:
                p = subprocess.run([sys.executable, __file__, "--point", str(rows)], capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                log.write("# rows=%d: no answer within %d s -- stopped here\n" % (rows, a.limit))
                return 2
            log.write(p.stdout)
            log.flush()
            sys.stdout.write(p.stdout)
            if p.returncode != 0:      # (a size that ended badly: nothing more is started on the device)
                log.write("# rows=%d: exit status %d -- stopped here\n%s\n" % (rows, p.returncode, p.stderr[-2000:]))
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
