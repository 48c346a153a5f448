"""256 pre-filter searches in one vk_index_search_labels_batch: label -> slot on the host (option prefilter-device-resolve = 0)
against the device label map (= 1), inside one process on one device lease.

    python scripts/prefilter_resolve_probe.py [--rows 400000] [--dim 256] [--reps 5] [--out profiles/r11_prefilter_resolve_probe.log]

A FLAT index (no graph to build) of rows x dim f32, COSINE, k = 10, 256 queries, 256 distinct key lists of 200, 2 000 and
20 000 keys -- what a batch collected from single callers looks like: one distinct list per member.  Per list length the option
alternates 0 and 1, --reps repetitions each (leases differ by a few percent, so nothing is compared across runs), and the
medians are compared; the map is resident during the timed repetitions (a read phase), and the time of ONE build at this size
is recorded on its own: the first batch after a write that published a label, minus the median batch.  Per list length the
reader pool's shape is timed too: 256 vk_index_search_labels calls from 16 threads against 256 vk_index_search_labels_submit
calls (coalescing 256 / 2 000 us) with the option 0 and 1 -- both through this binding's Python threads and callbacks, which
cost the two legs alike.  Every answer with the
option on is compared with the option off's (ids and distance bits); a mismatch ends the run.  Every measured step runs under
an alarm of its own that ends the process (a hung device call cannot be waited out), and the first failure stops the script.

By the project's rule the option ships 1 only if every point is above the option-off median; DESIGN section 8 has the figures."""
import argparse
import json
import signal
import statistics
import sys
import threading
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import _pkg  # noqa: E402

vsa = _pkg.vsa
STEP_LIMIT_S = 120
OPT = "prefilter-device-resolve"


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r11_prefilter_resolve_probe.log"))
    a = ap.parse_args()
    assert a.reps >= 5, "at least five repetitions per leg"
    N, D, K, NQ = a.rows, a.dim, 10, 256
    rng = np.random.default_rng(11)
    lines = []

    def say(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        lines.append(line)

    def save():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")

    def unit(n):
        x = rng.standard_normal((n, D), dtype=np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        return x

    g = vsa.Index("FLAT", D, "COSINE", initial_cap=N + 1)
    for lo in range(0, N, 100_000):
        limited(g.add_batch, unit(min(100_000, N - lo)), np.arange(lo, min(lo + 100_000, N), dtype=np.uint64))
    limited(g.flush)
    Q = unit(NQ)
    say({"index": {"algo": "FLAT", "rows": N, "dim": D, "metric": "COSINE", "dtype": "f32", "k": K, "queries": NQ, "lists": "distinct"}})

    def timed(labels, lb):
        t0 = time.perf_counter()
        out = limited(g.search_labels_batch, Q, K, labels, lb)
        return time.perf_counter() - t0, out

    for m in (N // 2000, 2000, 20000):
        lists = [rng.choice(N, size=m, replace=False).astype(np.uint64) for _ in range(NQ)]
        labels = np.concatenate(lists)
        lb = np.arange(NQ + 1, dtype=np.uint64) * np.uint64(m)
        # warm both legs (scratch buffers grow once, the map is built), and compare every answer
        g.set_option(OPT, 0)
        _, ref = timed(labels, lb)
        g.set_option(OPT, 1)
        s0 = g.prefilter_stats()
        _, got = timed(labels, lb)
        s1 = g.prefilter_stats()
        if any(x.tobytes() != y.tobytes() for x, y in zip(ref, got)) or s1.device_resolved_keys - s0.device_resolved_keys != labels.size:
            say({"keys": m, "mismatch": True, "device_resolved_keys": int(s1.device_resolved_keys - s0.device_resolved_keys)})
            save()
            sys.exit(1)
        t_off, t_on = [], []
        for _ in range(a.reps):       # both legs alike: one untimed batch behind the switch, then the timed one
            g.set_option(OPT, 0)      # (releases the map: the untimed batch of the other leg builds it again)
            timed(labels, lb)
            t_off.append(timed(labels, lb)[0])
            g.set_option(OPT, 1)
            timed(labels, lb)
            t_on.append(timed(labels, lb)[0])
        off, on = statistics.median(t_off), statistics.median(t_on)
        say({"keys": m, "host_resolve_ms": round(off * 1e3, 3), "device_resolve_ms": round(on * 1e3, 3), "ratio": round(off / on, 2),
             "host_all_ms": [round(t * 1e3, 3) for t in t_off], "device_all_ms": [round(t * 1e3, 3) for t in t_on], "answers_equal": True,
             "label_map_bytes": int(g.prefilter_stats().label_map_bytes)})
        # the reader pool's shape: 256 single calls from 16 threads against 256 submissions collected by the dispatcher
        def single_calls():
            def work(t):
                for q in range(t, NQ, 16):
                    g.search_labels(Q[q], K, lists[q])
            ts = [threading.Thread(target=work, args=(t,)) for t in range(16)]
            t0 = time.perf_counter()
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            return time.perf_counter() - t0

        def submissions():
            done = threading.Semaphore(0)
            t0 = time.perf_counter()
            hs = [g.submit_labels(Q[q], K, lists[q], lambda s: done.release()) for q in range(NQ)]
            for _ in hs:
                assert done.acquire(timeout=STEP_LIMIT_S)
            dt = time.perf_counter() - t0
            return dt, hs

        ref_single = [g.search_labels(Q[q], K, lists[q]) for q in range(NQ)]
        point = {"keys": m, "reader_pool": True}
        t_single = []
        for option in (0, 1):
            g.set_option(OPT, option)
            g.set_coalescing(NQ, 2000)
            _, hs = limited(submissions)
            for q, h in enumerate(hs):
                d, l = h.result()
                if h.status != 0 or l.tolist() != ref_single[q][1].tolist() or d.view(np.uint32).tolist() != ref_single[q][0].view(np.uint32).tolist():
                    say({"keys": m, "submit_mismatch_at_query": q, "option": option})
                    save()
                    sys.exit(1)
            t_sub = []
            for _ in range(a.reps):
                if option == 0:
                    t_single.append(limited(single_calls))
                t_sub.append(limited(submissions)[0])
            g.set_coalescing(0, 0)
            point["submit_ms_option_%d" % option] = round(statistics.median(t_sub) * 1e3, 3)
            point["submit_all_ms_option_%d" % option] = [round(t * 1e3, 3) for t in t_sub]
        point["single_calls_16_threads_ms"] = round(statistics.median(t_single) * 1e3, 3)
        point["single_all_ms"] = [round(t * 1e3, 3) for t in t_single]
        point["ratio_single_over_submit_option_0"] = round(point["single_calls_16_threads_ms"] / point["submit_ms_option_0"], 2)
        point["ratio_single_over_submit_option_1"] = round(point["single_calls_16_threads_ms"] / point["submit_ms_option_1"], 2)
        point["ratio_submit_option_0_over_1"] = round(point["submit_ms_option_0"] / point["submit_ms_option_1"], 2)
        point["answers_equal"] = True
        say(point)
    # one build at this size: the first batch behind a write that published a label, against the batch behind it
    g.set_option(OPT, 1)
    lists = [rng.choice(N, size=200, replace=False).astype(np.uint64) for _ in range(NQ)]
    labels, lb = np.concatenate(lists), np.arange(NQ + 1, dtype=np.uint64) * np.uint64(200)
    timed(labels, lb)
    firsts, seconds = [], []
    for r in range(a.reps):
        limited(g.add, N, unit(1)[0])          # an update in place after the first round: a label is published, the count stays
        limited(g.flush)
        b0 = g.prefilter_stats().label_map_builds
        firsts.append(timed(labels, lb)[0])
        assert g.prefilter_stats().label_map_builds == b0 + 1
        seconds.append(timed(labels, lb)[0])
    say({"map_build": {"rows": N + 1, "first_batch_ms": round(statistics.median(firsts) * 1e3, 3),
                       "next_batch_ms": round(statistics.median(seconds) * 1e3, 3),
                       "build_ms": round((statistics.median(firsts) - statistics.median(seconds)) * 1e3, 3),
                       "label_map_bytes": int(g.prefilter_stats().label_map_bytes)}})
    save()


if __name__ == "__main__":
    main()
