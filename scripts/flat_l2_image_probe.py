#!/usr/bin/env python3
"""FLAT f32 L2 batch search: option flat-l2-image = 1 (early and main pass over the resident f16 image of the rows, half norms
staged by the DMA producers; csrc/flat_filter.hip) against option 0 (the f32 rows through registers) on one index, in one
process.

f32 L2, un-normalised rows from a rank-32 latent model (norms over a decade), 256-query batches, k = 10, through
vk_index_search_batch_device on a stream of its own.  The two legs alternate in rounds; behind every switch one untimed call
(with option 1 it builds the image, with option 0 it releases it), then timed steps, each between two device events.  Per leg:
median, minimum and maximum of all timed steps (at least 20), the image bytes the last batch read, its survivor count, and whether
both legs answered byte for byte alike -- one JSON line per size.  Every size runs in a child process of its own under its own
time limit; the driver stops at the first child that does not end cleanly.

  python scripts/flat_l2_image_probe.py [--rows 1250000 ...] [--dim 768] [--out profiles/r17_flat_l2_image_probe.log]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BATCH, K, ROUNDS, STEPS = 256, 10, 4, 6                      # 4 x 6 = 24 timed steps per leg


def point(rows, dim):
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import _pkg
    vsa = _pkg.vsa
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    A = torch.randn(dim, 32, generator=g, device=dev)

    def make(n):
        x = torch.randn(n, 32, generator=g, device=dev) @ A.T + 0.05 * torch.randn(n, dim, generator=g, device=dev)
        x = torch.nn.functional.normalize(x, dim=1)
        return x * torch.exp(torch.empty(n, 1, device=dev).uniform_(-1.15, 1.15, generator=g))      # norms 0.32 .. 3.2

    ix = vsa.Index("FLAT", dim, "L2", initial_cap=rows, device_id=0)
    for lo in range(0, rows, 1 << 17):
        n = min(1 << 17, rows - lo)
        ix.add_batch(make(n).cpu().numpy(), np.arange(lo, lo + n, dtype=np.uint64))
    ix.flush()
    Q = make(BATCH).contiguous()
    Qh = Q.cpu().numpy()
    od = torch.empty(BATCH, K, device=dev, dtype=torch.float32)
    ol = torch.empty(BATCH, K, device=dev, dtype=torch.int64)
    on = torch.empty(BATCH, device=dev, dtype=torch.int32)
    stream = torch.cuda.Stream(device=dev)                   # (default priority)

    def step():
        ix.search_batch_device(Q.data_ptr(), BATCH, K, od.data_ptr(), ol.data_ptr(), on.data_ptr(), stream=stream.cuda_stream)

    times, info, answers = {0: [], 1: []}, {}, {}
    with torch.cuda.stream(stream):
        for _ in range(ROUNDS):
            for opt in (0, 1):
                ix.set_option("flat-l2-image", opt)
                step()                                       # untimed: the first call behind the switch
                stream.synchronize()
                for _ in range(STEPS):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    step()
                    e1.record(stream)
                    stream.synchronize()
                    times[opt].append(e0.elapsed_time(e1))
                answers[opt] = (od.cpu().numpy().copy(), ol.cpu().numpy().copy(), on.cpu().numpy().copy())
                image_bytes = ix.filter_image_bytes()
                ix.search_batch(Qh, K)                       # the host path once, untimed: it downloads the batch's counters
                st = ix.stats()
                info[opt] = {"image_bytes": image_bytes, "candidates": int(st.last_filter_candidates), "fallback": int(st.last_filter_fallback)}
    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(answers[0], answers[1]))
    on_path = info[1]["image_bytes"] > 0 and info[0]["image_bytes"] == 0 and info[1]["candidates"] > 0
    out = {"rows": rows, "dim": dim, "metric": "L2", "batch": BATCH, "k": K, "timed_steps_per_leg": len(times[0])}
    for opt, name in ((0, "f32_rows"), (1, "image")):
        t = times[opt]
        out[name] = {"ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3), "ms_max": round(max(t), 3), **info[opt]}
    out["image_over_f32_rows"] = round(out["image"]["ms_median"] / out["f32_rows"]["ms_median"], 3)
    out["identical"] = bool(same)
    print(json.dumps(out), flush=True)
    ix.close()
    return 0 if same and on_path else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1250000])
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r17_flat_l2_image_probe.log"))
    ap.add_argument("--limit", type=int, default=400, help="seconds per size")
    ap.add_argument("--point", type=int, metavar="ROWS")
    a = ap.parse_args()
    if a.point:
        return point(a.point, a.dim)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as log:
        log.write("# scripts/flat_l2_image_probe.py: f32 L2, %d-query batches, k = %d; flat-l2-image 0 / 1 alternating on one index, %d timed steps per leg\n"
                  % (BATCH, K, ROUNDS * STEPS))
        for rows in a.rows:
            try:
                p = subprocess.run([sys.executable, __file__, "--dim", str(a.dim), "--point", str(rows)], capture_output=True, text=True, timeout=a.limit)
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
