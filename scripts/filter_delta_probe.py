"""What a derived filter costs against a rebuilt one (vk_filter_apply_delta[_batch] against vk_filter_create).

On a filter over 10M labels at 10 % selectivity -- `@tag:{x}` on the 10M-row index of BASELINE configs[4] -- this times, as host
wall time around each blocking C call (the ctypes call itself, tables prepared and results released outside the clock):
  (a) vk_filter_create from the full id list (what BuildFilter does after every write phase today);
  (b) vk_filter_apply_delta with 10 / 1 000 / 100 000 changed labels (half set, half cleared);
  (c) vk_filter_apply_delta_batch of 16 and of 256 tags with 1 000 changes each, against 16 / 256 single calls;
  and, for the fixed cost of a blocking filter call on this lease, a single vk_filter_combine and an empty delta.
Median (and min / p90) of --reps calls after --warmup calls of the same shape; (b) against (a) of the SAME run is the
comparison that counts.  Writes the table to --out (default profiles/r07_filter_delta_probe.log) with the date of the run.

    python scripts/filter_delta_probe.py [--labels 10000000] [--selectivity 0.1] [--reps 30] [--warmup 5] [--out PATH]
"""
import argparse
import ctypes as C
import datetime
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--labels", type=int, default=10_000_000)
    ap.add_argument("--selectivity", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r07_filter_delta_probe.log"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("filter_delta_probe: no GPU (nothing is measured without one)")
    torch.cuda.init()
    import _pkg
    vsa = _pkg.vsa
    L = vsa.lib()
    rng = np.random.default_rng(7)
    n = a.labels
    g = vsa.Index("FLAT", 8, "L2", initial_cap=1024)
    g.add_batch(np.zeros((4, 8), np.float32))
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(name, call, after=lambda: None, reps=a.reps):
        """median / min / p90 in microseconds of call() (blocking); after() runs outside the clock"""
        for _ in range(a.warmup):
            call()
            after()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter_ns()
            call()
            t.append((time.perf_counter_ns() - t0) / 1e3)
            after()
        t = np.sort(np.array(t))
        med = float(np.median(t))
        say(f"{name:<58s} median {med:10.1f} us   min {t[0]:10.1f}   p90 {t[int(0.9 * (len(t) - 1))]:10.1f}   ({len(t)} calls)")
        return med

    say(f"# filter delta probe, {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}, {torch.cuda.get_device_name(0)}")
    say(f"# {n} labels, selectivity {a.selectivity}, {a.warmup} warm-up + {a.reps} timed calls per line, host wall time around the blocking call")
    ids = rng.permutation(n)[: int(n * a.selectivity)].astype(np.uint64)          # a posting list: ids in no particular order
    out = C.c_void_p()
    held = []

    def release_out():
        L.vk_filter_release(out)

    # (a) the rebuild
    def create():
        assert L.vk_filter_create(g._h, n, ids.ctypes.data, ids.size, None, 0, None, C.byref(out)) == 0
    t_create = timed(f"(a) vk_filter_create, {ids.size} ids", create, release_out)
    base = g.make_filter(n, labels=ids)
    other = g.make_filter(n, labels=rng.permutation(n)[: int(n * a.selectivity)].astype(np.uint64))
    # the fixed cost of a blocking filter call on this lease
    t_combine = timed("    vk_filter_combine (a AND b), single", lambda: L.vk_filter_combine(g._h, base._h, other._h, 0, C.byref(out)), release_out)

    def delta_table(bases, changes):
        tab = (vsa.FilterDelta * len(bases))()
        for i, b in enumerate(bases):
            lab = rng.integers(0, n, size=changes, dtype=np.uint64)
            st, cl = np.ascontiguousarray(lab[: changes // 2]), np.ascontiguousarray(lab[changes // 2:])
            held.extend([st, cl])
            tab[i] = vsa.FilterDelta(b._h, n, vsa._ptr(cl), cl.size, vsa._ptr(st), st.size)
        return tab

    # (b) one derived filter
    t_delta = {}
    for changes in (0, 10, 1000, 100_000):
        tab = delta_table([base], changes)
        def one(tab=tab):
            assert L.vk_filter_apply_delta(g._h, tab, C.byref(out)) == 0
        t_delta[changes] = timed(f"(b) vk_filter_apply_delta, {changes} changed labels", one, release_out)
    # ... growing by 1M labels as well (an ingest phase)
    tab = delta_table([base], 1000)
    tab[0].nbits = n + 1_000_000
    timed("(b) vk_filter_apply_delta, 1000 changed labels, +1M labels", lambda: L.vk_filter_apply_delta(g._h, tab, C.byref(out)), release_out)
    # (c) a batch of tags against its single calls
    t_batch = {}
    for tags in (16, 256):
        bases = [base] + [g.make_filter(n, labels=rng.permutation(n)[: int(n * a.selectivity)].astype(np.uint64)) for _ in range(min(tags, 16) - 1)]
        bases = [bases[i % len(bases)] for i in range(tags)]
        tab = delta_table(bases, 1000)
        outs = (C.c_void_p * tags)()

        def release_outs(outs=outs, tags=tags):
            for i in range(tags):
                L.vk_filter_release(outs[i])

        def batch(tab=tab, outs=outs, tags=tags):
            assert L.vk_filter_apply_delta_batch(g._h, tab, tags, outs) == 0

        def singles(tab=tab, outs=outs, tags=tags):
            for i in range(tags):
                L.vk_filter_apply_delta(g._h, C.byref(tab[i]), C.cast(C.byref(outs, i * C.sizeof(C.c_void_p)), C.POINTER(C.c_void_p)))
        reps = a.reps if tags <= 16 else max(20, a.reps // 2)
        tb = timed(f"(c) vk_filter_apply_delta_batch, {tags} tags x 1000 changes", batch, release_outs, reps)
        ts = timed(f"(c) {tags} single vk_filter_apply_delta calls, 1000 changes each", singles, release_outs, reps)
        t_batch[tags] = (tb, ts)
    say("")
    say(f"rebuild / delta(1000)   = {t_create / t_delta[1000]:.1f}x   ({t_create:.0f} us against {t_delta[1000]:.0f} us)")
    say(f"rebuild / delta(100000) = {t_create / t_delta[100_000]:.1f}x")
    say(f"delta(0) - combine      = {t_delta[0] - t_combine:+.1f} us (the fixed cost of a blocking filter call: combine {t_combine:.0f} us)")
    for tags, (tb, ts) in t_batch.items():
        say(f"{tags} singles / batch of {tags} = {ts / tb:.1f}x   ({ts:.0f} us against {tb:.0f} us; {tb / tags:.1f} us per tag in the batch)")
    # what was derived is right (the probe is no test, but a wrong answer would make its times meaningless)
    lab = rng.integers(0, n, size=1000, dtype=np.uint64)
    got = g.filter_apply_delta(base, n, set=lab[:500], clear=lab[500:])
    model = np.zeros(n, bool)
    model[ids.astype(np.int64)] = True
    model[lab[500:].astype(np.int64)] = False
    model[lab[:500].astype(np.int64)] = True
    assert got.info() == (n, int(model.sum())) and np.array_equal(got.read(), np.pad(np.packbits(model, bitorder="little"), (0, (-((n + 7) // 8)) % 8)).view(np.uint64)), "derived filter differs from the model"
    say(f"checked: the derived filter equals the host model ({int(model.sum())} allowed)")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
