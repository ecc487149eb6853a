"""What a record of an ensemble's energy costs inside a chain of steps (nb_hip_ensemble_trace) beside the host loop it
replaces; prints ONE JSON line.

B = 256 synthetic worlds (half of the particles massive) of N = 250 (the one-workgroup chain) and N = 1 000 (lane-split
launches), recorded every 1, 10 and 100 steps.  Per (N, every), blocking wall time of the whole call, best of 3 after a
warm-up, as microseconds per step and per record:
  loop         the host loop: energy(), then update(every) + energy() per record
  interleaved  trace() with the diagnostics launches enqueued between the step launches (forced where N <= 512)
  fused        trace() recording inside the chain launch (N <= 512 only)
  untraced     update(n) alone: what the steps cost without any record
n = max(200, 20 * every) steps per call, so every call makes at least 20 records.  Rows are compared bitwise on the way.

    python tools/batch_trace_probe.py [--out profiles/batch_trace_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nbody_amd as nb  # noqa: E402

COUNT, SIZES, EVERY, DT = 256, (250, 1000), (1, 10, 100), 0.01


def world(n, seed):
    """n particles, the first n // 2 massive (already partitioned)"""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * 1.0e4
    a[:, 2:4] = rng.standard_normal((n, 2)) * 10
    m = n // 2
    a[:, 7] = 0.5
    a[:m, 7] = 1.5 + 8 * rng.random(m)
    a[:m, 6] = 41.9 * a[:m, 7] ** 3
    return a, m


def best_of(fn, reset, reps=3):
    reset()
    fn()  # warm-up
    best, out = float("inf"), None
    for _ in range(reps):
        reset()
        t0 = time.perf_counter()
        out = fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e6, out


def probe(n):
    worlds = [world(n, 7919 * n + b) for b in range(COUNT)]
    start = np.stack([p for p, _ in worlds])
    batch = nb.SimBatch(n, [m for _, m in worlds])
    reset = lambda: batch.set_data(start)  # noqa: E731

    def loop(steps, every):
        rows = [batch.energy()]
        for _ in range(steps // every):
            batch.update(every, DT)
            rows.append(batch.energy())
        return rows

    def trace(mode, steps, every):
        batch.trace_mode(mode)
        rows = batch.trace(steps, DT, every)
        batch.trace_mode(0)
        return rows, batch.last_trace_info()

    out = []
    for every in EVERY:
        steps = max(200, 20 * every)
        records = 1 + steps // every
        us = {}
        us["loop"], want = best_of(lambda: loop(steps, every), reset)
        us["interleaved"], (rows, info) = best_of(lambda: trace(1, steps, every), reset)
        assert info["fused"] == 0 and [[nb.energy_row(x) for x in r] for r in rows] == want
        launches = {"interleaved": info["launches"]}
        if n <= 512:
            us["fused"], (fused, info) = best_of(lambda: trace(0, steps, every), reset)
            assert info["fused"] == 1 and fused.tobytes() == rows.tobytes()
            launches["fused"] = info["launches"]
        us["untraced"], _ = best_of(lambda: batch.update(steps, DT), reset)
        row = {"n": n, "mass_len": n // 2, "count": COUNT, "every": every, "steps": steps, "records": records, "launches": launches}
        for k, v in us.items():
            row[k + "_us_per_step"] = round(v / steps, 3)
            if k != "untraced":
                row[k + "_us_per_record"] = round(v / records, 3)
                row[k + "_record_cost_us"] = round((v - us["untraced"]) / records, 3)   # what one record adds to the steps
        out.append(row)
    batch.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert nb.device_count() >= 1, "batch_trace_probe needs an MI355X"
    out = {"tool": "batch_trace_probe", "device": nb.device_info(), "rows": [r for n in SIZES for r in probe(n)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
