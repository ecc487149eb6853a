#!/usr/bin/env python3
"""What adaptive steps cost (include/nbody_adaptive.h), one JSON line.  Needs an MI355X.

For N = 6 000, 65 536 and 2^20 (one world each) and for an ensemble of 256 worlds of 250 particles:
  adaptive_ms      n adaptive steps in one call (nb_hip_adaptive_steps / nb_hip_ensemble_adaptive_steps)
  fixed_ms         update(n, dt) of the same tree: what the criterion launches and the lost chains add
  host_loop_ms     the loop the call replaces: get_data + host criterion (tests/timestep_ref.py) + update(1, dt)
  criterion_us     the criterion launch alone (nb_hip_timestep, one small copy and one sync included; single worlds only)
Fastest of --repeats, wall clock around blocking calls.  Write the line to profiles/r14_adaptive_probe.json when it has run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nbody_amd as nb  # noqa: E402
import timestep_ref as tr  # noqa: E402

ETA, DT_MAX = 0.1, 0.05


def fastest(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def one_world(n, steps, repeats):
    ic = nb.make_galaxies(n, 2, seed=11037)
    w = nb.World(ic)
    part = w.particles()
    w.close()
    m = int((part[:, 6] > 0).sum())
    s = nb.SimPipeline(n, m)
    s.set_data(part)
    s.update(2, 0.01)
    log, _ = s.update_adaptive(steps, ETA, DT_MAX)          # warm, and a representative step size for the fixed run
    dt = float(np.median(log))

    def host_loop():
        for _ in range(steps):
            s.update(1, float(tr.timestep(s.get_data(), ETA, DT_MAX)))

    row = {"n": n, "steps": steps, "dt_median": dt,
           "adaptive_ms": fastest(lambda: s.update_adaptive(steps, ETA, DT_MAX), repeats),
           "fixed_ms": fastest(lambda: s.update(steps, dt), repeats),
           "host_loop_ms": fastest(host_loop, repeats),
           "criterion_us": fastest(lambda: s.timestep(ETA, DT_MAX), max(repeats, 10)) * 1e3}
    s.close()
    row["adaptive_over_fixed"] = row["adaptive_ms"] / row["fixed_ms"]
    row["adaptive_over_host_loop"] = row["adaptive_ms"] / row["host_loop_ms"]
    return row


def ensemble(count, n, steps, repeats):
    parts, ms = [], []
    for b in range(count):
        w = nb.World(nb.make_galaxies(n, 2, seed=1000 + b))
        p = w.particles()
        w.close()
        parts.append(p)
        ms.append(int((p[:, 6] > 0).sum()))
    s = nb.SimBatch(n, ms)
    s.set_data(np.stack(parts))
    s.update(2, 0.01)
    log, _ = s.update_adaptive(steps, ETA, DT_MAX)
    dts = np.median(log, axis=0).astype(np.float32)

    def host_loop():
        for _ in range(steps):
            state = s.get_data()
            s.update(1, np.array([tr.timestep(state[b], ETA, DT_MAX) for b in range(count)], dtype=np.float32))

    row = {"count": count, "n": n, "steps": steps,
           "adaptive_ms": fastest(lambda: s.update_adaptive(steps, ETA, DT_MAX), repeats),
           "fixed_ms": fastest(lambda: s.update(steps, dts), repeats),
           "host_loop_ms": fastest(host_loop, repeats)}
    s.close()
    row["adaptive_over_fixed"] = row["adaptive_ms"] / row["fixed_ms"]
    row["adaptive_over_host_loop"] = row["adaptive_ms"] / row["host_loop_ms"]
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[6000, 65536, 1 << 20])
    args = ap.parse_args()
    if nb.device_count() < 1:
        sys.exit("adaptive_probe.py needs an MI355X")
    out = {"tool": "adaptive_probe", "device": nb.device_info(), "eta": ETA, "dt_max": DT_MAX,
           "worlds": [one_world(n, args.steps, args.repeats) for n in args.sizes],
           "ensemble": ensemble(256, 250, args.steps, args.repeats)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
