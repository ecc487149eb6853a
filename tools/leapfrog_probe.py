#!/usr/bin/env python3
"""What leapfrog steps cost (include/nbody_leapfrog.h), one JSON line.  Needs an MI355X.

For N = 2^20, 65 536, 6 000 and 250 (one world each) and for an ensemble of 256 worlds of 250 particles:
  leapfrog_ms      n kick-drift-kick steps in one call (nb_hip_leapfrog_steps / nb_hip_ensemble_leapfrog); every call of the
                   timed loop follows a leapfrog call, so it makes n force launches and does not prime
  fixed_ms         update(n, dt) of the same tree: what the kick / drift passes and the lost chains add
  adaptive_ms      update_adaptive(n, ...): the existing path with the same launch count per step
"perf_test_ratio" repeats the measurement of tests/test_gpu_leapfrog_perf.py (N = 65 536, 50 steps, best of 5).
Fastest of --repeats, wall clock around blocking calls.  The recorded line: profiles/r16_leapfrog_probe.json."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import nbody_amd as nb  # noqa: E402

DT, ETA, DT_MAX = 0.01, 0.1, 0.05


def fastest(fn, repeats):
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def universe(n, seed):
    w = nb.World(nb.make_galaxies(n, 2, seed=seed))
    part = w.particles()
    w.close()
    return part, int((part[:, 6] > 0).sum())


def ratios(row):
    row["leapfrog_over_fixed"] = row["leapfrog_ms"] / row["fixed_ms"]
    row["leapfrog_over_adaptive"] = row["leapfrog_ms"] / row["adaptive_ms"]
    return row


def one_world(n, steps, repeats):
    part, m = universe(n, 11037)
    s = nb.SimPipeline(n, m)
    s.set_data(part)
    s.update(2, DT)
    s.update_adaptive(2, ETA, DT_MAX)          # warm every path
    s.update_leapfrog(2, DT)

    def leapfrog():
        s.update_leapfrog(steps, DT)

    row = {"n": n, "steps": steps, "leapfrog_ms": fastest(leapfrog, repeats + 1),          # the first repeat primes
           "force_launches": s.last_leapfrog_info()[0],
           "fixed_ms": fastest(lambda: s.update(steps, DT), repeats),
           "adaptive_ms": fastest(lambda: s.update_adaptive(steps, ETA, DT_MAX), repeats)}
    s.close()
    return ratios(row)


def ensemble(count, n, steps, repeats):
    worlds = [universe(n, 1000 + b) for b in range(count)]
    s = nb.SimBatch(n, [m for _, m in worlds])
    s.set_data(np.stack([p for p, _ in worlds]))
    s.update(2, DT)
    s.update_adaptive(2, ETA, DT_MAX)
    s.update_leapfrog(2, DT)
    row = {"count": count, "n": n, "steps": steps, "leapfrog_ms": fastest(lambda: s.update_leapfrog(steps, DT), repeats + 1),
           "force_launches": s.last_leapfrog_info()[0],
           "fixed_ms": fastest(lambda: s.update(steps, DT), repeats),
           "adaptive_ms": fastest(lambda: s.update_adaptive(steps, ETA, DT_MAX), repeats)}
    s.close()
    return ratios(row)


def perf_test_ratio():
    """The measurement of tests/test_gpu_leapfrog_perf.py: N = 65 536, 50 steps, best of 5, alternating."""
    part, m = universe(65536, 11037)
    s = nb.SimPipeline(65536, m)
    s.set_data(part)
    s.update(2, DT)
    s.update_adaptive(2, ETA, DT_MAX)
    s.update_leapfrog(2, DT)
    leapfrog, adaptive = [], []
    for _ in range(5):
        leapfrog.append(fastest(lambda: s.update_leapfrog(50, DT), 1))
        adaptive.append(fastest(lambda: s.update_adaptive(50, ETA, DT_MAX), 1))
    s.close()
    return min(leapfrog) / min(adaptive)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--big-steps", type=int, default=5, help="steps per call at N >= 2^19 (a step takes 0.2 s at 2^20)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 20, 65536, 6000, 250])
    args = ap.parse_args()
    if nb.device_count() < 1:
        sys.exit("leapfrog_probe.py needs an MI355X")
    out = {"tool": "leapfrog_probe", "device": nb.device_info(), "dt": DT, "eta": ETA, "dt_max": DT_MAX,
           "worlds": [one_world(n, args.big_steps if n >= 1 << 19 else args.steps, 2 if n >= 1 << 19 else args.repeats)
                      for n in args.sizes],
           "ensemble": ensemble(256, 250, args.steps, args.repeats),
           "perf_test_ratio": perf_test_ratio()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
