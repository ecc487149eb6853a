"""Cost of the ensemble diagnostics (nb_hip_ensemble_energy / nb_hip_ensemble_potential) against the two ways a caller had
before them; prints ONE JSON line.

For N in {250, 512, 1 000, 3 000} and B in {1, 64, 256, 1 024} synthetic worlds (half of the particles massive):
  energy_us / potential_us            device microseconds of the kernels of one call (their own event pair)
  energy_wall_us / potential_wall_us  blocking wall microseconds of one call
  loop_energy_wall_us                 the same worlds' SimPipeline.energy() one after another, summed blocking wall time;
                                      at most 256 pipelines are built, a larger B is scaled from those (loop_worlds)
  get_data_wall_us                    the read-back SimBatch.get_data() alone, the first half of "sum it on the host"
all medians of 5 after a warm-up call.

    python tools/batch_energy_probe.py [--out profiles/batch_energy_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nbody_amd as nb  # noqa: E402

SIZES, COUNTS, LOOP_MAX = (250, 512, 1000, 3000), (1, 64, 256, 1024), 256


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


def wall_us(fn, reps=5, after=None):
    fn()  # warm-up
    wall, extra = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e6)
        if after:
            extra.append(after())
    return statistics.median(wall), (statistics.median(extra) if extra else None)


def probe(n):
    worlds = [world(n, 7919 * n + b) for b in range(max(COUNTS))]
    sims = []
    for p, m in worlds[:LOOP_MAX]:
        s = nb.SimPipeline(n, m)
        s.set_data(p)
        sims.append(s)
    rows = []
    for count in COUNTS:
        batch = nb.SimBatch(n, [m for _, m in worlds[:count]])
        batch.set_data(np.stack([p for p, _ in worlds[:count]]))
        e_wall, e_dev = wall_us(batch.energy, after=lambda: batch.last_diag_ms() * 1e3)
        p_wall, p_dev = wall_us(batch.potential, after=lambda: batch.last_diag_ms() * 1e3)
        g_wall, _ = wall_us(batch.get_data)
        batch.close()
        loop = sims[:min(count, LOOP_MAX)]
        l_wall, _ = wall_us(lambda: [s.energy() for s in loop])
        l_wall *= count / len(loop)
        rows.append({"n": n, "mass_len": n // 2, "count": count,
                     "energy_us": round(e_dev, 2), "energy_wall_us": round(e_wall, 2),
                     "potential_us": round(p_dev, 2), "potential_wall_us": round(p_wall, 2),
                     "loop_energy_wall_us": round(l_wall, 2), "loop_worlds": len(loop),
                     "get_data_wall_us": round(g_wall, 2), "loop_over_ensemble": round(l_wall / e_wall, 2)})
    for s in sims:
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert nb.device_count() >= 1, "batch_energy_probe needs an MI355X"
    out = {"tool": "batch_energy_probe", "device": nb.device_info(), "rows": [r for n in SIZES for r in probe(n)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
