"""Cost and output of the energy diagnostics (nb_hip_energy / nb_hip_potential) on the worlds users run; prints ONE JSON line.

Worlds: the headline workload (MakeGalaxies(2^20, 2), libc seed 11037) and the GUI's world (6 000 particles, 3 galaxies).
For each: device ms of nb_hip_energy and nb_hip_potential (their own event pair, median of 5 after a warm-up call), the
wall ms of the blocking call (median of 5), one step's device ms in the same process (the "timing" knob's events, median
of 5 single-step calls), pair interactions per second of each call, and an energy / momentum series over --steps steps at
dt = 0.01 sampled every --every steps.

    python tools/energy_probe.py [--steps 1000] [--every 100] [--out profiles/energy_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nbody_amd as nb  # noqa: E402


def partition(a):
    """mass > 0 first, the World's own order (CreateWorld), read back without touching the device"""
    w = nb.World(a)
    p = w.particles()
    w.close()
    return p, int((p[:, 6] > 0).sum())


def timed(fn, sim, reps=5):
    fn()  # warm-up
    dev, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(sim.last_diag_ms())
    return statistics.median(dev), statistics.median(wall)


def probe(name, a, steps, every, dt=0.01):
    part, m = partition(a)
    n = part.shape[0]
    sim = nb.SimPipeline(n, m)
    sim.set_data(part)
    e_ms, e_wall = timed(sim.energy, sim)
    p_ms, p_wall = timed(sim.potential, sim)
    step_ms = []
    for _ in range(6):
        sim.update(1, dt)
        step_ms.append(sim.last_step_ms()[0])
    step = statistics.median(step_ms[1:])
    sim.close()
    # the series starts again from the initial state
    sim = nb.SimPipeline(n, m)
    sim.set_data(part)
    series = []
    for k in range(0, steps + 1, every):
        if k:
            sim.update(every, dt)
        e = sim.energy()
        series.append({"step": k, "kinetic": e["kinetic"], "potential": e["potential"], "total": e["total"],
                       "momentum": list(e["momentum"]), "angular_momentum": e["angular_momentum"]})
    sim.close()
    e0 = series[0]["total"]
    return {"world": name, "n": n, "mass_len": m,
            "energy_ms": round(e_ms, 4), "energy_wall_ms": round(e_wall, 4),
            "potential_ms": round(p_ms, 4), "potential_wall_ms": round(p_wall, 4),
            "step_ms": round(step, 4), "energy_over_step": round(e_ms / step, 4), "potential_over_step": round(p_ms / step, 4),
            "energy_pairs_per_s": m * m / (e_ms * 1e-3), "potential_pairs_per_s": n * m / (p_ms * 1e-3),
            "max_rel_energy_drift": max(abs(s["total"] - e0) / abs(e0) for s in series),
            "dt": dt, "series": series}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert nb.device_count() >= 1, "energy_probe needs an MI355X"
    worlds = [("galaxies_2^20x2_seed11037", nb.make_galaxies(1 << 20, 2, seed=11037)),
              ("gui_6000x3", nb.make_galaxies(6000, 3, seed=11037))]
    out = {"tool": "energy_probe", "device": nb.device_info(), "worlds": [probe(k, a, args.steps, args.every) for k, a in worlds]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
