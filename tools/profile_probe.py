"""Cost of a radial profile (nb_hip_profile, nb_hip_ensemble_profile) against the routes it replaces; prints ONE JSON line.

worlds      for N = 6 000 (the GUI's world), 65 536 and 2^20 (the headline galaxy pair), 64 logarithmic bins about the centre
            of mass: device us (nb_hip_last_diag_ms) and blocking wall us of one SimPipeline.profile call, fastest and median
            of --reps after a warm-up; beside it the route that existed before -- get_data() followed by the same sums in numpy
            (np.bincount per column: the cheapest numpy route, not the ordered one) -- and get_data() alone.
ensembles   256 x N = 250 and 32 x N = 3 000: ONE SimBatch.profile call against B resident SimPipelines called one after
            another, wall us and device us, members compared bit for bit.
yardstick   the two pairs tests/test_gpu_profile_perf.py asserts, as ratios.

    python tools/profile_probe.py [--reps 5] [--out profiles/profile_probe.json]
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

BINS = 64
SIZES = (6000, 65536, 1 << 20)
ENSEMBLES = ((256, 250), (32, 3000))          # (B, N)


def partitioned(n, seed):
    w = nb.World(nb.make_galaxies(n, 2, seed=seed))
    p = w.particles()
    w.close()
    return p, int((p[:, 6] > 0).sum())


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return {"best_us": round(min(out), 1), "median_us": round(statistics.median(out), 1)}


def numpy_route(p, m, edges, centre, velocity):
    """The sums of profile() from a read-back array: row by searchsorted, columns by bincount."""
    d = p[:m, 0:2].astype(np.float64) - centre
    v = p[:m, 2:4].astype(np.float64) - velocity
    wgt = p[:m, 6].astype(np.float64)
    q = d[:, 0] ** 2 + d[:, 1] ** 2
    row = np.searchsorted(edges.astype(np.float64) ** 2, q, side="right")
    cols = (np.ones(m), wgt, wgt * q, wgt * (d[:, 0] * v[:, 1] - d[:, 1] * v[:, 0]), wgt * (d[:, 0] * v[:, 0] + d[:, 1] * v[:, 1]),
            wgt * (v[:, 0] ** 2 + v[:, 1] ** 2))
    return np.stack([np.bincount(row, weights=c, minlength=len(edges) + 1) for c in cols], axis=1)


def world_row(n, reps):
    p, m = partitioned(n, seed=11037)
    sim = nb.SimPipeline(n, m)
    sim.set_data(p)
    e = sim.energy()
    centre = np.array(e["center_of_mass"])
    velocity = np.array(e["momentum"]) / e["mass"]
    r = np.hypot(*(p[:m, 0:2].astype(np.float64) - centre).T)
    edges = nb.profile_edges(float(np.percentile(r, 1)), float(np.percentile(r, 99)), BINS, log=True)
    device = []

    def call():
        out = sim.profile(edges, centre, velocity)
        device.append(sim.last_diag_ms() * 1e3)
        return out

    rows = call()
    wall = timed(call, reps)
    old = timed(lambda: numpy_route(sim.get_data(), m, edges, centre, velocity), reps)
    read = timed(sim.get_data, reps)
    approx = numpy_route(sim.get_data(), m, edges, centre.astype(np.float32).astype(np.float64), velocity.astype(np.float32).astype(np.float64))
    sim.close()
    return {"n": n, "mass_len": m, "bins": BINS, "device_us_best": round(min(device[1:]), 1), "device_us_median": round(statistics.median(device[1:]), 1),
            "wall": wall, "get_data_plus_numpy": old, "get_data_alone": read,
            "old_route_over_profile_wall": round(old["best_us"] / wall["best_us"], 2),
            "get_data_alone_over_profile_wall": round(read["best_us"] / wall["best_us"], 2),
            "counts_equal_numpy": bool(np.array_equal(rows[:, 0], approx[:, 0])),
            "worst_relative_difference_to_numpy": float(np.max(np.abs(rows - approx) / np.maximum(np.abs(approx), 1e-300)))}


def ensemble_row(count, n, reps):
    made = [partitioned(n, seed=100 + b) for b in range(count)]
    batch = nb.SimBatch(n, [m for _, m in made])
    batch.set_data(np.stack([p for p, _ in made]))
    batch.update(20, 0.01)
    states = batch.get_data()
    pipes = []
    for a, (_, m) in zip(states, made):
        pipes.append(nb.SimPipeline(n, m))
        pipes[-1].set_data(a)
    edges = nb.profile_edges(1.0, 5.0e4, BINS, log=True)
    centres = np.array([np.average(a[:m, 0:2], axis=0, weights=a[:m, 6]) for a, (_, m) in zip(states, made)], dtype=np.float32)
    one = lambda: batch.profile(edges, centre=centres)
    loop = lambda: [s.profile(edges, centre=c) for s, c in zip(pipes, centres)]
    equal = bool(np.array_equal(one().view(np.uint64), np.stack(loop()).view(np.uint64)))
    t_one, t_loop = timed(one, reps), timed(loop, reps)
    one()
    device = batch.last_diag_ms() * 1e3
    batch.close()
    for s in pipes:
        s.close()
    return {"count": count, "n": n, "bins": BINS, "one_call": t_one, "device_us": round(device, 1), "pipelines": t_loop,
            "ratio": round(t_loop["best_us"] / t_one["best_us"], 1), "members_bitwise_equal": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    worlds = [world_row(n, args.reps) for n in SIZES]
    ensembles = [ensemble_row(b, n, args.reps) for b, n in ENSEMBLES]
    line = json.dumps({"probe": "profile", "device": nb.device_info(), "reps": args.reps, "worlds": worlds, "ensembles": ensembles,
                       "yardstick": {"get_data_alone_over_profile_at_2_20": worlds[-1]["get_data_alone_over_profile_wall"],
                                     "pipelines_over_one_call_256_x_250": ensembles[0]["ratio"]}})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
