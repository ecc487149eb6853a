"""Cost of the neighbour call (nb_hip_neighbours, nb_hip_ensemble_neighbours); prints ONE JSON line.  Nothing is asserted.

worlds      for N = 6 000 (the GUI's world), 65 536 and 2^20 (galaxy pairs, M = what the generator gives), all receivers against
            all sources, per kernel instance (`nearest`: no radius; `counted`: a radius of 1 % of the system size, the 99th
            percentile radius).  Per case: blocking wall ms and kernel ms (nb_hip_last_diag_ms), fastest and median of the repeats
            after a warm-up, pairs per second and cycles per wave-pair (64 pairs) at 2.4 GHz on 1 024 SIMDs.  Beside them
            potential() of the same world in the same run, and the ratio of the nearest-only instance's cycles to its.
spans       per world: the kernel ms of the nearest-only instance for forced span lengths (nb_hip_neighbour_span; those that
            make at most 1 024 spans) beside auto, and whether every length gave the bits of auto: what the host's policy is
            held against.
old_route   N = 6 000 only: get_data() + the same answer in numpy (a float32 q matrix per block of rows, argmin, a count).
ensemble    256 x N = 250: ONE SimBatch.neighbours call against 256 resident SimPipelines one after another, members compared.

    python tools/neighbour_probe.py [--reps 5] [--sizes 6000,65536,1048576] [--out profiles/neighbour_probe.json]
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

CLOCK_HZ, SIMDS = 2.4e9, 1024


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
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def stats(values):
    return {"best_ms": round(min(values), 4), "median_ms": round(statistics.median(values), 4)}


def cycles_per_wave_pair(kernel_ms, pairs):
    return round(kernel_ms * 1e-3 * CLOCK_HZ * SIMDS / (pairs / 64.0), 2) if pairs else None


def same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def numpy_neighbours(p, radius):
    """(q, index, count) of neighbours(radius) from a read-back array: all against all, float32 q, self masked by index."""
    x, y = p[:, 0], p[:, 1]
    n = p.shape[0]
    q, index, count = np.empty(n, np.float32), np.empty(n, np.uint32), np.empty(n, np.uint32)
    r2 = float(np.float32(radius)) ** 2
    for i0 in range(0, n, 1024):
        i = np.arange(i0, min(i0 + 1024, n))
        with np.errstate(all="ignore"):
            dx, dy = x[i, None] - x[None, :], y[i, None] - y[None, :]
            v = dx * dx + dy * dy
        v[i - i0, i] = np.nan
        count[i] = (v.astype(np.float64) < r2).sum(axis=1)
        v[~(v < np.inf)] = np.inf
        j = v.argmin(axis=1)
        q[i] = v[i - i0, j]
        index[i] = np.where(np.isinf(q[i]), 0xFFFFFFFF, j)
    return q, index, count


def case(sim, radius, pairs, reps):
    kernel = []

    def call():
        out = sim.neighbours(radius)
        kernel.append(sim.last_diag_ms())
        return out

    wall = timed(call, reps)
    k = min(kernel[1:])
    return {"radius": radius, "pairs": pairs, "wall": stats(wall), "kernel": stats(kernel[1:]),
            "pairs_per_s": round(pairs / (k * 1e-3), 1) if k > 0 else None, "cycles_per_wave_pair": cycles_per_wave_pair(k, pairs)}


def span_sweep(sim, n, reps):
    blocks = n // 256 + 1
    auto = sim.neighbours()
    rows, equal = {}, True
    try:
        for span in [0] + [s for s in sorted({1, 2, 4, 8, 16, 64, 256, 1024, blocks}) if s <= blocks and blocks <= 1024 * s]:
            nb.hip_lib().nb_hip_neighbour_span(span)
            kernel = []
            for _ in range(reps + 1):
                equal = same(sim.neighbours(), auto) and equal
                kernel.append(sim.last_diag_ms())
            rows["auto" if span == 0 else str(span)] = round(min(kernel[1:]), 4)
    finally:
        nb.hip_lib().nb_hip_neighbour_span(0)
    return {"blocks": blocks, "kernel_ms_by_span_blocks": rows, "every_span_equals_auto": equal}


def world_row(n, reps):
    p, m = partitioned(n, seed=11037)
    sim = nb.SimPipeline(n, m)
    sim.set_data(p)
    e = sim.energy()
    r = np.hypot(*(p[:m, 0:2].astype(np.float64) - np.array(e["center_of_mass"])).T)
    size = float(np.percentile(r, 99))
    radius = float(np.float32(1e-2 * size))
    reps = reps if n < (1 << 19) else 2
    pairs = n * (n - 1)
    row = {"n": n, "mass_len": m, "system_size": size, "nearest": case(sim, None, pairs, reps), "counted": case(sim, radius, pairs, reps)}
    q, index, count = sim.neighbours(radius)
    row["closest_pair"] = [list(t) for t in nb.closest_pairs(q, index)]
    row["mean_count_within_radius"] = round(float(count.mean()), 3)
    phi_kernel = []

    def potential():
        sim.potential()
        phi_kernel.append(sim.last_diag_ms())

    phi_wall = timed(potential, reps)
    k = min(phi_kernel[1:])
    row["potential"] = {"interactions": n * m, "wall": stats(phi_wall), "kernel": stats(phi_kernel[1:]),
                        "cycles_per_wave_interaction": cycles_per_wave_pair(k, n * m)}
    row["nearest_cycles_over_potential_cycles"] = round(row["nearest"]["cycles_per_wave_pair"] / row["potential"]["cycles_per_wave_interaction"], 2)
    row["spans"] = span_sweep(sim, n, reps)
    if n <= 6000:
        old = timed(lambda: numpy_neighbours(sim.get_data(), radius), reps)
        row["old_route"] = {"get_data_plus_numpy": stats(old), "equal": same(numpy_neighbours(sim.get_data(), radius), (q, index, count)),
                            "over_neighbours_wall": round(min(old) / row["counted"]["wall"]["best_ms"], 1)}
    sim.close()
    return row


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
    radius = 100.0
    one = lambda: batch.neighbours(radius)
    loop = lambda: [s.neighbours(radius) for s in pipes]
    equal = same(one(), tuple(np.stack(c) for c in zip(*loop())))
    t_one, t_loop = timed(one, reps), timed(loop, reps)
    one()
    kernel = batch.last_diag_ms()
    batch.close()
    for s in pipes:
        s.close()
    return {"count": count, "n": n, "one_call": stats(t_one), "kernel_ms": round(kernel, 4), "pipelines": stats(t_loop),
            "ratio": round(min(t_loop) / min(t_one), 1), "members_equal": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="6000,65536,1048576")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    worlds = [world_row(int(n), args.reps) for n in args.sizes.split(",")]
    line = json.dumps({"probe": "neighbour", "device": nb.device_info(), "reps": args.reps, "clock_hz": CLOCK_HZ, "simds": SIMDS, "worlds": worlds,
                       "ensemble": ensemble_row(256, 250, args.reps)})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
