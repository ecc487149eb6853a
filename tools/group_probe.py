"""Cost of the groups call (nb_hip_groups, nb_hip_ensemble_groups); prints ONE JSON line.  Nothing is asserted.

worlds      for N = 6 000 (the GUI's world), 65 536 and 2^20 (galaxy pairs, M = what the generator gives), all particles, per
            linking length: b = 0.05, 0.2 and 1.0 of the mean separation over the bounding box, and `everything`, a length
            above the box's diagonal so that every pair links.  Per case: blocking wall ms and kernel ms (nb_hip_last_diag_ms:
            ONE interval around the three launches -- init, pairs, flatten; the launches apart are not measured), fastest and
            median of the repeats after a warm-up, cycles per wave-pair (64 of the N (N - 1) / 2 pairs examined) at 2.4 GHz on
            1 024 SIMDs, the number of groups and the largest.  Beside them neighbours() of the same world in the same run (it
            examines N (N - 1) ordered pairs) and its cycles per wave-pair.
spans       per world, at b = 0.2: the kernel ms for forced span lengths (nb_hip_group_span; those that make at most 1 024
            spans) beside auto, and whether every length gave the bits of auto: what the host's policy is held against.
old_route   N = 6 000 only, per length: get_data() + the same labels in numpy (linked pairs per block of rows, then min-label
            propagation with pointer jumping to a fixpoint).
ensemble    256 x N = 250: ONE SimBatch.groups call against 256 resident SimPipelines one after another, members compared.

    python tools/group_probe.py [--reps 3] [--sizes 6000,65536,1048576] [--everything-up-to 1048576] [--out profiles/group_probe.json]
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
BS = (0.05, 0.2, 1.0)


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


def numpy_groups(p, length):
    """labels of groups(length) from a read-back array: all particles, float32 q against the float64 square."""
    x, y = p[:, 0], p[:, 1]
    n = p.shape[0]
    l2 = float(np.float32(length)) ** 2
    ii, jj = [], []
    for i0 in range(0, n, 1024):
        i = np.arange(i0, min(i0 + 1024, n))
        with np.errstate(all="ignore"):
            dx, dy = x[i, None] - x[None, :i[-1]], y[i, None] - y[None, :i[-1]]
            hit = (dx * dx + dy * dy).astype(np.float64) < l2
        hit &= np.arange(i[-1])[None, :] < i[:, None]
        r, c = np.nonzero(hit)
        ii.append(i[r])
        jj.append(c)
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    label = np.arange(n)
    while True:
        new = label.copy()
        np.minimum.at(new, ii, label[jj])
        np.minimum.at(new, jj, label[ii])
        new = new[new]
        if np.array_equal(new, label):
            return label.astype(np.uint32)
        label = new


def case(sim, length, pairs, reps):
    kernel = []

    def call():
        out = sim.groups(length, return_count=True)
        kernel.append(sim.last_diag_ms())
        return out

    wall = timed(call, reps)
    labels, groups = call()
    k = min(kernel[1:])
    return {"linking_length": length, "pairs": pairs, "wall": stats(wall), "kernel": stats(kernel[1:]),
            "pairs_per_s": round(pairs / (k * 1e-3), 1) if k > 0 else None, "cycles_per_wave_pair": cycles_per_wave_pair(k, pairs),
            "groups": groups, "largest": int(nb.group_table(labels)[1][0])}


def span_sweep(sim, n, length, reps):
    blocks = n // 256 + 1
    auto = sim.groups(length)
    rows, equal = {}, True
    try:
        for span in [0] + [s for s in sorted({1, 2, 4, 8, 16, 64, 256, 1024, blocks}) if s <= blocks and blocks <= 1024 * s]:
            nb.hip_lib().nb_hip_group_span(span)
            kernel = []
            for _ in range(reps + 1):
                equal = sim.groups(length).tobytes() == auto.tobytes() and equal
                kernel.append(sim.last_diag_ms())
            rows["auto" if span == 0 else str(span)] = round(min(kernel[1:]), 4)
    finally:
        nb.hip_lib().nb_hip_group_span(0)
    return {"blocks": blocks, "kernel_ms_by_span_blocks": rows, "every_span_equals_auto": equal}


def world_row(n, reps, everything_up_to):
    p, m = partitioned(n, seed=11037)
    sim = nb.SimPipeline(n, m)
    sim.set_data(p)
    lo, hi = p[:, 0:2].min(axis=0).astype(np.float64), p[:, 0:2].max(axis=0).astype(np.float64)
    area = float(np.prod(hi - lo))
    reps = reps if n < (1 << 19) else 2
    pairs = n * (n - 1) // 2
    row = {"n": n, "mass_len": m, "box_area": area, "mean_separation": nb.linking_length_for(n, area, 1.0), "lengths": {}}
    lengths = {f"b={b}": nb.linking_length_for(n, area, b) for b in BS}
    if n <= everything_up_to:
        lengths["everything"] = float(np.float32(2.0 * np.hypot(*(hi - lo))))
    for name, length in lengths.items():
        row["lengths"][name] = case(sim, length, pairs, reps)
    near_kernel = []

    def neighbours():
        sim.neighbours()
        near_kernel.append(sim.last_diag_ms())

    near_wall = timed(neighbours, reps)
    k = min(near_kernel[1:])
    row["neighbours"] = {"pairs": 2 * pairs, "wall": stats(near_wall), "kernel": stats(near_kernel[1:]),
                         "cycles_per_wave_pair": cycles_per_wave_pair(k, 2 * pairs)}
    row["spans"] = span_sweep(sim, n, lengths["b=0.2"], reps)
    if n <= 6000:
        row["old_route"] = {}
        for name, length in lengths.items():
            old = timed(lambda: numpy_groups(sim.get_data(), length), reps)
            row["old_route"][name] = {"get_data_plus_numpy": stats(old), "equal": numpy_groups(sim.get_data(), length).tobytes() == sim.groups(length).tobytes(),
                                      "over_groups_wall": round(min(old) / row["lengths"][name]["wall"]["best_ms"], 1)}
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
    length = 100.0
    one = lambda: batch.groups(length)
    loop = lambda: [s.groups(length) for s in pipes]
    equal = one().tobytes() == np.stack(loop()).tobytes()
    t_one, t_loop = timed(one, reps), timed(loop, reps)
    labels, groups = batch.groups(length, return_count=True)
    kernel = batch.last_diag_ms()
    batch.close()
    for s in pipes:
        s.close()
    return {"count": count, "n": n, "linking_length": length, "one_call": stats(t_one), "kernel_ms": round(kernel, 4), "pipelines": stats(t_loop),
            "ratio": round(min(t_loop) / min(t_one), 1), "members_equal": equal, "mean_groups_per_member": round(float(groups.mean()), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="6000,65536,1048576")
    ap.add_argument("--everything-up-to", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    worlds = [world_row(int(n), args.reps, args.everything_up_to) for n in args.sizes.split(",")]
    line = json.dumps({"probe": "group", "device": nb.device_info(), "reps": args.reps, "clock_hz": CLOCK_HZ, "simds": SIMDS, "worlds": worlds,
                       "ensemble": ensemble_row(256, 250, args.reps)})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
