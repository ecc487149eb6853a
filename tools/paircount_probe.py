"""Cost of pair-separation counts (nb_hip_pair_counts, nb_hip_ensemble_pair_counts); prints ONE JSON line.  Nothing is asserted.

worlds      for N = 6 000 (the GUI's world), 65 536 and 2^20 (galaxy pairs, M = what the generator gives), 64 logarithmic bins,
            classes "mm" and "all", two edge sets: `wide` reaches twice the system size (the 99th percentile radius), `short`
            ends at 1 % of it, where almost every wave takes the wave-uniform skip.  Per case: blocking wall ms and kernel ms
            (nb_hip_last_diag_ms), fastest and median of the repeats after a warm-up, pairs per second and cycles per wave-pair
            (64 pairs) at 2.4 GHz on 1 024 SIMDs.  Beside them potential() of the same world (~18 cycles per
            wave-interaction: 5 VALU + 1 rsq) as context.
coincident  N = 65 536 at one place: every pair in one row, the case the wave merge is for (there is no hook to switch the
            merge off, so only the merged kernel is timed).
old_route   N = 6 000 only: get_data() + the same counts in numpy (every pair once, one sort per block of rows).
ensemble    256 x N = 250: ONE SimBatch.pair_counts call against 256 resident SimPipelines one after another, members compared.

    python tools/paircount_probe.py [--reps 5] [--sizes 6000,65536,1048576] [--out profiles/paircount_probe.json]
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
    return round(kernel_ms * 1e-3 * CLOCK_HZ * SIMDS / (pairs / 64.0), 1) if pairs else None


def class_pairs(n, m, classes):
    t = n - m
    return (m * (m - 1) // 2 if "mm" in classes or classes == "all" else 0) + (m * t if "mt" in classes or classes == "all" else 0) + \
        (t * (t - 1) // 2 if "tt" in classes or classes == "all" else 0)


def numpy_counts(p, m, edges):
    """The counts of pair_counts(edges, "all") from a read-back array: float32 q of every unordered pair, the blocks of rows
    sorted, the float64 squares of the edges looked up in them."""
    x, y = p[:, 0], p[:, 1]
    n = p.shape[0]
    e2 = edges.astype(np.float64) ** 2
    out = np.zeros((len(edges) + 1, 3), dtype=np.uint64)
    for col, (r0, r1, s0, s1) in enumerate(((0, m, 0, m), (0, m, m, n), (m, n, m, n))):
        j = np.arange(s0, s1)
        for i0 in range(r0, r1, 2048):
            i = np.arange(i0, min(i0 + 2048, r1))
            dx, dy = x[i, None] - x[None, s0:s1], y[i, None] - y[None, s0:s1]
            q = dx * dx + dy * dy
            q = q[j[None, :] > i[:, None]] if col != 1 else q.ravel()
            qs = np.sort(q[~np.isnan(q)]).astype(np.float64)
            below = np.searchsorted(qs, e2, side="left")
            out[:, col] += np.diff(np.concatenate([[0], below, [qs.shape[0]]])).astype(np.uint64)
    return out


def case(sim, edges, classes, pairs, reps):
    kernel = []

    def call():
        out = sim.pair_counts(edges, classes)
        kernel.append(sim.last_diag_ms())
        return out

    wall = timed(call, reps)
    k = min(kernel[1:])
    return {"classes": classes, "pairs": pairs, "wall": stats(wall), "kernel": stats(kernel[1:]),
            "pairs_per_s": round(pairs / (k * 1e-3), 1) if k > 0 else None, "cycles_per_wave_pair": cycles_per_wave_pair(k, pairs)}


def world_row(n, reps):
    p, m = partitioned(n, seed=11037)
    sim = nb.SimPipeline(n, m)
    sim.set_data(p)
    e = sim.energy()
    r = np.hypot(*(p[:m, 0:2].astype(np.float64) - np.array(e["center_of_mass"])).T)
    size = float(np.percentile(r, 99))
    sets = {"wide": nb.profile_edges(1e-3 * size, 2.0 * size, BINS, log=True), "short": nb.profile_edges(1e-5 * size, 1e-2 * size, BINS, log=True)}
    reps = reps if n < (1 << 19) else 2
    row = {"n": n, "mass_len": m, "bins": BINS, "system_size": size, "cases": {}}
    for name, edges in sets.items():
        row["cases"][name] = [case(sim, edges, c, class_pairs(n, m, c), reps) for c in ("mm", "all")]
        got = sim.pair_counts(edges, "all")
        row["cases"][name][1]["fraction_beyond_last_edge"] = round(float(got[-1].sum()) / max(1, int(got.sum())), 6)
    phi_kernel = []

    def potential():
        sim.potential()
        phi_kernel.append(sim.last_diag_ms())

    phi_wall = timed(potential, reps)
    k = min(phi_kernel[1:])
    row["potential"] = {"interactions": n * m, "wall": stats(phi_wall), "kernel": stats(phi_kernel[1:]),
                        "cycles_per_wave_interaction": cycles_per_wave_pair(k, n * m)}
    if n <= 6000:
        edges = sets["wide"]
        old = timed(lambda: numpy_counts(sim.get_data(), m, edges), reps)
        row["old_route"] = {"get_data_plus_numpy": stats(old), "equal": bool(np.array_equal(numpy_counts(sim.get_data(), m, edges), sim.pair_counts(edges, "all"))),
                            "over_pair_counts_wall": round(min(old) / row["cases"]["wide"][1]["wall"]["best_ms"], 1)}
    sim.close()
    return row


def coincident_row(n, reps):
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2], a[: n // 2, 6], a[:, 7] = (3.25, -1.5), 1.0, 0.25
    sim = nb.SimPipeline(n, n // 2)
    sim.set_data(a)
    edges = nb.profile_edges(0.0, 1.0, BINS)
    row = {"n": n, "mass_len": n // 2, "bins": BINS, "wave_merge": True, "case": case(sim, edges, "all", n * (n - 1) // 2, reps)}
    row["all_in_row_1"] = bool(sim.pair_counts(edges, "all")[1].sum() == n * (n - 1) // 2)
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
    edges = nb.profile_edges(1.0, 5.0e4, BINS, log=True)
    one = lambda: batch.pair_counts(edges, "all")
    loop = lambda: [s.pair_counts(edges, "all") for s in pipes]
    equal = bool(np.array_equal(one(), np.stack(loop())))
    t_one, t_loop = timed(one, reps), timed(loop, reps)
    one()
    kernel = batch.last_diag_ms()
    batch.close()
    for s in pipes:
        s.close()
    return {"count": count, "n": n, "bins": BINS, "one_call": stats(t_one), "kernel_ms": round(kernel, 4), "pipelines": stats(t_loop),
            "ratio": round(min(t_loop) / min(t_one), 1), "members_equal": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="6000,65536,1048576")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    worlds = [world_row(int(n), args.reps) for n in args.sizes.split(",")]
    line = json.dumps({"probe": "paircount", "device": nb.device_info(), "reps": args.reps, "clock_hz": CLOCK_HZ, "simds": SIMDS, "worlds": worlds,
                       "coincident": coincident_row(65536, args.reps), "ensemble": ensemble_row(256, 250, args.reps)})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
