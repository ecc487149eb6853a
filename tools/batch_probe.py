#!/usr/bin/env python3
"""World ensembles (nb.SimBatch) beside the same worlds in B SimPipelines stepped one after another.

For N in {250, 512, 1000, 2000, 3000} and B in {1, 4, 64, 256, 1024}: microseconds per step of the whole ensemble (device
time by the ensemble's own event pair, and wall), median of 5 calls after one warm-up call, each call sized to last tens
of milliseconds -- beside the loop over B SimPipelines on auto in the same process (device time = the sum of the
pipelines' own timers), the two alternating.  Plus aggregate interactions/s, its fraction of the fp32 peak (14 flops per
interaction, 157.3 TFLOP/s: SURVEY.md 8d), and the cells where the ensemble is SLOWER per world than the loop.

Prints one JSON line.  The parent process never touches the GPU: every N runs in a child process of its own under a
time limit, and nothing is started after a child that failed.
usage: batch_probe.py [--n 250,512,...] [--b 1,4,...] [--limit-s 300]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

PEAK_FLOPS, FLOPS_PER_INTERACTION = 157.3e12, 14
DT = 0.01
LOOP_STEPS = 100          # per pipeline and call
TARGET_MS = 30.0          # an ensemble call


def worlds(n, count):
    import numpy as np
    import nbody_amd as nb
    parts, ms = [], []
    for b in range(count):
        w = nb.World(nb.make_galaxies(n, 2, seed=1 + b, own_rng=True))
        p = w.particles()
        w.close()
        parts.append(p)
        ms.append(int((p[:, 6] > 0).sum()))
    return np.stack(parts), ms


def cell(n, count, parts, ms):
    import nbody_amd as nb
    batch = nb.SimBatch(n, ms[:count])
    batch.set_data(parts[:count])
    sims = []
    for b in range(count):
        s = nb.SimPipeline(n, ms[b])
        s.set_data(parts[b])
        sims.append(s)
    batch.update(8, DT)                                    # sizes the calls; the warm-up call follows
    steps = int(min(20000, max(8, TARGET_MS / max(batch.last_ms() / 8, 1e-6))))

    def ensemble():
        t0 = time.perf_counter()
        batch.update(steps, DT)
        wall = time.perf_counter() - t0
        return batch.last_ms() * 1e3 / steps, wall * 1e6 / steps

    def loop():
        dev = 0.0
        t0 = time.perf_counter()
        for s in sims:
            s.update(LOOP_STEPS, DT)
            dev += s.last_step_ms()[0]
        wall = time.perf_counter() - t0
        return dev * 1e3 / LOOP_STEPS, wall * 1e6 / LOOP_STEPS

    ensemble(), loop()                                     # warm-up
    e, l = [], []
    for _ in range(5):
        e.append(ensemble())
        l.append(loop())
    shape, single = batch.launch_shape(), sims[0].launch_shape()
    fused = sims[0].fused_steps()
    batch.close()
    for s in sims:
        s.close()
    med = lambda rows, i: statistics.median(r[i] for r in rows)
    pairs = float(sum(n * m for m in ms[:count]))
    e_dev, e_wall, l_dev, l_wall = med(e, 0), med(e, 1), med(l, 0), med(l, 1)
    return {"n": n, "b": count, "path": shape["path"], "w": shape["w"], "lanes": shape["lanes"], "steps_per_call": steps,
            "ensemble_device_us_per_step": round(e_dev, 3), "ensemble_wall_us_per_step": round(e_wall, 3),
            "loop_device_us_per_step": round(l_dev, 3), "loop_wall_us_per_step": round(l_wall, 3),
            "loop_steps_per_call": LOOP_STEPS, "loop_member0_fused_steps": fused, "loop_member0_shape": single,
            "ensemble_device_us_per_world_step": round(e_dev / count, 4), "loop_device_us_per_world_step": round(l_dev / count, 4),
            "device_ratio_ensemble_over_loop": round(e_dev / l_dev, 5), "wall_ratio_ensemble_over_loop": round(e_wall / l_wall, 5),
            "interactions_per_s": pairs / (e_dev * 1e-6),
            "fp32_peak_frac": round(pairs / (e_dev * 1e-6) * FLOPS_PER_INTERACTION / PEAK_FLOPS, 4)}


def child(n, counts):
    import nbody_amd as nb
    assert nb.device_count() >= 1, "batch_probe needs an MI355X"
    parts, ms = worlds(n, max(counts))
    rows = [cell(n, c, parts, ms) for c in counts]
    print("ROWS " + json.dumps({"device": nb.device_info(), "rows": rows}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="250,512,1000,2000,3000")
    ap.add_argument("--b", default="1,4,64,256,1024")
    ap.add_argument("--limit-s", type=int, default=300)
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    counts = [int(x) for x in a.b.split(",")]
    if a.child:
        child(a.child, counts)
        return 0
    rows, device, failed = [], "", None
    for n in [int(x) for x in a.n.split(",")]:
        # one GPU step = one child under its own limit; after a failure nothing more is started on the GPU
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--b", a.b], capture_output=True,
                               text=True, timeout=a.limit_s)
        except subprocess.TimeoutExpired:
            failed = {"n": n, "why": f"no result within {a.limit_s} s"}
            break
        line = [x for x in r.stdout.splitlines() if x.startswith("ROWS ")]
        if r.returncode != 0 or not line:
            failed = {"n": n, "returncode": r.returncode, "stderr_tail": r.stderr[-400:]}
            break
        got = json.loads(line[-1][5:])
        print(f"[batch_probe] N = {n} done", file=sys.stderr, flush=True)
        device = got["device"]
        rows += got["rows"]
    slower = [{"n": r["n"], "b": r["b"], "ensemble_device_us_per_world_step": r["ensemble_device_us_per_world_step"],
               "loop_device_us_per_world_step": r["loop_device_us_per_world_step"]}
              for r in rows if r["ensemble_device_us_per_world_step"] > r["loop_device_us_per_world_step"]]
    perf = [r for r in rows if r["n"] == 250 and r["b"] == 256]
    out = {"tool": "tools/batch_probe.py", "device": device, "dt": DT, "peak_fp32_flops": PEAK_FLOPS,
           "flops_per_interaction": FLOPS_PER_INTERACTION, "rows": rows, "ensemble_slower_per_world_than_loop": slower,
           "n250_b256_device_ratio": perf[0]["device_ratio_ensemble_over_loop"] if perf else None, "failed": failed}
    print(json.dumps(out))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
