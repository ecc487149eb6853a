"""Cost of looking at a resident world (nb_hip_bounds / nb_hip_render_rgba) against reading it back; prints ONE JSON line.

Worlds: MakeGalaxies(N, 2), libc seed 11037, N = 6 000, 65 536 and 2^20.  For each, and for the fitted, edge, mixed and
collapsed views (tests/render_ref.py builds them) at 1280 x 720 and 4096 x 4096: device ms of bounds / clear + splat / disc /
shade (the "render_detail" hook's events, median of 5 after a warm-up call), the wall ms of the blocking render(), the
wall ms of a blocking SimPipeline.get_data() and of the World's page-locked GetWorldParticles after a step (the step + read
minus the same step on a World that never reads back), one step's
device ms, and the A/B behind the splat's merge scheme: the same render with "render_merge" = 0 (one atomic per lane).

    python tools/render_probe.py [--sizes 6000,65536,1048576] [--out profiles/render_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nbody_amd as nb  # noqa: E402
import render_ref as rr  # noqa: E402

REPS = 5


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def timed_render(sim, view):
    sim.render(view)   # warm-up (and buffer growth)
    wall, total, parts = [], [], []
    for _ in range(REPS):
        wall.append(wall_ms(lambda: sim.render(view)))
        t, p = sim.last_render_ms()
        total.append(t)
        parts.append(p)
    med = [statistics.median(p[i] for p in parts) for i in range(4)]
    return {"wall_ms": round(min(wall), 4), "device_ms": round(statistics.median(total), 4), "splat_ms": round(med[1], 4),
            "disc_ms": round(med[2], 4), "shade_ms": round(med[3], 4)}


def probe(n):
    ic = nb.make_galaxies(n, 2, seed=11037)
    w = nb.World(ic)
    part = w.particles()
    m = int((part[:, 6] > 0).sum())
    # the World's own route to a picture: the page-locked read-back of the particle array after a step.  The frame loop's
    # eager read-back folds the copy into the step's own submission, so it is priced as (step + GetWorldParticles) minus the
    # same step on a twin World that never reads back.
    twin = nb.World(ic)
    for x in (w, twin):
        x.update_gpu(0.01, 1)
    w.particles()
    both, alone = [], []
    for _ in range(REPS):
        both.append(wall_ms(lambda: (w.update_gpu(0.01, 1), nb.nbody_lib().GetWorldParticles(w._h, None))))
        alone.append(wall_ms(lambda: twin.update_gpu(0.01, 1)))
    world_wall = [max(min(both) - min(alone), 0.0)]
    w.close()
    twin.close()
    sim = nb.SimPipeline(n, m)
    sim.configure(render_detail=1)
    sim.set_data(part)
    step_ms = []
    for _ in range(REPS + 1):
        sim.update(1, 0.01)
        step_ms.append(sim.last_step_ms()[0])
    step = statistics.median(step_ms[1:])
    sim.get_data()
    get_wall = min(wall_ms(sim.get_data) for _ in range(REPS))
    sim.bounds()
    bounds_wall, bounds_dev = [], []
    for _ in range(REPS):
        bounds_wall.append(wall_ms(sim.bounds))
        bounds_dev.append(sim.last_render_ms()[1][0])
    state = sim.get_data()
    out = {"n": n, "mass_len": m, "step_ms": round(step, 4), "get_data_wall_ms": round(get_wall, 4),
           "world_readback_wall_ms": round(min(world_wall), 4), "bounds_wall_ms": round(min(bounds_wall), 4),
           "bounds_ms": round(statistics.median(bounds_dev), 4), "views": []}
    for width, height in ((1280, 720), (4096, 4096)):
        views = {"fitted": rr.fit_view(state, width, height), "edge": rr.edge_view(state, width, height),
                 "mixed": rr.mixed_view(state, width, height), "collapsed": rr.collapsed_view(state, width, height)}
        for name, view in views.items():
            row = {"view": name, "width": width, "height": height}
            row.update(timed_render(sim, view))
            sim.configure(render_merge=0)
            row["one_atomic_per_lane"] = timed_render(sim, view)
            sim.configure(render_merge=1)
            row["render_over_step"] = round(row["device_ms"] / step, 5)
            row["get_data_over_render_wall"] = round(get_wall / row["wall_ms"], 2)
            out["views"].append(row)
    sim.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="6000,65536,1048576")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert nb.device_count() >= 1, "render_probe needs an MI355X"
    out = {"tool": "render_probe", "device": nb.device_info(), "reps": REPS,
           "worlds": [probe(int(n)) for n in args.sizes.split(",")]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
