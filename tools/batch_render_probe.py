"""Cost of looking at every member of a resident ensemble (nb_hip_ensemble_bounds / _render_counts / _render_rgba) beside
the ways there were before; prints ONE JSON line.

B = 256 worlds of N = 250, 1 000 and 3 000 (MakeGalaxiesSeeded(N, 2, seed = member), partitioned by CreateWorld), each
stepped 20 times, each shown through its own fitted view at 32 x 32, 64 x 64, 128 x 128 and 256 x 256.  Per (N, tile),
after one warm-up call, min and median of 5 blocking calls (wall ms) and the median device ms of their kernels:
  bounds                   SimBatch.bounds()
  counts / frames          SimBatch.render_counts() / render(): "auto" is what ships; where that is the tile path
                           (tile_path = 1) the same call with render_mode(1), the global path, is timed beside it
  pipelines_frames         B resident SimPipelines holding the same worlds, render() one after another
  readback_host_frames     SimBatch.get_data(), then the host path (a WorldBatch that never stepped) render()
All of them in one process, alternating; the frames of every route are compared bytewise on the way.

--views collapsed shows every member through rr.collapsed_view instead (all of a member's particles in one pixel: the
most adds one word can receive, LDS atomics on the tile path, global atomics without a same-word merge on the global path);
its rows carry "view": "collapsed".

    python tools/batch_render_probe.py [--views collapsed] [--out profiles/batch_render_probe.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nbody_amd as nb  # noqa: E402
import render_ref as rr  # noqa: E402

COUNT, SIZES, TILES, REPS, DT = 256, (250, 1000, 3000), (32, 64, 128, 256), 5, 0.01
VIEWS = {"fitted": rr.fit_view, "collapsed": rr.collapsed_view}


def world(n, seed):
    w = nb.World(nb.make_galaxies(n, 2, seed=seed, own_rng=True))
    part = w.particles()
    w.close()
    return part, int((part[:, 6] > 0).sum())


def timed(fn, device_ms=None):
    out = fn()   # warm-up (and buffer growth)
    wall, dev = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        if device_ms:
            dev.append(device_ms())
    row = {"wall_ms_min": round(min(wall), 4), "wall_ms_median": round(statistics.median(wall), 4)}
    if dev:
        row["device_ms_median"] = round(statistics.median(dev), 4)
    return row, out


def probe(n, count, tiles, kind):
    made = [world(n, b + 1) for b in range(count)]
    batch = nb.SimBatch(n, [m for _, m in made])
    batch.set_data(np.stack([p for p, _ in made]))
    batch.update(20, DT)
    state = batch.get_data()
    pipes = []
    for b, (_, m) in enumerate(made):
        pipes.append(nb.SimPipeline(n, m))
        pipes[-1].set_data(state[b])
    rows = []
    for size in tiles:
        views = [VIEWS[kind](p, size, size) for p in state]
        row = {"n": n, "count": count, "width": size, "height": size}
        if kind != "fitted":
            row["view"] = kind
        row["bounds"], _ = timed(batch.bounds, batch.last_render_ms)
        frames = None
        for what, call in (("counts", batch.render_counts), ("frames", batch.render)):
            row[what] = {}
            batch.render_mode(0)
            row[what]["auto"], got = timed(lambda: call(views), batch.last_render_ms)
            info = batch.last_render_info()
            row[what]["auto"].update(info)
            if info["tile_path"]:
                batch.render_mode(1)
                row[what]["global"], other = timed(lambda: call(views), batch.last_render_ms)
                row[what]["global"].update(batch.last_render_info())
                batch.render_mode(0)
                assert np.array_equal(got, other), (n, size, what)
            frames = got
        row["pipelines_frames"], alone = timed(lambda: [s.render(v) for s, v in zip(pipes, views)])
        assert np.array_equal(frames, np.stack(alone)), (n, size)

        def readback():
            wb = nb.WorldBatch(batch.get_data())
            out = wb.render(views)
            wb.close()
            return out

        row["readback_host_frames"], host = timed(readback)
        assert np.array_equal(frames, host), (n, size)
        best = row["frames"]["auto"]["wall_ms_min"]
        row["frames_speedup_vs_pipelines"] = round(row["pipelines_frames"]["wall_ms_min"] / best, 2)
        row["frames_speedup_vs_readback_host"] = round(row["readback_host_frames"]["wall_ms_min"] / best, 2)
        rows.append(row)
    batch.close()
    for s in pipes:
        s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--count", type=int, default=COUNT)
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--tiles", default=",".join(str(t) for t in TILES))
    ap.add_argument("--views", choices=sorted(VIEWS), default="fitted")
    args = ap.parse_args()
    assert nb.device_count() >= 1, "batch_render_probe needs an MI355X"
    tiles = [int(t) for t in args.tiles.split(",")]
    out = {"tool": "batch_render_probe", "device": nb.device_info(), "reps": REPS,
           "rows": [r for n in args.sizes.split(",") for r in probe(int(n), args.count, tiles, args.views)]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
