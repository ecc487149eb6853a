"""Cost of the tidal map (nb_hip_tidal_map) on the worlds users run, against the acceleration map of the same view and against
the finite-difference route it replaces, the sweep of the two kernel shapes, and the ensemble call against B pipelines; prints
ONE JSON line.

maps        for N = 6 000 (the GUI's world) and 2^20 (the headline galaxy pair): tidal_map at 1280 x 720 and at 256 x 256 under
            the fitted view -- device ms (nb_hip_last_diag_ms) and wall ms of the blocking call, fastest and median of --reps
            after a warm-up call, pairs per second of the fastest device time, and device cycles per wave-interaction (one
            source against the 64 lanes' one sample each) at the 2.4 GHz the chip is specified for, over its 1 024 SIMDs.
acceleration_map    nb_hip_acceleration_map of the same view, device ms fastest of --reps, and the ratio.
finite_differences  the route a caller had before: ONE acceleration_at of the 4 n offset points p +- h e_x, p +- h e_y (device
            and wall ms of that call; the host's differencing of the four results is not counted), and the ratios.
shapes      the two kernel shapes (the "tidal_shape" tuning hook) across M = 64 ... 4 096 at two fixed images, 256 x 256 and
            1280 x 720 (the sizes of tools/gravity_probe.py): device ms of each, fastest of --reps alternating, the device ms
            of what "auto" ran, and per image whether the crossover lies where pick_wave_shape's inherited thresholds put it.
ensemble    B members of N particles (worlds of tools/batch_field_probe.py) after 20 steps: ONE SimBatch.tidal_map against B
            resident SimPipelines called one after another, wall ms and device ms, members compared bytewise.
yardstick   tests/test_gpu_tidal_perf.py's pair: the 256 x 128 map over M = N = 4 096 against acceleration_at of the 4 x 32 768
            offset points, fastest of 5 alternating, and their ratio; the ratio to one acceleration_map.

    python tools/tidal_probe.py [--reps 5] [--out profiles/tidal_probe.json]
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

SOFT, DT = 0.75, 0.01
SIMDS, CLOCK_HZ = 1024, 2.4e9
WAVE_SHAPE_BLOCKS_MAX, WAVE_SHAPE_TILES_MIN = 2, 4096          # nbody_amd/csrc/field_sampler.h pick_wave_shape
ENSEMBLES = ((256, 250, 64, 64), (32, 3000, 256, 256))          # (B, N, width, height)


def partition(a):
    """mass > 0 first, the World's own order (CreateWorld), read back without touching the device"""
    w = nb.World(a)
    p = w.particles()
    view = {(wd, ht): w.fit_view(wd, ht) for wd, ht in ((1280, 720), (256, 256), (256, 128), (64, 64))}
    w.close()
    return p, int((p[:, 6] > 0).sum()), view


def pixel_points(view):
    f = np.float32
    xs = ((np.arange(view.width, dtype=np.float32) + f(0.5)) - f(view.offset[0])) / f(view.zoom) + f(view.target[0])
    ys = ((np.arange(view.height, dtype=np.float32) + f(0.5)) - f(view.offset[1])) / f(view.zoom) + f(view.target[1])
    pts = np.empty((view.height, view.width, 2), dtype=np.float32)
    pts[:, :, 0], pts[:, :, 1] = xs[None, :], ys[:, None]
    return pts.reshape(-1, 2)


def offset_points(pts, h=2.0 ** -4):
    """the 4 n points of central differences: p + h e_x, p - h e_x, p + h e_y, p - h e_y per sample"""
    off = np.array([[h, 0], [-h, 0], [0, h], [0, -h]], dtype=np.float32)
    return np.ascontiguousarray((pts[:, None, :] + off[None, :, :]).reshape(-1, 2))


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def time_call(sim, fn, reps):
    fn()  # warm-up
    dev, wl = [], []
    for _ in range(reps):
        _, w = wall(fn)
        wl.append(w)
        dev.append(sim.last_diag_ms())
    return dev, wl


def probe_world(name, a, reps):
    part, m, views = partition(a)
    sim = nb.SimPipeline(part.shape[0], m)
    sim.set_data(part)
    out = {"world": name, "n": int(part.shape[0]), "mass_len": m, "maps": []}
    for size in ((1280, 720), (256, 256)):
        view = views[size]
        fd_pts = offset_points(pixel_points(view))
        dev, wl = time_call(sim, lambda: sim.tidal_map(view, SOFT), reps)
        g_dev, _ = time_call(sim, lambda: sim.acceleration_map(view, SOFT), reps)
        fd_dev, fd_wl = time_call(sim, lambda: sim.acceleration_at(fd_pts, SOFT), reps)
        pairs = size[0] * size[1] * m
        out["maps"].append({
            "width": size[0], "height": size[1], "device_ms_best": round(min(dev), 4), "device_ms_median": round(statistics.median(dev), 4),
            "wall_ms_best": round(min(wl), 4), "wall_ms_median": round(statistics.median(wl), 4),
            "pairs": pairs, "pairs_per_s": pairs / (min(dev) * 1e-3),
            "cycles_per_wave_interaction_at_2.4GHz": round(min(dev) * 1e-3 * CLOCK_HZ * SIMDS / (pairs / 64.0), 2),
            "acceleration_map_device_ms_best": round(min(g_dev), 4), "over_acceleration_map": round(min(dev) / min(g_dev), 4),
            "finite_differences": {"points": int(fd_pts.shape[0]), "device_ms_best": round(min(fd_dev), 4),
                                   "wall_ms_median": round(statistics.median(fd_wl), 4)},
            "over_finite_differences_device": round(min(dev) / min(fd_dev), 4),
            "over_finite_differences_wall": round(statistics.median(wl) / statistics.median(fd_wl), 4)})
    sim.close()
    return out


def sweep_shapes(reps):
    rng = np.random.default_rng(5)
    out = []
    for width, height in ((256, 256), (1280, 720)):
        view = nb.RenderView.make((0.0, 0.0), (width * 0.5, height * 0.5), 0.05, width, height, 1.0)
        tiles = (width * height + 127) // 128
        rows = []
        for m in (64, 256, 512, 768, 1024, 2048, 4096):
            a = np.zeros((m, 8), dtype=np.float32)
            a[:, 0:2] = rng.standard_normal((m, 2)) * 1.0e3
            a[:, 6], a[:, 7] = 100.0, 1.0
            sim = nb.SimPipeline(m, m)
            sim.set_data(a)
            t = {1: [], 2: []}
            imgs = {}
            for shape in (1, 2):
                sim.configure(tidal_shape=shape)
                imgs[shape] = sim.tidal_map(view, SOFT)      # warm-up
            assert imgs[1].tobytes() == imgs[2].tobytes()
            for _ in range(reps):
                for shape in (1, 2):
                    sim.configure(tidal_shape=shape)
                    sim.tidal_map(view, SOFT)
                    t[shape].append(sim.last_diag_ms())
            sim.configure(tidal_shape=0)
            auto_img = sim.tidal_map(view, SOFT)
            auto = sim.last_diag_ms()
            assert auto_img.tobytes() == imgs[1].tobytes()
            sim.close()
            split, wave = min(t[1]), min(t[2])
            blocks = (m + 255) // 256
            picks_wave = blocks <= WAVE_SHAPE_BLOCKS_MAX and tiles >= WAVE_SHAPE_TILES_MIN
            rows.append({"m": m, "source_blocks": blocks, "split_ms": round(split, 4), "wave_ms": round(wave, 4),
                         "wave_over_split": round(wave / split, 4), "auto_ms": round(auto, 4), "auto_picks_wave": picks_wave,
                         "auto_picks_the_faster": bool((wave < split) == picks_wave)})
        out.append({"image": [width, height], "tiles": tiles, "rows": rows,
                    "crossover_where_the_inherited_thresholds_put_it": all(r["auto_picks_the_faster"] for r in rows)})
    return out


def ensemble(count, n, width, height, reps):
    made = []
    for b in range(count):
        w = nb.World(nb.make_galaxies(n, 2, seed=b + 1, own_rng=True))
        p = w.particles()
        w.close()
        made.append((p, int((p[:, 6] > 0).sum())))
    batch = nb.SimBatch(n, [m for _, m in made])
    batch.set_data(np.stack([p for p, _ in made]))
    batch.update(20, DT)
    state = batch.get_data()
    pipes, views = [], []
    for b, (_, m) in enumerate(made):
        pipes.append(nb.SimPipeline(n, m))
        pipes[-1].set_data(state[b])
        w = nb.World(state[b])
        views.append(w.fit_view(width, height))
        w.close()
    dev, wl = time_call(batch, lambda: batch.tidal_map(views, SOFT), reps)
    got = batch.tidal_map(views, SOFT)
    p_dev, p_wl, alone = [], [], None
    for _ in range(reps + 1):      # the first round is the warm-up
        t0 = time.perf_counter()
        alone, d = [], 0.0
        for s, v in zip(pipes, views):
            alone.append(s.tidal_map(v, SOFT))
            d += s.last_diag_ms()
        p_wl.append((time.perf_counter() - t0) * 1e3)
        p_dev.append(d)
    p_dev, p_wl = p_dev[1:], p_wl[1:]
    bitwise = got.tobytes() == np.stack(alone).tobytes()
    batch.close()
    for s in pipes:
        s.close()
    return {"count": count, "n": n, "width": width, "height": height, "mass_len_max": max(m for _, m in made),
            "ensemble": {"wall_ms_min": round(min(wl), 4), "wall_ms_median": round(statistics.median(wl), 4),
                         "device_ms_median": round(statistics.median(dev), 4)},
            "pipelines": {"wall_ms_min": round(min(p_wl), 4), "wall_ms_median": round(statistics.median(p_wl), 4),
                          "device_ms_median": round(statistics.median(p_dev), 4)},
            "speedup_vs_pipelines": round(min(p_wl) / min(wl), 2),
            "device_ratio_vs_pipelines": round(statistics.median(dev) / statistics.median(p_dev), 3), "members_bitwise": bool(bitwise)}


def yardstick():
    rng = np.random.default_rng(12)
    a = np.zeros((4096, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((4096, 2)) * 1.0e4
    a[:, 7] = 1.5 + 8 * rng.random(4096)
    a[:, 6] = 41.9 * a[:, 7] ** 3
    part, m, views = partition(a)
    view = views[(256, 128)]
    fd_pts = offset_points(pixel_points(view))
    sim = nb.SimPipeline(4096, m)
    sim.set_data(part)
    sim.tidal_map(view, SOFT)
    sim.acceleration_at(fd_pts, SOFT)
    sim.acceleration_map(view, SOFT)
    t_map, t_ref, t_g = [], [], []
    for _ in range(5):
        sim.tidal_map(view, SOFT)
        t_map.append(sim.last_diag_ms())
        sim.acceleration_at(fd_pts, SOFT)
        t_ref.append(sim.last_diag_ms())
        sim.acceleration_map(view, SOFT)
        t_g.append(sim.last_diag_ms())
    sim.close()
    return {"map_ms": [round(t, 4) for t in t_map], "finite_differences_ms": [round(t, 4) for t in t_ref],
            "acceleration_map_ms": [round(t, 4) for t in t_g], "ratio_of_bests": round(min(t_map) / min(t_ref), 4),
            "yardstick_spread": round((max(t_ref) - min(t_ref)) / min(t_ref), 4),
            "over_acceleration_map": round(min(t_map) / min(t_g), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert nb.device_count() >= 1, "tidal_probe needs an MI355X"
    worlds = [("gui_6000x3", nb.make_galaxies(6000, 3, seed=11037)),
              ("galaxies_2^20x2_seed11037", nb.make_galaxies(1 << 20, 2, seed=11037))]
    out = {"tool": "tidal_probe", "device": nb.device_info(), "softening": SOFT, "reps": args.reps,
           "worlds": [probe_world(k, a, args.reps) for k, a in worlds], "shapes": sweep_shapes(args.reps),
           "ensembles": [ensemble(*case, args.reps) for case in ENSEMBLES], "yardstick": yardstick()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
