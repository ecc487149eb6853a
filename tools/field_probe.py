"""Cost of the potential map (nb_hip_potential_map) on the worlds users run, against the route that existed before it, and
the sweep behind the threshold between the two kernel shapes; prints ONE JSON line.

maps        for N = 6 000 (the GUI's world), 65 536 and 2^20 (the headline galaxy pair): the map at 1280 x 720 and at
            256 x 256 under the fitted view -- device ms (nb_hip_last_diag_ms) and wall ms of the blocking call, best and
            median of --reps after a warm-up call, and pairs per second of the best device time.
old_route   the same map with the calls that existed before: get_data(), a second SimPipeline of particles + one massless
            particle per pixel (created, set_data), potential() (device ms and wall ms), destroyed; each part's wall ms and
            the total, median of --reps.  Its bits equal the map's (checked).
shapes      the two kernel shapes (the "field_shape" tuning hook) across M = 64 ... 4 096 at two fixed images, 256 x 256 and
            1280 x 720: device ms of each, best of --reps alternating, and the device ms of what "auto" ran.
yardstick   tests/test_gpu_field_perf.py's pair: the 256 x 128 map over M = N = 4 096 against potential() of the augmented
            pipeline, best of 5 alternating, and their ratio.

    python tools/field_probe.py [--reps 5] [--out profiles/field_probe.json]
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

SOFT = 0.75


def partition(a):
    """mass > 0 first, the World's own order (CreateWorld), read back without touching the device"""
    w = nb.World(a)
    p = w.particles()
    view = {(wd, ht): w.fit_view(wd, ht) for wd, ht in ((1280, 720), (256, 256), (256, 128))}
    w.close()
    return p, int((p[:, 6] > 0).sum()), view


def pixel_points(view):
    f = np.float32
    xs = ((np.arange(view.width, dtype=np.float32) + f(0.5)) - f(view.offset[0])) / f(view.zoom) + f(view.target[0])
    ys = ((np.arange(view.height, dtype=np.float32) + f(0.5)) - f(view.offset[1])) / f(view.zoom) + f(view.target[1])
    pts = np.empty((view.height, view.width, 2), dtype=np.float32)
    pts[:, :, 0], pts[:, :, 1] = xs[None, :], ys[:, None]
    return pts.reshape(-1, 2)


def augmented(part, pts):
    extra = np.zeros((pts.shape[0], 8), dtype=np.float32)
    extra[:, 0:2], extra[:, 7] = pts, SOFT
    return np.concatenate([part, extra], axis=0)


def wall(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def time_map(sim, view, reps):
    sim.potential_map(view, SOFT)  # warm-up
    dev, wl = [], []
    for _ in range(reps):
        _, w = wall(lambda: sim.potential_map(view, SOFT))
        wl.append(w)
        dev.append(sim.last_diag_ms())
    return dev, wl


def old_route(sim, m, view, reps, want):
    rows = []
    for _ in range(reps + 1):      # the first round is the warm-up
        part, t_get = wall(sim.get_data)
        both, t_host = wall(lambda: augmented(part, pixel_points(view)))

        def build():
            s2 = nb.SimPipeline(both.shape[0], m)
            s2.set_data(both)
            return s2
        s2, t_build = wall(build)
        phi, t_phi = wall(s2.potential)
        dev = s2.last_diag_ms()
        _, t_close = wall(s2.close)
        assert phi[part.shape[0]:].tobytes() == want.tobytes()
        rows.append({"get_data_wall_ms": t_get, "host_concat_wall_ms": t_host, "second_pipeline_wall_ms": t_build,
                     "potential_wall_ms": t_phi, "potential_device_ms": dev, "destroy_wall_ms": t_close,
                     "total_wall_ms": t_get + t_host + t_build + t_phi + t_close})
    rows = rows[1:]
    return {k: round(statistics.median(r[k] for r in rows), 4) for k in rows[0]}


def probe_world(name, a, reps):
    part, m, views = partition(a)
    sim = nb.SimPipeline(part.shape[0], m)
    sim.set_data(part)
    out = {"world": name, "n": int(part.shape[0]), "mass_len": m, "maps": []}
    for size in ((1280, 720), (256, 256)):
        view = views[size]
        dev, wl = time_map(sim, view, reps)
        pairs = size[0] * size[1] * m
        row = {"width": size[0], "height": size[1], "device_ms_best": round(min(dev), 4), "device_ms_median": round(statistics.median(dev), 4),
               "wall_ms_best": round(min(wl), 4), "wall_ms_median": round(statistics.median(wl), 4),
               "pairs": pairs, "pairs_per_s": pairs / (min(dev) * 1e-3)}
        row["old_route"] = old_route(sim, m, view, max(2, reps // 2), sim.potential_map(view, SOFT).reshape(-1))
        row["old_route_over_map_wall"] = round(row["old_route"]["total_wall_ms"] / row["wall_ms_median"], 3)
        out["maps"].append(row)
    sim.close()
    return out


def sweep_shapes(reps):
    rng = np.random.default_rng(5)
    out = []
    for width, height in ((256, 256), (1280, 720)):
        view = nb.RenderView.make((0.0, 0.0), (width * 0.5, height * 0.5), 0.05, width, height, 1.0)
        rows = []
        for m in (64, 128, 256, 512, 1024, 1536, 1792, 2048, 2304, 3072, 4096):
            a = np.zeros((m, 8), dtype=np.float32)
            a[:, 0:2] = rng.standard_normal((m, 2)) * 1.0e3
            a[:, 6], a[:, 7] = 100.0, 1.0
            sim = nb.SimPipeline(m, m)
            sim.set_data(a)
            t = {1: [], 2: []}
            imgs = {}
            for shape in (1, 2):
                sim.configure(field_shape=shape)
                imgs[shape] = sim.potential_map(view, SOFT)      # warm-up
            assert imgs[1].tobytes() == imgs[2].tobytes()
            for _ in range(reps):
                for shape in (1, 2):
                    sim.configure(field_shape=shape)
                    sim.potential_map(view, SOFT)
                    t[shape].append(sim.last_diag_ms())
            sim.configure(field_shape=0)
            auto_img = sim.potential_map(view, SOFT)
            auto = sim.last_diag_ms()
            assert auto_img.tobytes() == imgs[1].tobytes()
            sim.close()
            split, wave = min(t[1]), min(t[2])
            rows.append({"m": m, "source_blocks": (m + 255) // 256, "split_ms": round(split, 4), "wave_ms": round(wave, 4),
                         "wave_over_split": round(wave / split, 4), "auto_ms": round(auto, 4)})
        out.append({"image": [width, height], "rows": rows})
    return out


def yardstick():
    rng = np.random.default_rng(12)
    a = np.zeros((4096, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((4096, 2)) * 1.0e4
    a[:, 7] = 1.5 + 8 * rng.random(4096)
    a[:, 6] = 41.9 * a[:, 7] ** 3
    part, m, views = partition(a)
    view = views[(256, 128)]
    sim = nb.SimPipeline(4096, m)
    sim.set_data(part)
    both = augmented(part, pixel_points(view))
    aug = nb.SimPipeline(both.shape[0], m)
    aug.set_data(both)
    assert sim.potential_map(view, SOFT).reshape(-1).tobytes() == aug.potential()[4096:].tobytes()
    t_map, t_ref = [], []
    for _ in range(5):
        sim.potential_map(view, SOFT)
        t_map.append(sim.last_diag_ms())
        aug.potential()
        t_ref.append(aug.last_diag_ms())
    sim.close()
    aug.close()
    return {"map_ms": [round(t, 4) for t in t_map], "potential_ms": [round(t, 4) for t in t_ref],
            "ratio_of_bests": round(min(t_map) / min(t_ref), 4), "yardstick_spread": round((max(t_ref) - min(t_ref)) / min(t_ref), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert nb.device_count() >= 1, "field_probe needs an MI355X"
    worlds = [("gui_6000x3", nb.make_galaxies(6000, 3, seed=11037)),
              ("galaxies_65536x2_seed11037", nb.make_galaxies(65536, 2, seed=11037)),
              ("galaxies_2^20x2_seed11037", nb.make_galaxies(1 << 20, 2, seed=11037))]
    out = {"tool": "field_probe", "device": nb.device_info(), "softening": SOFT, "reps": args.reps,
           "worlds": [probe_world(k, a, args.reps) for k, a in worlds], "shapes": sweep_shapes(args.reps), "yardstick": yardstick()}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
