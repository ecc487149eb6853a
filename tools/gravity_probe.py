"""Cost of the acceleration map (nb_hip_acceleration_map) on the worlds users run, against the route that existed before it
and against the potential map of the same view, and the sweep behind the threshold between the two kernel shapes; prints ONE
JSON line.

maps        for N = 6 000 (the GUI's world) and 2^20 (the headline galaxy pair): the map at 1280 x 720 and at 256 x 256
            under the fitted view -- device ms (nb_hip_last_diag_ms) and wall ms of the blocking call, fastest and median of
            --reps after a warm-up call, pairs per second of the fastest device time, and device cycles per wave-interaction
            (one source against the 64 lanes' one sample each) at the 2.4 GHz the chip is specified for, over its 1 024 SIMDs.
potential_map   nb_hip_potential_map of the same view, device ms fastest of --reps, and the ratio.
old_route   the same map with the calls that existed before: get_data(), a second SimPipeline of particles + one massless
            particle of radius s per pixel (created, set_data), one dt = 0 step (device ms and wall ms), get_data() of
            that pipeline, destroyed; each part's wall ms and the total, median of --reps.  Its result agrees with the map's
            (a sanity check relative to the image's largest component; the tolerance proper is tests/test_gpu_gravity.py's).
shapes      the two kernel shapes (the "gravity_shape" tuning hook) across M = 64 ... 4 096 at two fixed images, 256 x 256
            and 1280 x 720: device ms of each, fastest of --reps alternating, and the device ms of what "auto" ran.
yardstick   tests/test_gpu_gravity_perf.py's pair: the 256 x 128 map over M = N = 4 096 against one dt = 0 step of the
            augmented pipeline, fastest of 5 alternating, and their ratio.

    python tools/gravity_probe.py [--reps 5] [--out profiles/gravity_probe.json]
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
SIMDS, CLOCK_HZ = 1024, 2.4e9


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


def time_call(sim, fn, reps):
    fn()  # warm-up
    dev, wl = [], []
    for _ in range(reps):
        _, w = wall(fn)
        wl.append(w)
        dev.append(sim.last_diag_ms())
    return dev, wl


def agrees(img, step):
    """the step kernel sums the same pairs in another order: agreement to 1e-3 of the image's largest component"""
    scale = float(np.max(np.abs(img)))
    return float(np.max(np.abs(img.astype(np.float64) - step.astype(np.float64)))) <= 1e-3 * scale


def old_route(sim, m, view, reps, want):
    rows = []
    for _ in range(reps + 1):      # the first round is the warm-up
        part, t_get = wall(sim.get_data)
        both, t_host = wall(lambda: augmented(part, pixel_points(view)))

        def build():
            s2 = nb.SimPipeline(both.shape[0], m)
            s2.configure(timing=1)
            s2.set_data(both)
            return s2
        s2, t_build = wall(build)
        _, t_step = wall(lambda: s2.update(1, 0.0))
        dev = s2.last_step_ms()[0]
        back, t_back = wall(s2.get_data)
        _, t_close = wall(s2.close)
        assert agrees(want, back[part.shape[0]:, 4:6])
        rows.append({"get_data_wall_ms": t_get, "host_concat_wall_ms": t_host, "second_pipeline_wall_ms": t_build,
                     "step_wall_ms": t_step, "step_device_ms": dev, "read_back_wall_ms": t_back, "destroy_wall_ms": t_close,
                     "total_wall_ms": t_get + t_host + t_build + t_step + t_back + t_close})
    rows = rows[1:]
    return {k: round(statistics.median(r[k] for r in rows), 4) for k in rows[0]}


def probe_world(name, a, reps):
    part, m, views = partition(a)
    sim = nb.SimPipeline(part.shape[0], m)
    sim.set_data(part)
    out = {"world": name, "n": int(part.shape[0]), "mass_len": m, "maps": []}
    for size in ((1280, 720), (256, 256)):
        view = views[size]
        dev, wl = time_call(sim, lambda: sim.acceleration_map(view, SOFT), reps)
        phi_dev, _ = time_call(sim, lambda: sim.potential_map(view, SOFT), reps)
        pairs = size[0] * size[1] * m
        row = {"width": size[0], "height": size[1], "device_ms_best": round(min(dev), 4), "device_ms_median": round(statistics.median(dev), 4),
               "wall_ms_best": round(min(wl), 4), "wall_ms_median": round(statistics.median(wl), 4),
               "pairs": pairs, "pairs_per_s": pairs / (min(dev) * 1e-3),
               "cycles_per_wave_interaction_at_2.4GHz": round(min(dev) * 1e-3 * CLOCK_HZ * SIMDS / (pairs / 64.0), 2),
               "potential_map_device_ms_best": round(min(phi_dev), 4), "over_potential_map": round(min(dev) / min(phi_dev), 4)}
        row["old_route"] = old_route(sim, m, view, max(2, reps // 2), sim.acceleration_map(view, SOFT).reshape(-1, 2))
        row["old_route_over_map_wall"] = round(row["old_route"]["total_wall_ms"] / row["wall_ms_median"], 3)
        row["old_step_over_map_device"] = round(row["old_route"]["step_device_ms"] / row["device_ms_best"], 3)
        out["maps"].append(row)
    sim.close()
    return out


def sweep_shapes(reps):
    rng = np.random.default_rng(5)
    out = []
    for width, height in ((256, 256), (1280, 720)):
        view = nb.RenderView.make((0.0, 0.0), (width * 0.5, height * 0.5), 0.05, width, height, 1.0)
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
                sim.configure(gravity_shape=shape)
                imgs[shape] = sim.acceleration_map(view, SOFT)      # warm-up
            assert imgs[1].tobytes() == imgs[2].tobytes()
            for _ in range(reps):
                for shape in (1, 2):
                    sim.configure(gravity_shape=shape)
                    sim.acceleration_map(view, SOFT)
                    t[shape].append(sim.last_diag_ms())
            sim.configure(gravity_shape=0)
            auto_img = sim.acceleration_map(view, SOFT)
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
    aug.configure(timing=1)
    aug.set_data(both)
    img = sim.acceleration_map(view, SOFT).reshape(-1, 2)
    aug.update(1, 0.0)
    assert agrees(img, aug.get_data()[4096:, 4:6])
    t_map, t_ref = [], []
    for _ in range(5):
        sim.acceleration_map(view, SOFT)
        t_map.append(sim.last_diag_ms())
        aug.update(1, 0.0)
        t_ref.append(aug.last_step_ms()[0])
    shape = aug.launch_shape()
    sim.close()
    aug.close()
    return {"map_ms": [round(t, 4) for t in t_map], "step_ms": [round(t, 4) for t in t_ref], "step_launch_shape": shape,
            "ratio_of_bests": round(min(t_map) / min(t_ref), 4), "yardstick_spread": round((max(t_ref) - min(t_ref)) / min(t_ref), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert nb.device_count() >= 1, "gravity_probe needs an MI355X"
    worlds = [("gui_6000x3", nb.make_galaxies(6000, 3, seed=11037)),
              ("galaxies_2^20x2_seed11037", nb.make_galaxies(1 << 20, 2, seed=11037))]
    out = {"tool": "gravity_probe", "device": nb.device_info(), "softening": SOFT, "reps": args.reps,
           "worlds": [probe_world(k, a, args.reps) for k, a in worlds], "shapes": sweep_shapes(args.reps), "yardstick": yardstick()}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
