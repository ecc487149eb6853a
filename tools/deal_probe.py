#!/usr/bin/env python3
"""Dealt launches against classic ones on ONE box, in one process (the "deal" hook; kernels.hip dealt_kernel).

For each N (default 2^20, the headline world: MakeGalaxies(N, 2), seed 11037) two pipelines on the auto shape, one with
deal = 0 and one with deal = 1, take turns: after 5 warm-up steps each, `--repeats` turns of one 20-step call per pipeline,
classic first.  Reported per N: the kernel milliseconds per step launch of every turn (nb_hip_last_step_ms over its launch
count), median / min / max of both sides, gain = 1 - median(dealt) / median(classic), and the classic side's own spread
(max - min) / median -- the yardstick a gain has to beat.  `--extra a,b,c` repeats the dealt side with that many workgroups
on top of the items ("deal_extra" hook; 0 = the default, items / 32).  The final states of the two sides are compared
bytewise on the way.  `--clocks mean,slowest` records the box's sampler clocks (bench.py --full: roofline.held_clock_ghz,
held_clock_ghz_slowest_xcd) and the gain they predict, 1 - slowest / mean.  One JSON line; `--out` keeps it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import nbody_amd as nb   # noqa: E402


def universe(n):
    w = nb.World(nb.make_galaxies(n, 2, seed=11037))
    part = w.particles()
    w.close()
    return part, int((part[:, 6] > 0).sum())


def pipeline(part, m, **knobs):
    sim = nb.SimPipeline(part.shape[0], m)
    sim.configure(timing=1, **knobs)
    sim.set_data(part)
    sim.update(5, 0.01)
    sim.sync()
    return sim


def turn(sim, steps):
    sim.update(steps, 0.01)
    sim.sync()
    ms, launches = sim.last_step_ms()
    return ms / launches


def stats(v):
    med = statistics.median(v)
    return {"per_launch_ms": [round(x, 5) for x in v], "median": round(med, 5), "min": round(min(v), 5), "max": round(max(v), 5),
            "spread": round((max(v) - min(v)) / med, 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=str(1 << 20))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--extra", default="0", help="comma list of deal_extra values for the dealt side; 0 = items / 32")
    ap.add_argument("--clocks", default="", help="held_clock_ghz,held_clock_ghz_slowest_xcd of this box")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"probe": "deal_probe", "steps_per_call": a.steps, "repeats": a.repeats, "rows": []}
    if a.clocks:
        mean, slow = (float(x) for x in a.clocks.split(","))
        out["held_clock_ghz"], out["held_clock_ghz_slowest_xcd"] = mean, slow
        out["predicted_gain"] = round(1.0 - slow / mean, 5)
    for n in (int(x) for x in a.sizes.split(",")):
        part, m = universe(n)
        for extra in (int(x) for x in a.extra.split(",")):
            classic = pipeline(part, m, deal=0)
            dealt = pipeline(part, m, deal=1, deal_extra=extra)
            c, d = [], []
            for _ in range(a.repeats):
                c.append(turn(classic, a.steps))
                d.append(turn(dealt, a.steps))
            is_dealt, items, extra_groups = dealt.last_deal()
            shape = classic.launch_shape()
            row = {"n": n, "m": m, "shape": shape, "rounds": shape["workgroups"] / 512.0, "dealt": is_dealt, "items": items,
                   "extra": extra_groups, "classic": stats(c), "dealt_launches": stats(d),
                   "bits_identical": classic.get_data().tobytes() == dealt.get_data().tobytes()}
            row["gain"] = round(1.0 - row["dealt_launches"]["median"] / row["classic"]["median"], 6)
            row["gain_over_classic_spread"] = round(row["gain"] / row["classic"]["spread"], 2) if row["classic"]["spread"] > 0 else None
            out["rows"].append(row)
            classic.close()
            dealt.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
