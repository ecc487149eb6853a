"""Cost of the field of every member of a resident ensemble (nb_hip_ensemble_potential_at / _potential_map and the two g
calls) beside the ways there were before; prints ONE JSON line.

Worlds are MakeGalaxiesSeeded(N, 2, seed = member) partitioned by CreateWorld, each stepped 20 times in the ensemble; maps
are taken through each member's own fitted view, probes are 16 points per member.  The cases:
    256 x N = 250   at 64 x 64        the contact sheet of a sweep (what tests/test_gpu_batch_field_perf.py times)
    256 x N = 250   at 16 probes      a few radii in every member
     32 x N = 3 000 at 256 x 256
      4 x N = 3 000 at 1 280 x 720    the corner in which field.hip's source-split shape would win: few members, large maps, 6 blocks
Per case and quantity (Phi, g), after one warm-up call, min and median of 5 blocking calls (wall ms) and the median device ms:
  ensemble        ONE SimBatch call
  pipelines       B resident SimPipelines holding the same worlds, the same call one after another (device ms: their sum)
  readback_host   SimBatch.get_data(), then the host path (a WorldBatch that never stepped); Phi only, timed once (it is
                  float64 on the host cores: seconds for the large maps)
All in one process, alternating.  Every member of the ensemble result is compared bytewise with its pipeline's on the way
("members_bitwise"); the host path is float64 and only has to be close.

    python tools/batch_field_probe.py [--out profiles/batch_field_probe.json]
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

REPS, DT, SOFT, PROBES = 5, 0.01, 0.75, 16
CASES = ((256, 250, 64, 64), (256, 250, 0, 0), (32, 3000, 256, 256), (4, 3000, 1280, 720))   # (B, N, width, height); 0 x 0 = probes


def world(n, seed):
    w = nb.World(nb.make_galaxies(n, 2, seed=seed, own_rng=True))
    part = w.particles()
    w.close()
    return part, int((part[:, 6] > 0).sum())


def timed(fn, device_ms=None, reps=REPS, warm=True):
    out = fn() if warm else None   # warm-up (and buffer growth)
    wall, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        if device_ms:
            dev.append(device_ms())
    row = {"wall_ms_min": round(min(wall), 4), "wall_ms_median": round(statistics.median(wall), 4), "runs": reps}
    if dev:
        row["device_ms_median"] = round(statistics.median(dev), 4)
    return row, out


def probe(count, n, width, height):
    made = [world(n, b + 1) for b in range(count)]
    batch = nb.SimBatch(n, [m for _, m in made])
    batch.set_data(np.stack([p for p, _ in made]))
    batch.update(20, DT)
    state = batch.get_data()
    pipes = []
    for b, (_, m) in enumerate(made):
        pipes.append(nb.SimPipeline(n, m))
        pipes[-1].set_data(state[b])
    row = {"n": n, "count": count, "mass_len_max": max(m for _, m in made)}
    if width:
        row.update(width=width, height=height)
        where = [rr.fit_view(p, width, height) for p in state]
        calls = (("phi", "potential_map"), ("g", "acceleration_map"))
    else:
        row.update(probes=PROBES)
        rng = np.random.default_rng(n)
        where = [(p[rng.integers(0, n, PROBES), 0:2] * np.float32(1.1)).astype(np.float32) for p in state]
        calls = (("phi", "potential_at"), ("g", "acceleration_at"))
    arg = where if width else np.stack(where)
    bitwise = True
    for what, call in calls:
        row[what] = {}
        row[what]["ensemble"], got = timed(lambda: getattr(batch, call)(arg, SOFT), batch.last_diag_ms)
        device = []

        def loop():
            device.clear()
            out = []
            for s, x in zip(pipes, where):
                out.append(getattr(s, call)(x, SOFT))
                device.append(s.last_diag_ms())
            return out

        row[what]["pipelines"], alone = timed(loop, lambda: sum(device))
        bitwise = bitwise and got.tobytes() == np.stack(alone).tobytes()
        row[what]["speedup_vs_pipelines"] = round(row[what]["pipelines"]["wall_ms_min"] / row[what]["ensemble"]["wall_ms_min"], 2)
        row[what]["device_ratio_vs_pipelines"] = round(row[what]["ensemble"]["device_ms_median"] /
                                                       row[what]["pipelines"]["device_ms_median"], 3)
        if what == "phi":
            def readback():
                wb = nb.WorldBatch(batch.get_data())
                out = getattr(wb, call)(arg, SOFT)
                wb.close()
                return out

            row[what]["readback_host"], host = timed(readback, reps=1, warm=False)
            assert np.allclose(host, got, rtol=1e-4, atol=0.0), (count, n, what)
            row[what]["speedup_vs_readback_host"] = round(row[what]["readback_host"]["wall_ms_min"] / row[what]["ensemble"]["wall_ms_min"], 2)
    row["members_bitwise"] = bool(bitwise)
    batch.close()
    for s in pipes:
        s.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert nb.device_count() >= 1, "batch_field_probe needs an MI355X"
    rows = [probe(*case) for case in CASES]
    out = {"tool": "batch_field_probe", "device": nb.device_info(), "reps": REPS, "softening": SOFT,
           "members_bitwise": all(r["members_bitwise"] for r in rows), "rows": rows}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
