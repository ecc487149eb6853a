"""What stepping worlds of DIFFERENT sizes in one ragged ensemble (nb.SimBatch.ragged) costs beside the two things users
could do before; prints ONE JSON line.

Two mixes of synthetic worlds (half of the particles massive):
  chain_mix   8 sizes (200, 230, ..., 410) x 32 members: every member in the one-workgroup chain group
  mixed       128 x 250 + 64 x 1 000 + 32 x 2 000: the chain group and both lane-split groups
Per mix, device time (the ensembles' own event pairs) of a call of STEPS steps, fastest of 5 after a warm-up, the three
ways interleaved, as microseconds per world-step (time / (steps x members)):
  ragged      ONE ragged ensemble, member order interleaved across the sizes
  per_size    one uniform ensemble per size, stepped one after another (their device times added)
  padded      every member padded to the largest size with massless particles far away, in ONE uniform ensemble: the
              workaround that needs no ragged ensemble; it changes the physics only through phantom receivers, and costs
              the largest member's time for every member
The ragged members are compared bitwise with the per-size ensembles' on the way.

    python tools/ragged_probe.py [--out profiles/ragged_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import nbody_amd as nb  # noqa: E402

DT, REPS = 0.01, 5
MIXES = {
    "chain_mix": {"sizes": [(200 + 30 * i, 32) for i in range(8)], "steps": 64},
    "mixed": {"sizes": [(250, 128), (1000, 64), (2000, 32)], "steps": 16},
}


def world(n, seed):
    """n particles, the first n // 2 massive (already partitioned)"""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * 1.0e4
    a[:, 2:4] = rng.standard_normal((n, 2)) * 10
    m = n // 2
    a[:, 7] = 0.5
    a[:m, 7] = 1.5 + 8 * rng.random(m)
    a[:m, 6] = 41.9 * a[:m, 7] ** 3
    return a, m


def padded(a, n):
    """a with massless particles appended up to n: far away and apart from each other, at rest"""
    out = np.zeros((n, 8), dtype=np.float32)
    out[:a.shape[0]] = a
    extra = n - a.shape[0]
    out[a.shape[0]:, 0] = 1.0e9 + 1.0e3 * np.arange(extra)
    out[a.shape[0]:, 1] = 1.0e9
    out[a.shape[0]:, 7] = 0.5
    return out


def probe(name, sizes, steps):
    worlds = {n: [world(n, 7919 * n + b) for b in range(count)] for n, count in sizes}
    order = [(n, b) for b in range(max(c for _, c in sizes)) for n, c in sizes if b < c]   # interleaved across the sizes
    members = len(order)
    largest = max(n for n, _ in sizes)

    ragged = nb.SimBatch.ragged([n for n, _ in order], [worlds[n][b][1] for n, b in order])
    ragged.set_data([worlds[n][b][0] for n, b in order])
    per_size = {}
    for n, count in sizes:
        u = nb.SimBatch(n, [m for _, m in worlds[n]])
        u.set_data(np.stack([p for p, _ in worlds[n]]))
        per_size[n] = u
    pad = nb.SimBatch(largest, [worlds[n][b][1] for n, b in order])
    pad.set_data(np.stack([padded(worlds[n][b][0], largest) for n, b in order]))

    def ragged_ms():
        ragged.update(steps, DT)
        return ragged.last_ms()

    def per_size_ms():
        total = 0.0
        for u in per_size.values():
            u.update(steps, DT)
            total += u.last_ms()
        return total

    def padded_ms():
        pad.update(steps, DT)
        return pad.last_ms()

    ways = {"ragged": ragged_ms, "per_size": per_size_ms, "padded": padded_ms}
    for fn in ways.values():
        fn()   # warm-up
    ms = {k: [] for k in ways}
    for _ in range(REPS):
        for k, fn in ways.items():
            ms[k].append(fn())
    # same calls on both sides so far: the ragged members must be the per-size members, bit for bit
    got = ragged.get_data()
    want = {n: u.get_data() for n, u in per_size.items()}
    assert all(got[i].tobytes() == want[n][b].tobytes() for i, (n, b) in enumerate(order)), "ragged members differ from per-size ones"
    shape = ragged.launch_shape()["groups"]
    ragged.close()
    pad.close()
    for u in per_size.values():
        u.close()
    row = {"mix": name, "sizes": [[n, c] for n, c in sizes], "members": members, "steps": steps, "groups": shape}
    for k, v in ms.items():
        row[k + "_us_per_world_step"] = round(min(v) * 1e3 / (steps * members), 4)
        row[k + "_call_us"] = round(min(v) * 1e3, 1)
    row["ragged_over_per_size"] = round(min(ms["ragged"]) / min(ms["per_size"]), 4)
    row["ragged_over_padded"] = round(min(ms["ragged"]) / min(ms["padded"]), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert nb.device_count() >= 1, "ragged_probe needs an MI355X"
    out = {"tool": "ragged_probe", "device": nb.device_info(),
           "rows": [probe(name, mix["sizes"], mix["steps"]) for name, mix in MIXES.items()]}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
