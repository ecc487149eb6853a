"""Record the bits of the field sampler (nb_hip_potential_at / _map, nb_hip_acceleration_at / _map) on a small fixed grid as
sha256 digests: the anchor tests/test_gpu_field_bits.py holds both kernel shapes of both quantities to.  The g kernels have no
other bitwise anchor outside their own file (the step kernel sums in another order, and v_rsq_f32 has no numpy restatement),
so an edit that moves both shapes' bits together is caught here and nowhere else.

The grid (SOFT = 0.75): worlds tests/test_gpu_gravity.py's world(m, seed=m) for M in SOURCES, probes its points_for cut to
n in COUNTS, one 37 x 7 map under its offset_view, kernel shapes 1 (source split) and 2 (one wave per tile), Phi and g.
    M = 0, 1   no source, a ragged tail only          M = 257    a block edge plus one source
    M = 2049   a partial block in a ninth slot, per = 2, empty trailing slices          M = 4500   per = 3
    n = 1, 129 a lone sample, a tile edge plus one    n = 1000   a partial last workgroup of the wave kernel
The file also holds the digests of the inputs (each world, each probe array), so a changed input shows as such.

After a DELIBERATE change of the kernels' arithmetic, on an MI355X:
    python tools/record_field_bits.py --commit $(git rev-parse HEAD) --out tests/golden/field_bits.json
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import nbody_amd as nb  # noqa: E402

SOURCES = (0, 1, 257, 2049, 4500)
COUNTS = (1, 129, 1000)
IMAGE = (37, 7)
SHAPES = (1, 2)


def digest(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def inputs():
    """{m: (world, probes)}: the builders of tests/test_gpu_gravity.py, untouched"""
    import test_gpu_gravity as tg

    assert tg.SOFT == 0.75 and max(tg.COUNTS) == max(COUNTS)
    out = {}
    for m in SOURCES:
        part = tg.world(m, seed=m)
        out[m] = (part, tg.points_for(part, m))
    return out, tg.offset_view(*IMAGE), tg.SOFT


def input_digests(worlds):
    out = {}
    for m, (part, pts) in worlds.items():
        out[f"world/M{m}"], out[f"probes/M{m}"] = digest(part), digest(pts)
    return out


def result_digests(worlds, view, soft):
    """every cell of the grid on device 0: {"<quantity>/M<m>/shape<s>/<n<n> | map37x7>": sha256 of the raw result bytes}"""
    out = {}
    for m, (part, pts) in worlds.items():
        sim = nb.SimPipeline(part.shape[0], m)
        sim.set_data(part)
        for shape in SHAPES:
            sim.configure(field_shape=shape, gravity_shape=shape)
            for name, at, as_map in (("phi", sim.potential_at, sim.potential_map), ("g", sim.acceleration_at, sim.acceleration_map)):
                for n in COUNTS:
                    out[f"{name}/M{m}/shape{shape}/n{n}"] = digest(at(pts[:n], soft))
                out[f"{name}/M{m}/shape{shape}/map{IMAGE[0]}x{IMAGE[1]}"] = digest(as_map(view, soft))
        sim.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose build runs: recorded in the file's header")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "field_bits.json"))
    args = ap.parse_args()
    assert nb.device_count() >= 1, "record_field_bits needs an MI355X"
    worlds, view, soft = inputs()
    doc = {"what": "sha256 of the raw result bytes of the field sampler on the grid of tools/record_field_bits.py; the project's own "
                   "output on an MI355X, refreshed by that script after a deliberate kernel change",
           "recorded_from_commit": args.commit, "device": nb.device_info(), "softening": soft,
           "inputs": input_digests(worlds), "results": result_digests(worlds, view, soft)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(doc['results'])} result digests, {len(doc['inputs'])} input digests -> {args.out}")


if __name__ == "__main__":
    main()
