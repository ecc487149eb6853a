"""One scratch for every read-only call, on the MI355X: energy, potential, the six field calls, profile, pair_counts,
neighbours, bounds, render_counts and render of a SimPipeline / SimBatch share two device buffers and one host vector, and all
but the last three one interval (nbody_amd/csrc/pipeline_internal.h ReadScratch, read_call).  What that could break is a call
that sees what a call of another kind left behind, or a buffer another call sized.  So one long-lived object makes all its calls
in a fixed order -- fifteen on a pipeline, seventeen on a uniform ensemble (render_counts and render once on the tile path and
once on the global path with its disc list), twelve on a ragged one (which renders nothing, by contract) -- at small sizes, at
large ones and at the small ones again (inside buffers now larger than it needs), and every output must equal, byte
for byte, the same call on a fresh object of the same sizes in the same state -- one fresh object per call.  The two neighbour
calls are the ones that merge into the scratch by atomicMin and atomicAdd: one with a radius, then one without under other masks.
The renders add into a count image: render_counts comes directly behind neighbours, whose all-ones keys lie at the head of the
work buffer, render behind pair_counts and bounds behind tidal_map.  A render call records last_render_ms() and leaves
last_diag_ms() as it was.
The ragged ensemble has a member with no massless particle, for which the second of them has nothing to launch while the
other members do.  The interval must have been recorded by every call that launched something, and cleared by the one that had
nothing to launch.  tests/test_gpu_sequences.py (the reads kinds) issues the same calls in drawn orders, among steps."""
import numpy as np
import pytest

import nbody_amd as nb
from gpu_common import synth

pytestmark = pytest.mark.gpu

DT = 0.01
SOFT = 1.0
R_MAX = 8.0e3      # synth's worlds span 1e4
RADIUS = 600.0     # neighbours: a few inside it in the middle of a world, none at its rim


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def view(width, height):
    return nb.RenderView.make((0.0, 0.0), (0.0, 0.0), 0.01, width, height, 100.0)


def world(n, m, seed=0):
    """n particles in the World's order, exactly the first m of them massive"""
    part, _ = synth(n, frac_massive=1.1, seed=seed + n)
    part[m:, 6] = 0.0
    part[m:, 7] = 0.5
    return part


def pipeline():
    """N = 1100, M = 600: two profile chunks of 1024, three source blocks of 256, nine tiles of 128"""
    s = nb.SimPipeline(1100, 600)
    s.set_data(world(1100, 600))
    s.update(2, DT)
    return s


def uniform():
    mass_lens = [120, 250, 1]
    s = nb.SimBatch(250, mass_lens)
    s.set_data(np.stack([world(250, m, seed=b) for b, m in enumerate(mass_lens)]))
    s.update(2, DT)
    return s


def ragged():
    sizes, mass_lens = [100, 600, 2000, 130], [50, 300, 1000, 130]          # the last member: no massless particle
    s = nb.SimBatch.ragged(sizes, mass_lens)
    s.set_data([world(n, m) for n, m in zip(sizes, mass_lens)])
    s.update(2, DT)
    return s


def points(n):
    rng = np.random.default_rng(n)
    return rng.uniform(-R_MAX, R_MAX, (n, 2)).astype(np.float32)


RENDERS = ("bounds", "render_counts", "render")


def on_global_path(call):
    """the same call of an ensemble with render_mode(1); the mode is set back"""
    def run(s):
        s.render_mode(1)
        try:
            return call(s)
        finally:
            s.render_mode(0)
    return run


def round_calls(make, n_points, map_size, bins):
    """the calls of a round on what `make` makes, in order: (name, call on an object)"""
    pts, v, edges = points(n_points), view(*map_size), nb.profile_edges(0.0, R_MAX, bins)
    behind = {"tidal_map": "bounds", "pair_counts": "render", "neighbours": "render_counts"} if make is not ragged else {}
    calls = []
    for name, call in reads(pts, v, edges):
        calls.append((name, call))
        if name in behind:
            method = behind[name]
            render = (lambda s: s.bounds()) if method == "bounds" else (lambda s, method=method: getattr(s, method)(v))
            calls.append((method, render))
            if make is uniform and method != "bounds":
                calls.append((method + "_global", on_global_path(render)))
    return calls


def reads(pts, v, edges):
    """the twelve calls inside read.iv"""
    return [
        ("energy", lambda s: s.energy()),
        ("potential_at", lambda s: s.potential_at(pts, SOFT)),
        ("tidal_map", lambda s: s.tidal_map(v, SOFT)),
        ("profile", lambda s: s.profile(edges, return_unplaced=True)),
        ("acceleration_at", lambda s: s.acceleration_at(pts, SOFT)),
        ("pair_counts", lambda s: s.pair_counts(edges, classes="all", return_unplaced=True)),
        ("potential", lambda s: s.potential()),
        ("potential_map", lambda s: s.potential_map(v, SOFT)),
        ("tidal_at", lambda s: s.tidal_at(pts, SOFT)),
        ("acceleration_map", lambda s: s.acceleration_map(v, SOFT)),
        ("neighbours", lambda s: s.neighbours(RADIUS)),
        ("neighbours_massless", lambda s: s.neighbours(None, "massless", "massive")),
    ]


SMALL = dict(n_points=1, map_size=(16, 9), bins=4)
LARGE = dict(n_points=300, map_size=(40, 30), bins=64)


def blob(out):
    """every bit of a call's output: energy dicts through their float64 bits, arrays through tobytes()"""
    if isinstance(out, dict):
        return b"".join(np.asarray(out[k], dtype=np.float64).tobytes() for k in sorted(out))
    if isinstance(out, (list, tuple)):
        return b"".join(blob(x) for x in out)
    return np.asarray(out).tobytes()


@pytest.mark.parametrize("make", [pipeline, uniform, ragged])
def test_a_long_lived_object_answers_like_a_fresh_one_after_calls_of_every_other_kind(make):
    calls = [(f"{tag}.{name}", call) for tag, sizes in (("S1", SMALL), ("L", LARGE), ("S2", SMALL)) for name, call in round_calls(make, **sizes)]
    assert len(calls) == 3 * {pipeline: 15, uniform: 17, ragged: 12}[make]
    old = make()
    try:
        for name, call in calls:
            before = old.last_diag_ms()
            got = blob(call(old))
            assert old.last_diag_ms() > 0.0, name
            method = name.split(".")[1].replace("_global", "")
            if method in RENDERS:
                ms = old.last_render_ms()
                if make is pipeline:
                    ms = ms[1][0] if method == "bounds" else ms[0]
                assert ms > 0.0 and old.last_diag_ms() == before, name          # the hook remembers what it said of a recorded pair
            fresh = make()
            try:
                want = blob(call(fresh))
            finally:
                fresh.close()
            assert len(got) > 0 and got == want, name
        nothing = np.empty((0, 2), dtype=np.float32)
        assert old.potential_at(nothing, SOFT).size == 0
        assert old.last_diag_ms() == 0.0
    finally:
        old.close()
