"""The Python binding's surface (no GPU): the public names, what callers reach through `nb.`, the read-only methods written
once for SimPipeline / SimBatch / World / WorldBatch, and what each of them returns -- type, dtype and shape, on the host path
of a World / WorldBatch that never stepped on the device.  tests/test_gpu_binding_surface.py runs the same table on the seam.

tests/binding_surface.json is the record the first test compares with: regenerate it from the repository root with

    import inspect, json, nbody_amd as nb
    classes = ("SimPipeline", "SimBatch", "World", "WorldBatch", "LocalShardGroup")
    methods = {c: {m: str(inspect.signature(getattr(getattr(nb, c), m))) for m in dir(getattr(nb, c))
                   if not m.startswith("_") and callable(getattr(getattr(nb, c), m))} for c in classes}
    names = sorted(n for n in dir(nb) if not n.startswith("_"))
    json.dump({"names": names, "methods": methods}, open("tests/binding_surface.json", "w"), indent=1, sort_keys=True)
"""
import glob
import inspect
import json
import os
import re

import numpy as np
import pytest

import nbody_amd as nb

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CLASSES = ("SimPipeline", "SimBatch", "World", "WorldBatch")
READS = ("energy", "potential", "potential_at", "potential_map", "acceleration_at", "acceleration_map", "tidal_at", "tidal_map",
         "profile", "pair_counts", "neighbours", "bounds", "render_counts", "render")


# ---- 1. public names and signatures ---------------------------------------------------------------------------------------------

def recorded():
    with open(os.path.join(ROOT, "tests", "binding_surface.json")) as f:
        return json.load(f)


def test_every_recorded_public_name_is_still_there():
    missing = [n for n in recorded()["names"] if not hasattr(nb, n)]
    assert not missing, missing


def test_every_recorded_method_keeps_its_signature():
    """Names, order and defaults of every parameter.  One spelling is not held: the record has `view` on the single-world classes
    and `views` on the ensembles for the first parameter of the maps and renders, and one function cannot carry both; every
    caller passes it by position."""
    one_spelling = lambda sig: re.sub(r"\bviews\b", "view", sig)      # noqa: E731
    rec = recorded()["methods"]
    assert sorted(rec) == sorted(CLASSES + ("LocalShardGroup",))
    for cls, methods in rec.items():
        assert set(READS) <= set(methods) or cls == "LocalShardGroup", cls
        for name, sig in methods.items():
            assert one_spelling(str(inspect.signature(getattr(getattr(nb, cls), name)))) == one_spelling(sig), (cls, name)


# ---- 2. callers resolve ---------------------------------------------------------------------------------------------------------

def callers():
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")))
    return files + [os.path.join(ROOT, "bench.py")]


def test_every_name_a_caller_reaches_through_the_package_exists():
    import importlib.util
    unknown = set()
    for path in callers():
        text = open(path).read()
        if not re.search(r"import nbody_amd as nb\b", text):
            continue
        for name in set(re.findall(r"(?<![A-Za-z0-9_.])nb\.([A-Za-z_][A-Za-z0-9_]*)", text)):
            if not hasattr(nb, name) and importlib.util.find_spec("nbody_amd." + name) is None:
                unknown.add((os.path.relpath(path, ROOT), name))
    assert not unknown, sorted(unknown)


# ---- 3. written once ------------------------------------------------------------------------------------------------------------

def test_the_read_only_methods_are_written_once():
    """Cannot pass before the four copies were merged: skipped where the package has no reads module."""
    if not os.path.exists(os.path.join(ROOT, "nbody_amd", "reads.py")):
        pytest.skip("this binding still writes the read-only methods once per class")
    for name in READS:
        for cls in CLASSES:
            assert name not in vars(getattr(nb, cls)), (cls, name)
        assert len({id(getattr(getattr(nb, cls), name)) for cls in CLASSES}) == 1, name


# ---- 4. return conventions ------------------------------------------------------------------------------------------------------

N, MASSIVE, B = 5, 3, 2
SIZES = (5, 1)                  # the ragged ensemble; its one-particle member has no neighbour
POINTS, W, H, BINS = 2, 3, 2, 2
EDGES = np.array([0.25, 1.0, 2.5], dtype=np.float32)
SOFTENING, RADIUS = 0.05, 1.0
ENERGY_KEYS = {"kinetic", "potential", "total", "mass", "momentum", "angular_momentum", "center_of_mass"}


def particles(seed, n=N, massive=MASSIVE):
    """(n, 8), the massive particles first: already in the order a World keeps and a SimPipeline wants."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2], a[:, 2:4] = rng.uniform(-1.0, 1.0, (n, 2)), rng.uniform(-0.5, 0.5, (n, 2))
    a[:massive, 6], a[:, 7] = rng.uniform(0.5, 2.0, massive), 0.01
    return a


def view(zoom):
    return nb.RenderView.make((0.0, 0.0), (W / 2.0, H / 2.0), zoom, W, H, 1.0)


def arguments(per_member):
    """(view(s), points, centre) for a single world or shared by the members of an ensemble, or one of each per member."""
    pts = np.random.default_rng(7).uniform(-1.0, 1.0, (B, POINTS, 2)).astype(np.float32)
    if per_member:
        return [view(1.0), view(0.75)], pts, np.array([[0.0, 0.0], [0.1, -0.2]], dtype=np.float32)
    return view(1.0), pts[0], (0.0, 0.0)


def arguments_of(b):
    """What member b sees of arguments(per_member=True)."""
    views, pts, centres = arguments(True)
    return views[b], pts[b], centres[b]


def reads(obj, views, points, centre, renders=True):
    """Every read-only method, with each argument that changes what comes back given and omitted.  renders=False leaves out
    bounds / render_counts / render: the library does not render ragged ensembles and ends the process when asked to."""
    values = {
        "energy": obj.energy(),
        "potential": obj.potential(),
        "potential_at": obj.potential_at(points, SOFTENING),
        "potential_map": obj.potential_map(views, SOFTENING),
        "acceleration_at": obj.acceleration_at(points, SOFTENING),
        "acceleration_map": obj.acceleration_map(views, SOFTENING),
        "tidal_at": obj.tidal_at(points, SOFTENING),
        "tidal_map": obj.tidal_map(views, SOFTENING),
        "profile": obj.profile(EDGES, centre=centre, weights="number"),
        "profile unplaced": obj.profile(EDGES, centre=centre, return_unplaced=True),
        "pair_counts": obj.pair_counts(EDGES, classes="all"),
        "pair_counts unplaced": obj.pair_counts(EDGES, return_unplaced=True),
        "neighbours": obj.neighbours(),
        "neighbours radius": obj.neighbours(RADIUS, "all", "massive"),
    }
    if renders:
        values.update({
            "bounds": obj.bounds(),
            "render_counts": obj.render_counts(views),
            "render": obj.render(views),
            "render palette": obj.render(views, palette=nb.default_palette()),
        })
    return values


class A:
    """An array of one dtype and shape."""

    def __init__(self, dtype, *shape):
        self.dtype, self.shape = np.dtype(dtype), shape


f32, f64, u8, u32, u64 = np.float32, np.float64, np.uint8, np.uint32, np.uint64

SINGLE = {
    "energy": dict,
    "potential": A(f32, N),
    "potential_at": A(f32, POINTS),
    "potential_map": A(f32, H, W),
    "acceleration_at": A(f32, POINTS, 2),
    "acceleration_map": A(f32, H, W, 2),
    "tidal_at": A(f32, POINTS, 3),
    "tidal_map": A(f32, H, W, 3),
    "profile": A(f64, BINS + 2, 6),
    "profile unplaced": (A(f64, BINS + 2, 6), int),
    "pair_counts": A(u64, BINS + 2, 3),
    "pair_counts unplaced": (A(u64, BINS + 2, 3), A(u64, 3)),
    "neighbours": (A(f32, N), A(u32, N)),
    "neighbours radius": (A(f32, N), A(u32, N), A(u32, N)),
    "bounds": A(f32, 4),
    "render_counts": A(u32, 3, H, W),
    "render": A(u8, H, W, 4),
    "render palette": A(u8, H, W, 4),
}

UNIFORM = {
    "energy": [dict] * B,
    "potential": A(f32, B, N),
    "potential_at": A(f32, B, POINTS),
    "potential_map": A(f32, B, H, W),
    "acceleration_at": A(f32, B, POINTS, 2),
    "acceleration_map": A(f32, B, H, W, 2),
    "tidal_at": A(f32, B, POINTS, 3),
    "tidal_map": A(f32, B, H, W, 3),
    "profile": A(f64, B, BINS + 2, 6),
    "profile unplaced": (A(f64, B, BINS + 2, 6), A(u32, B)),
    "pair_counts": A(u64, B, BINS + 2, 3),
    "pair_counts unplaced": (A(u64, B, BINS + 2, 3), A(u64, B, 3)),
    "neighbours": (A(f32, B, N), A(u32, B, N)),
    "neighbours radius": (A(f32, B, N), A(u32, B, N), A(u32, B, N)),
    "bounds": A(f32, B, 4),
    "render_counts": A(u32, B, 3, H, W),
    "render": A(u8, B, H, W, 4),
    "render palette": A(u8, B, H, W, 4),
}

# a ragged ensemble keeps every shape but those with one entry per particle: lists of per-member arrays; it is not rendered
RAGGED = {label: want for label, want in UNIFORM.items() if label not in ("bounds", "render_counts", "render", "render palette")}
RAGGED.update({
    "potential": [A(f32, n) for n in SIZES],
    "neighbours": ([A(f32, n) for n in SIZES], [A(u32, n) for n in SIZES]),
    "neighbours radius": ([A(f32, n) for n in SIZES], [A(u32, n) for n in SIZES], [A(u32, n) for n in SIZES]),
})


def check(got, want, where):
    if isinstance(want, (tuple, list)):
        assert type(got) is type(want) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            check(g, w, where + (i,))
            if isinstance(want, list) and isinstance(w, A):
                assert g.flags.owndata, where          # a member of a ragged result is a copy, not a view of the packed array
    elif want is dict:
        assert type(got) is dict and set(got) == ENERGY_KEYS, where
    elif want is int:
        assert type(got) is int, where
    else:
        assert type(got) is np.ndarray and got.dtype == want.dtype and got.shape == want.shape, (where, got)


def check_table(values, table, what):
    assert set(values) == set(table)
    for label, want in table.items():
        check(values[label], want, (what, label))


def member(value, b):
    return tuple(member(v, b) for v in value) if isinstance(value, tuple) else value[b]


def same(a, b):
    """bit for bit"""
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    return a == b


def check_members(values, singles, what):
    for b, alone in enumerate(singles):
        for label in SINGLE:
            assert same(member(values[label], b), alone[label]), (what, label, b)


def check_the_lone_particle(values):
    for label in ("neighbours", "neighbours radius"):
        got = member(values[label], 1)
        assert np.isposinf(got[0][0]) and got[1][0] == nb.NB_NEIGH_NONE and (len(got) == 2 or got[2][0] == 0), label


def surface_of(single, uniform, ragged):
    """The whole of part 4 for three factories: single(particles), uniform((B, N, 8)), ragged(list of members)."""
    states = [particles(1), particles(2)]
    alone_shared, alone_own = [], []
    for b, a in enumerate(states):
        w = single(a)
        alone_shared.append(reads(w, *arguments(False)))
        alone_own.append(reads(w, *arguments_of(b)))
        w.close()
        check_table(alone_shared[b], SINGLE, "single")
        check_table(alone_own[b], SINGLE, "single")
    batch = uniform(np.stack(states))
    for per_member, singles in ((False, alone_shared), (True, alone_own)):
        values = reads(batch, *arguments(per_member))
        check_table(values, UNIFORM, ("uniform", per_member))
        check_members(values, singles, ("uniform", per_member))
    batch.close()
    batch = ragged([particles(1), particles(3, 1, 1)])
    for per_member in (False, True):
        values = reads(batch, *arguments(per_member), renders=False)
        check_table(values, RAGGED, ("ragged", per_member))
        check_the_lone_particle(values)
    batch.close()


def test_what_every_read_returns_on_the_host_path():
    surface_of(nb.World, nb.WorldBatch, nb.WorldBatch.ragged)


def test_bad_arguments_raise_the_same_errors():
    w, wb = nb.World(particles(1)), nb.WorldBatch(np.stack([particles(1), particles(2)]))
    v = view(1.0)
    cases = [
        (lambda: w.potential_at(np.zeros((2, 3)), SOFTENING), "points must have shape (n, 2)"),
        (lambda: w.tidal_at(np.zeros((B, 2, 2)), SOFTENING), "points must have shape (n, 2)"),
        (lambda: wb.acceleration_at(np.zeros((3, 2, 2)), SOFTENING), "points must have shape (n, 2) or (2, n, 2)"),
        (lambda: wb.potential_map([v] * 3, SOFTENING), "expected one RenderView or 2 of them"),
        (lambda: wb.render([v], None), "expected one RenderView or 2 of them"),
        (lambda: w.profile([1.0]), "edges must be a sequence of at least two radii"),
        (lambda: w.profile(EDGES, weights="charge"), 'weights must be "mass" or "number"'),
        (lambda: w.profile(EDGES, centre=np.zeros((2, 2))), "centre and centre_velocity must have shape (2,)"),
        (lambda: wb.profile(EDGES, centre=np.zeros((3, 2))), "centre and centre_velocity must have shape (2,) or (2, 2)"),
        (lambda: wb.pair_counts([1.0]), "edges must be a sequence of at least two radii"),
        (lambda: w.pair_counts(EDGES, classes="xx"), 'classes must be a subset of "mm", "mt", "tt", or "all"'),
        (lambda: wb.pair_counts(EDGES, classes=()), 'classes must name at least one of "mm", "mt", "tt"'),
        (lambda: w.neighbours(receivers="mm"), 'receivers must be "massive", "massless" or "all"'),
        (lambda: wb.neighbours(sources=1.5), 'sources must be "massive", "massless" or "all"'),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    # integers pass through: the library names the fault, and these are the values the names stand for
    assert same(w.profile(EDGES, weights=nb.NB_PROFILE_BY_NUMBER), w.profile(EDGES, weights="number"))
    assert same(wb.pair_counts(EDGES, classes=nb.NB_PAIRS_ALL), wb.pair_counts(EDGES, classes="all"))
    assert same(w.neighbours(None, nb.NB_NEIGH_ALL, nb.NB_NEIGH_MASSIVE), w.neighbours(None, "all", "massive"))
    w.close()
    wb.close()
