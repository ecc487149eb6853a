"""Non-finite state on the GPU (include/nbody_hip.h and include/nbody_diag.h "Non-finite state"): every step route, the
sharded group and the ensembles against the reference's AVX order class for class, the diagnostics and the field samplers
against the host path class for class, and a plant on one row or in one member changes no bit anywhere else.

The cases and the checkers are tests/nonfinite_cases.py; tests/test_nonfinite_cpu.py shows what the cases do in the oracle and
that the checkers reject an inf turned NaN, a leaked NaN and a finite value off its bound.  A non-finite value is ordinary
data to these kernels: no call here has a loop bound or a termination that depends on a value (the adaptive calls are not
used).  A test walks its whole case list and reports every case that failed, not the first one."""
import numpy as np
import pytest

import nbody_amd as nb
import nonfinite_cases as nc
from field_ref import phi_at_f64
from gpu_common import SHAPES, acc_bound, matched_shape
from gravity_ref import g_at_f64
from sequence_driver import PIPE_ROWS, ebits

pytestmark = pytest.mark.gpu

DT = nc.DT
SOFT = 0.75
SPLIT, WAVE = 1, 2          # the "field_shape" / "gravity_shape" hooks of tests/test_gpu_field.py, tests/test_gpu_gravity.py


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


class Failures:
    """collects (case, what failed) so that one run names every failing case"""

    def __init__(self):
        self.lines = []

    def run(self, label, fn, *args, **kw):
        try:
            fn(*args, **kw)
        except AssertionError as e:
            self.lines.append(f"{label}: {str(e).splitlines()[0] if str(e) else 'assertion'}")

    def done(self):
        assert not self.lines, f"{len(self.lines)} failed:\n" + "\n".join(self.lines)


def pipeline(n, m, **knobs):
    sim = nb.SimPipeline(n, m)
    sim.configure(**knobs)
    return sim


def steps_of(sim, p, n):
    sim.set_data(p)
    sim.update(n, DT)
    return sim.get_data()


# ---- the step routes ------------------------------------------------------------------------------------------------------------

assert (1, 1) in SHAPES and (2, 16) in SHAPES

# name -> (N, massive fraction, knobs): the smallest world at which the route exists.  Classic at 700 so that a w = 1 slice
# spans three blocks of 256 sources (two with M = 435); lanes = 1 keeps the lane-split route, which auto takes here, away.
ROUTES = {}
for _tag, _frac in (("M435", 0.6), ("M700", 1.0)):
    for _k, _w in ((1, 1), (2, 16)):
        for _v in (0, 1):
            ROUTES[f"classic-k{_k}w{_w}-variant{_v}-{_tag}"] = (700, _frac, dict(k=_k, w=_w, variant=_v, lanes=1))
ROUTES["lanes4-w8-900"] = PIPE_ROWS["lanes4-w8-900"]
ROUTES["lanes8-w16-900"] = (900, 0.4, dict(lanes=8, w=16))
ROUTES["chain-200"] = (200, 0.5, dict(fused_chain=1))
ROUTES["chain-333"] = (333, 0.5, dict(fused_chain=1))
ROUTES["split3-finish-700"] = (700, 1.0, dict(PIPE_ROWS["split3-finish-9000"][2], lanes=1))
ROUTES["fused-finish-700"] = (700, 1.0, dict(PIPE_ROWS["fused-finish-9000"][2], split=3))
ROUTES["passes2-1500"] = PIPE_ROWS["passes2-1500"]
ROUTES["auto-700"] = (700, 0.6, dict(graph=0))


def check_route_taken(sim, knobs, steps):
    shape = sim.launch_shape()
    if knobs.get("fused_chain") == 1:
        assert sim.fused_steps() == (steps if steps >= 2 else 0)          # a one-step call makes a plain launch
        return
    if "lanes" in knobs:
        assert shape["lanes"] == knobs["lanes"], shape
    for key in ("k", "w", "split"):
        if key in knobs and shape["lanes"] == 1:
            assert shape[key] == knobs[key], shape
    if "variant" in knobs:
        assert shape["variant"] == ("smem" if knobs["variant"] else "lds"), shape
    if "fused_finish" in knobs:
        assert (sim.finish_launches() == 0) == (knobs["fused_finish"] == 1), sim.finish_launches()


def check_case(case, part, m, one, two, twin=None):
    """one / two: the state under test one and two steps after the planted world `part`; twin: the same for the world whose
    plant is an ordinary tracer instead (containment plants)."""
    n = part.shape[0]
    min_rows = n - 1 if case.kind == "contain" else 0
    nc.assert_step_matches(one, part, m, DT, 1, min_rows=min_rows)
    nc.assert_step_matches(two, part, m, DT, 2, prev=one, min_rows=min_rows)
    if case.kind == "contain":
        others = np.arange(n) != case.row(n, m)
        for got, ref, steps in ((one, twin[0], 1), (two, twin[1], 2)):
            assert got[others].tobytes() == ref[others].tobytes(), \
                f"{int((got[others].view(np.uint32) != ref[others].view(np.uint32)).sum())} words of other rows changed, {steps} step(s)"


@pytest.mark.parametrize("route", list(ROUTES))
def test_every_step_route_gives_the_references_classes(route):
    n, frac, knobs = ROUTES[route]
    part, m = nc.world(n, frac, seed=n)
    sim = pipeline(n, m, **knobs)
    # the chain makes both steps of a two-step call in one launch; its first step is the matched per-step shape's
    # (tests/test_gpu_chains.py), which gives the state the second step's identities start from
    chain = knobs.get("fused_chain") == 1
    walker = pipeline(n, m, **dict(matched_shape(n), fused_chain=0)) if chain else sim
    cases = nc.cases_for(n, m)
    assert len(cases) >= (14 if m == n else 23 if m < 257 else 33), (n, m, len(cases))
    fails = Failures()
    for case in cases:
        p = case.plant(part, m)
        one = steps_of(walker, p, 1)
        two = steps_of(sim, p, 2)
        fails.run(f"{case} [route]", check_route_taken, sim, knobs, 2)
        if chain:
            fails.run(f"{case} [one-step call]", nc.assert_step_matches, steps_of(sim, p, 1), p, m, DT, 1)
        twin = None
        if case.kind == "contain":
            t = nc.ordinary_tracer(p, case.row(n, m))
            twin = (steps_of(walker, t, 1), steps_of(sim, t, 2))
        fails.run(str(case), check_case, case, p, m, one, two, twin)
    if chain:
        walker.close()
    sim.close()
    fails.done()


def same_bytes(a, b):
    assert a.tobytes() == b.tobytes(), f"{int((a.view(np.uint32) != b.view(np.uint32)).sum())} words differ"


@pytest.mark.parametrize("knobs", [dict(), dict(lanes=1)], ids=["auto", "classic"])
def test_a_graph_chain_gives_the_bytes_of_plain_launches(knobs):
    n = 700
    part, m = nc.world(n, 0.6, seed=n)
    plain, graph = pipeline(n, m, graph=0, **knobs), pipeline(n, m, graph=1, **knobs)
    fails = Failures()
    for case in nc.cases_for(n, m):
        p = case.plant(part, m)
        a, b = steps_of(plain, p, 2), steps_of(graph, p, 2)
        fails.run(str(case), same_bytes, a, b)
    plain.close()
    graph.close()
    fails.done()


@pytest.mark.parametrize("knobs", [dict(), dict(k=1, w=1)], ids=["auto", "k1w1"])
def test_a_sharded_group_gives_the_references_classes(knobs):
    """Three shards of a 333-particle world: the pad sources of the short shards sit at (1e15, 1e15) with no mass, and the
    "pad-seat" case puts a receiver exactly there."""
    n, ranks = 333, 3
    part, m = nc.world(n, 0.5, seed=n)
    assert m % ranks != 0
    group = nb.LocalShardGroup(n, m, ranks, **knobs)
    cases = nc.cases_for(n, m)
    assert any(c.name == "contain-last-pad-seat" for c in cases)

    def steps(p, count):
        group.set_data(p)
        group.step(count, DT)
        outs = [group.get_data(r) for r in range(ranks)]
        for o in outs[1:]:
            assert o.tobytes() == outs[0].tobytes(), "the ranks hold different bytes"
        return outs[0]

    fails = Failures()
    for case in cases:
        p = case.plant(part, m)
        twin = None
        if case.kind == "contain":
            t = nc.ordinary_tracer(p, case.row(n, m))
            twin = (steps(t, 1), steps(t, 2))
        fails.run(str(case), check_case, case, p, m, steps(p, 1), steps(p, 2), twin)
    group.close()
    fails.done()


# ---- ensembles: the steps -------------------------------------------------------------------------------------------------------

PLANTED = 1          # member 1 of 4 carries the plant
FRACS = (0.3, 0.6, 0.8, 0.5)


def pinned_pipeline(n, m):
    u = nb.SimBatch(n, [m])
    knobs = u.pinned_knobs()
    u.close()
    return pipeline(n, m, **knobs)


def batch_steps(batch, worlds, count, ragged):
    batch.set_data(worlds if ragged else np.stack(worlds))
    batch.update(count, DT)
    got = batch.get_data()
    return [got[b] for b in range(len(worlds))]


@pytest.mark.parametrize("sizes", [(250,) * 4, (1000,) * 4, (250, 700, 129, 1000), (700, 250, 1000, 129)],
                         ids=["chain-250", "lanes-1000", "ragged-plant-in-lanes", "ragged-plant-in-chain"])
def test_an_ensemble_member_steps_like_its_own_pipeline_and_its_neighbours_see_nothing(sizes):
    ragged = len(set(sizes)) > 1
    worlds, ms = zip(*[nc.world(n, FRACS[b], seed=40 + b) for b, n in enumerate(sizes)])
    worlds, ms = list(worlds), list(ms)
    batch = nb.SimBatch.ragged(sizes, ms) if ragged else nb.SimBatch(sizes[0], ms)
    n, m = sizes[PLANTED], ms[PLANTED]
    alone = pinned_pipeline(n, m)
    clean = {c: batch_steps(batch, worlds, c, ragged) for c in (1, 2)}
    fails = Failures()

    def check(case, p):
        got = {}
        for c in (1, 2):
            got[c] = batch_steps(batch, worlds[:PLANTED] + [p] + worlds[PLANTED + 1:], c, ragged)
            for b in range(len(sizes)):
                if b != PLANTED:
                    assert got[c][b].tobytes() == clean[c][b].tobytes(), f"member {b} changed with its neighbour's plant, {c} step(s)"
            want = steps_of(alone, p, c)
            assert np.array_equal(got[c][PLANTED], want, equal_nan=True), f"member {PLANTED} is not its own pinned pipeline, {c} step(s)"
        min_rows = n - 1 if case.kind == "contain" else 0
        nc.assert_step_matches(got[1][PLANTED], p, m, DT, 1, min_rows=min_rows)
        nc.assert_step_matches(got[2][PLANTED], p, m, DT, 2, prev=got[1][PLANTED], min_rows=min_rows)

    for case in nc.cases_for(n, m):
        fails.run(str(case), check, case, case.plant(worlds[PLANTED], m))
    alone.close()
    batch.close()
    fails.done()


# ---- diagnostics ----------------------------------------------------------------------------------------------------------------

def host_diag(part):
    """the host path (float64; against numpy in tests/test_nonfinite_cpu.py) on a CPU-only World of the same particles"""
    w = nb.World(part)
    e, phi = w.energy(), w.potential()
    w.close()
    return e, phi


def check_diag(e, phi, a, m, name, row, clean):
    want_e, want_phi = host_diag(a)
    nc.assert_diag_matches(e, phi, want_e, want_phi, a, m, rel_u=1e-5, rel_phi=1e-5)
    if name == "massless-pos-nan":          # a massless row is no source and no term of any sum
        assert ebits(e) == ebits(clean[0]), "the energy changed with a massless row"
        assert np.delete(phi, row).tobytes() == np.delete(clean[1], row).tobytes(), "Phi of other rows changed"
        assert np.isnan(phi[row])


@pytest.mark.parametrize("m", nc.DIAG_M)
def test_pipeline_energy_and_potential_have_the_host_paths_classes(m):
    base, plants = nc.diag_plants(m)
    sim = pipeline(base.shape[0], m)
    sim.set_data(base)
    clean = (sim.energy(), sim.potential())
    fails = Failures()
    fails.run("clean", check_diag, clean[0], clean[1], base, m, "clean", None, clean)
    for name, row, a in plants:
        sim.set_data(a)
        fails.run(name, check_diag, sim.energy(), sim.potential(), a, m, name, row, clean)
    sim.close()
    fails.done()


@pytest.mark.parametrize("sizes,m", [((250,) * 4, 181), ((513,) * 4, 300), ((250, 340, 129, 513), 300), ((513, 221, 1000, 64), 181)],
                         ids=["uniform-250", "uniform-513", "ragged-340", "ragged-221"])
def test_ensemble_energy_and_potential(sizes, m):
    ragged = len(set(sizes)) > 1
    n = sizes[PLANTED]
    ms = [s // 3 if b != PLANTED else m for b, s in enumerate(sizes)]
    worlds = [nc.diag_world(mb, s - mb, seed=70 + b) for b, (s, mb) in enumerate(zip(sizes, ms))]
    base, plants = nc.diag_plants(m, n - m)
    worlds[PLANTED] = base
    batch = nb.SimBatch.ragged(sizes, ms) if ragged else nb.SimBatch(sizes[0], ms)
    alone = pipeline(n, m)

    def diag(members):
        batch.set_data(members if ragged else np.stack(members))
        e, phi = batch.energy(), batch.potential()
        return e, [phi[b] for b in range(len(sizes))]

    clean = diag(worlds)
    for b, (s, mb) in enumerate(zip(sizes, ms)):          # the clean members by themselves: what they must stay equal to
        one = pipeline(s, mb)
        one.set_data(worlds[b])
        assert ebits(one.energy()) == ebits(clean[0][b]) and one.potential().tobytes() == clean[1][b].tobytes(), b
        one.close()
    fails = Failures()

    def check(name, row, a):
        e, phi = diag(worlds[:PLANTED] + [a] + worlds[PLANTED + 1:])
        for b in range(len(sizes)):
            if b != PLANTED:
                assert ebits(e[b]) == ebits(clean[0][b]) and phi[b].tobytes() == clean[1][b].tobytes(), f"member {b} changed"
        check_diag(e[PLANTED], phi[PLANTED], a, m, name, row, (clean[0][PLANTED], clean[1][PLANTED]))
        alone.set_data(a)                    # include/nbody_hip.h "World ensembles": the pipeline's bits
        assert np.array_equal(nc.energy_vector(e[PLANTED]), nc.energy_vector(alone.energy()), equal_nan=True)
        assert np.array_equal(phi[PLANTED], alone.potential(), equal_nan=True)

    for name, row, a in plants:
        fails.run(name, check, name, row, a)
    alone.close()
    batch.close()
    fails.done()


@pytest.mark.parametrize("n", [250, 1000], ids=["fused-250", "interleaved-1000"])
def test_a_traced_ensemble_records_the_host_paths_classes(n):
    """vel.x = +inf on particle 0 of member 1: row 0 has +inf in kinetic, momentum.x and angular momentum; after two steps
    the particle is at x = +inf and the member's rows are what the host path makes of that state."""
    ms = [n // 3, 181 if n == 250 else 300, n - 5, n // 2]
    worlds = [nc.diag_world(mb, n - mb, seed=90 + b) for b, mb in enumerate(ms)]
    planted = list(worlds)
    planted[PLANTED] = worlds[PLANTED].copy()
    planted[PLANTED][0, 2] = np.inf
    batch = nb.SimBatch(n, ms)

    def trace(members):
        batch.set_data(np.stack(members))
        rows = batch.trace(4, DT, 2)
        assert batch.last_trace_info()["fused"] == (1 if n <= 512 else 0)
        return rows

    clean, rows = trace(worlds), trace(planted)
    assert rows.shape == (3, 4, 8)
    others = [b for b in range(4) if b != PLANTED]
    assert rows[:, others].tobytes() == clean[:, others].tobytes(), "a clean member's rows changed with its neighbour's plant"
    c = nc.classes(rows[0, PLANTED]).tolist()          # kinetic potential mass px py L cx cy
    assert c[5] in (nc.POS_INF, nc.NEG_INF) and c[:5] + c[6:] == [1, 0, 0, 1, 0, 0, 0], c
    # the states the rows describe, by separate calls; the host path on each
    batch.set_data(np.stack(planted))
    for r in range(3):
        state = batch.get_member(PLANTED)
        want_e, _ = host_diag(state)
        nc.assert_diag_matches(nb.energy_row(rows[r, PLANTED]), None, want_e, None, state, ms[PLANTED], rel_u=1e-5)
        batch.update(2, DT)
    batch.close()


# ---- the field samplers ---------------------------------------------------------------------------------------------------------

def test_field_samplers_with_a_non_finite_source():
    """potential_at and acceleration_at on both kernel shapes over a 300-source world with one source at NaN, then at
    x = +inf (Phi loses that source's term and stays finite; g.x is dx * 0 = NaN, g.y stays finite): the host path's
    classes, the finite values within the samplers' standing tolerances, and the clean world's samples unchanged."""
    m, extra = 300, 50
    base = nc.diag_world(m, extra, seed=3)
    rng = np.random.default_rng(11)
    pts = (rng.standard_normal((333, 2)) * 150.0).astype(np.float32)
    pts[0] = base[7, 0:2]                     # a probe on a source
    sim = pipeline(m + extra, m)
    fails = Failures()

    def sample(a, shape):
        sim.set_data(a)
        sim.configure(field_shape=shape, gravity_shape=shape)
        return sim.potential_at(pts, SOFT), sim.acceleration_at(pts, SOFT)

    def check(a, shape, clean):
        phi, g = sample(a, shape)
        w = nb.World(a)
        want_phi, want_g = w.potential_at(pts, SOFT), w.acceleration_at(pts, SOFT)
        w.close()
        assert np.array_equal(nc.classes(phi), nc.classes(want_phi)), "Phi classes differ from the host path's"
        assert np.array_equal(nc.classes(g), nc.classes(want_g)), "g classes differ from the host path's"
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            phi64 = phi_at_f64(a, m, pts, SOFT)
            g64, mag = g_at_f64(a, m, pts, SOFT)
            ok = np.isfinite(want_phi) & np.isfinite(phi64)
            assert np.all(np.abs(phi[ok] - phi64[ok]) <= 1e-5 * np.abs(phi64[ok])), "finite Phi outside 1e-5"
            ok = np.isfinite(want_g) & np.isfinite(g64) & np.isfinite(mag)
            assert np.all(np.abs(g[ok] - g64[ok]) <= acc_bound(g64, mag)[ok]), "finite g outside acc_bound"
        again = sample(base, shape)
        assert again[0].tobytes() == clean[0].tobytes() and again[1].tobytes() == clean[1].tobytes(), "the clean samples changed"

    for shape in (SPLIT, WAVE):
        clean = sample(base, shape)
        assert np.all(np.isfinite(clean[0])) and np.all(np.isfinite(clean[1]))
        for j in (0, 255, 256, m - 1):
            a = base.copy()
            a[j, 0:2] = np.nan
            fails.run(f"shape {shape} source {j} pos NaN", check, a, shape, clean)
            a = base.copy()
            a[j, 0] = np.inf
            fails.run(f"shape {shape} source {j} x = +inf", check, a, shape, clean)
    sim.close()
    fails.done()
