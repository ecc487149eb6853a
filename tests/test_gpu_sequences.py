"""Long-lived pipelines and ensembles against chains of fresh ones (tests/sequence_driver.py), on the MI355X: seeded
sequences of every kind of call -- fixed and adaptive steps, blocking and async, diagnostics, fields, render, get / set -- on
ONE object, each output bit for bit what a new object gives for the same call from the same state.  One row per step route
and launch shape, so that the phase bit, the cached chains, the device-side step size, the adaptive head and the scratch
buffers are all left behind by one feature and found by another.  The hazards that have a name are also written out in full
(the directed tests).  The reads kinds put tidal_at, tidal_map, profile, pair_counts and neighbours -- and on ensembles, uniform
and ragged, the Phi / g field calls -- among them: the calls that share one scratch and merge into it through integer atomics,
each output followed by whether the call recorded the interval.  The seeds are the ones tests/test_sequence_cpu.py shows to catch every planted fault.  This file
compares the library with itself; tests/test_gpu_adaptive.py anchors the same launch shapes to the numpy criterion."""
import time

import numpy as np
import pytest

import nbody_amd as nb
import sequence_driver as sd
from gpu_common import synth
from reads_common import assert_the_reads_have_something_to_say, factories
from test_gpu_ragged import MASS as RAGGED_MASS, SIZES as RAGGED_SIZES, world as ragged_world

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


PIPE_ROWS = sd.PIPE_ROWS
BATCH_ROWS = {"chain-5x250": (5, 250), "lanes-3x800": (3, 800)}

_points = np.random.default_rng(77).standard_normal((max(sd.POINT_COUNTS), 2)).astype(np.float32) * 1.0e4


def second_world(n, m, seed):
    """a second seeded world with the same N and M: other positions, velocities, masses and radii"""
    part = synth(n, frac_massive=1.1, seed=seed)[0].copy()
    part[m:, 6], part[m:, 7] = 0.0, 0.5
    return part


def views(centre):
    """32 x 18 and the maps: the whole world, every particle a point; 80 x 45: close on one massive particle, so discs."""
    def view(w, h):
        if (w, h) == (80, 45):
            return nb.RenderView.make((float(centre[0]), float(centre[1])), (w / 2, h / 2), 0.5, w, h, 2.0e4)
        return nb.RenderView.make((0.0, 0.0), (w / 2, h / 2), w / 6.0e4, w, h, 2.0e4)
    return view


_envs = {}


def pipe_env(n, frac):
    """Start and second state of a row, each two fixed steps in (so acc is not zero and the criterion has something to say);
    computed once per size, shared, never changed."""
    if (n, frac) not in _envs:
        part, m = synth(n, frac_massive=frac, seed=n)
        states = []
        for p in (part, second_world(n, m, n + 1)):
            s = nb.SimPipeline(n, m)
            s.set_data(p)
            s.update(2, 0.01)
            states.append(s.get_data())
            s.close()
        sd.assert_premise(*states)          # finite, no -0.0: what the leapfrog kinds rest on (sequence_driver's docstring)
        _envs[(n, frac)] = (sd.Env("pipeline", states[0], states[1], views(states[0][0, 0:2]), lambda k: _points[:k]), m)
    return _envs[(n, frac)]


def as_kind(env, kind):
    """the same states, views and points under another kind: the leapfrog kinds run on their base kind's worlds"""
    return sd.Env(kind, env.start, env.other, env.view, env.points, env.members)


def pipe_maker(n, m, knobs):
    def make():
        s = nb.SimPipeline(n, m)
        s.configure(**knobs)
        return s
    return make


def run_row(row, ops, seed=None, kind="pipeline"):
    n, frac, knobs = PIPE_ROWS[row]
    env, m = pipe_env(n, frac)
    t0 = time.perf_counter()
    compared = sd.check(pipe_maker(n, m, knobs), ops, env if kind == "pipeline" else as_kind(env, kind), seed)
    print(f"[sequence] {row} {kind} seed {seed}: {len(ops)} operations, {compared} outputs compared, {time.perf_counter() - t0:.2f} s")
    return compared


@pytest.mark.parametrize("seed", sd.SEEDS["pipeline"])
@pytest.mark.parametrize("row", list(PIPE_ROWS))
def test_a_long_lived_pipeline_is_a_chain_of_fresh_ones(row, seed):
    ops = sd.generate("pipeline", seed)
    assert run_row(row, ops, seed) > len(ops) // 2


LEAPFROG_PIPE_ROWS = ["chain-200", "lanes-600-graph1", "classic-4133", "classic-4133-graph2", "classic-4133-lds", "split3-finish-9000",
                      "fused-finish-9000", "passes2-1500"]


@pytest.mark.parametrize("seed", sd.SEEDS["pipeline-lf"])
@pytest.mark.parametrize("row", LEAPFROG_PIPE_ROWS)
def test_a_long_lived_pipeline_with_leapfrog_calls_is_a_chain_of_fresh_ones(row, seed):
    """Leapfrog calls, fixed and adaptive, blocking and async, among everything the "pipeline" kind draws; and after every
    one of them last_leapfrog_info() against the driver's model of "acc is current": it primed exactly when it had to."""
    ops = sd.generate("pipeline-lf", seed)
    assert run_row(row, ops, seed, "pipeline-lf") > len(ops) // 2


# ---- ensembles -----------------------------------------------------------------------------------------------------------------

def batch_env(count, n):
    if (count, n) not in _envs:
        worlds = [synth(n, frac_massive=0.5, seed=1000 * n + b) for b in range(count)]
        ms = [m for _, m in worlds]
        states = []
        for parts in (np.stack([p for p, _ in worlds]), np.stack([second_world(n, m, 2000 * n + b) for b, m in enumerate(ms)])):
            s = nb.SimBatch(n, ms)
            s.set_data(parts)
            s.update(2, 0.01)
            states.append(s.get_data())
            s.close()
        sd.assert_premise(*states)
        _envs[(count, n)] = (sd.Env("batch", states[0], states[1], views(states[0][0, 0, 0:2]), None, members=count), ms)
    return _envs[(count, n)]


@pytest.mark.parametrize("seed", sd.SEEDS["batch"])
@pytest.mark.parametrize("row", list(BATCH_ROWS))
def test_a_long_lived_ensemble_is_a_chain_of_fresh_ones(row, seed):
    count, n = BATCH_ROWS[row]
    env, ms = batch_env(count, n)
    ops = sd.generate("batch", seed, members=count)
    t0 = time.perf_counter()
    compared = sd.check(lambda: nb.SimBatch(n, ms), ops, env, seed)
    print(f"[sequence] {row} seed {seed}: {len(ops)} operations, {compared} outputs compared, {time.perf_counter() - t0:.2f} s")
    assert compared > len(ops) // 2


@pytest.mark.parametrize("seed", sd.SEEDS["batch-lf"])
@pytest.mark.parametrize("row", list(BATCH_ROWS))
def test_a_long_lived_ensemble_with_leapfrog_calls_is_a_chain_of_fresh_ones(row, seed):
    count, n = BATCH_ROWS[row]
    env, ms = batch_env(count, n)
    ops = sd.generate("batch-lf", seed, members=count)
    t0 = time.perf_counter()
    compared = sd.check(lambda: nb.SimBatch(n, ms), ops, as_kind(env, "batch-lf"), seed)
    print(f"[sequence] {row} batch-lf seed {seed}: {len(ops)} operations, {compared} outputs compared, {time.perf_counter() - t0:.2f} s")
    assert compared > len(ops) // 2


@pytest.mark.parametrize("seed", sd.SEEDS["ragged"])
def test_a_long_lived_ragged_ensemble_is_a_chain_of_fresh_ones(seed):
    """The ensemble of tests/test_gpu_ragged.py; steps, trace, energy, potential, get and set of the calls
    include/nbody_batch_ragged.h lists (the driver refuses any other on this kind before it reaches the library; the
    "ragged-reads" kind below draws the rest)."""
    members = range(len(RAGGED_SIZES))
    env = sd.Env("ragged", [ragged_world(b, 0) for b in members], [ragged_world(b, 1) for b in members], None, None,
                 members=len(RAGGED_SIZES))
    ops = sd.generate("ragged", seed, members=len(RAGGED_SIZES))
    t0 = time.perf_counter()
    compared = sd.check(lambda: nb.SimBatch.ragged(RAGGED_SIZES, RAGGED_MASS), ops, env, seed)
    print(f"[sequence] ragged seed {seed}: {len(ops)} operations, {compared} outputs compared, {time.perf_counter() - t0:.2f} s")
    assert compared > len(ops) // 2


# ---- the reads kinds: tidal, profile, pair-count and neighbour calls among all the others ----------------------------------------

def reads_env(kind, env, worlds):
    """the states of `env` under a reads kind, with the factories of tests/reads_common.py for the new calls; worlds: the
    start state as [(particles, mass_len)], on which the radius and the edges are held to have something to say"""
    assert_the_reads_have_something_to_say(worlds)
    f = factories(env.members, env.view)
    return sd.Env(kind, env.start, env.other, f["view"], f["points"], members=env.members, edges=f["edges"], centre=f["centre"], radius=f["radius"])


_reads_envs = {}


def pipe_reads_env(n, frac):
    if (n, frac) not in _reads_envs:
        env, m = pipe_env(n, frac)
        _reads_envs[(n, frac)] = (reads_env("pipeline-reads", env, [(env.start, m)]), m)
    return _reads_envs[(n, frac)]


def run_reads_row(row, ops, seed=None):
    n, frac, knobs = PIPE_ROWS[row]
    env, m = pipe_reads_env(n, frac)
    t0 = time.perf_counter()
    compared = sd.check(pipe_maker(n, m, knobs), ops, env, seed)
    print(f"[sequence] {row} pipeline-reads seed {seed}: {len(ops)} operations, {compared} outputs compared, {time.perf_counter() - t0:.2f} s")
    return compared


# the reads depend on the step route only through the phase bit and the stream: one row per route, and the sizes that lie inside
# one block (200), span 17 source blocks and 33 receiver tiles of the neighbour and pair-count kernels (4 133) and beyond (9 000)
READS_PIPE_ROWS = ["chain-200", "lanes-600-graph1", "classic-4133", "passes2-1500", "split3-finish-9000"]


@pytest.mark.parametrize("seed", sd.SEEDS["pipeline-reads"])
@pytest.mark.parametrize("row", READS_PIPE_ROWS)
def test_a_long_lived_pipeline_with_every_read_only_call_is_a_chain_of_fresh_ones(row, seed):
    """tidal_at, tidal_map, profile, pair_counts and neighbours with drawn arguments among everything the "pipeline" kind draws,
    every output followed by whether the call recorded the interval.  In classic-4133 every particle is massive, so the planted
    neighbours call under EMPTY_MASKS has nothing to launch there."""
    ops = sd.generate("pipeline-reads", seed)
    assert run_reads_row(row, ops, seed) > len(ops) // 2


def batch_reads_env(count, n):
    if ("reads", count, n) not in _reads_envs:
        env, ms = batch_env(count, n)
        _reads_envs[("reads", count, n)] = (reads_env("batch-reads", env, list(zip(env.start, ms))), ms)
    return _reads_envs[("reads", count, n)]


@pytest.mark.parametrize("seed", sd.SEEDS["batch-reads"])
@pytest.mark.parametrize("row", list(BATCH_ROWS))
def test_a_long_lived_ensemble_with_every_read_only_call_is_a_chain_of_fresh_ones(row, seed):
    """and the four Phi / g field calls, which the "batch" kind never draws; points, views and centres one for all members or
    one per member, as drawn"""
    count, n = BATCH_ROWS[row]
    env, ms = batch_reads_env(count, n)
    ops = sd.generate("batch-reads", seed, members=count)
    t0 = time.perf_counter()
    compared = sd.check(lambda: nb.SimBatch(n, ms), ops, env, seed)
    print(f"[sequence] {row} batch-reads seed {seed}: {len(ops)} operations, {compared} outputs compared, {time.perf_counter() - t0:.2f} s")
    assert compared > len(ops) // 2


def ragged_reads_env():
    if "ragged" not in _reads_envs:
        members = range(len(RAGGED_SIZES))
        env = sd.Env("ragged", [ragged_world(b, 0) for b in members], [ragged_world(b, 1) for b in members], None, None,
                     members=len(RAGGED_SIZES))
        _reads_envs["ragged"] = reads_env("ragged-reads", env, list(zip(env.start, RAGGED_MASS)))
    return _reads_envs["ragged"]


def ragged_maker():
    return nb.SimBatch.ragged(RAGGED_SIZES, RAGGED_MASS)


@pytest.mark.parametrize("seed", sd.SEEDS["ragged-reads"])
def test_a_long_lived_ragged_ensemble_with_every_read_only_call_is_a_chain_of_fresh_ones(seed):
    """The ensemble of tests/test_gpu_ragged.py (a member of one particle, one without a massive and three without a massless
    particle among them) with every call include/nbody_batch_ragged.h lists; render, bounds and the adaptive calls still abort
    on it and the driver refuses them."""
    ops = sd.generate("ragged-reads", seed, members=len(RAGGED_SIZES))
    t0 = time.perf_counter()
    compared = sd.check(ragged_maker, ops, ragged_reads_env(), seed)
    print(f"[sequence] ragged-reads seed {seed}: {len(ops)} operations, {compared} outputs compared, {time.perf_counter() - t0:.2f} s")
    assert compared > len(ops) // 2


# ---- directed sequences: the hazards that have a name ----------------------------------------------------------------------------

def op(name, **args):
    return name, args


def neigh(radius, receivers="all", sources="all"):
    return op("neighbours", radius=radius, receivers=receivers, sources=sources)


# counts under (all, all); a call with no radius under other masks, which must leave them alone; a pair-count table over the keys;
# then counts under those other masks, added into what must have been zeroed; and two tables in a row with other classes
ACCUMULATORS = [neigh(True), neigh(False, "massive", "all"), op("pair_counts", bins=64, classes="all"), neigh(True, "massive", "all"),
                op("pair_counts", bins=4, classes="all"), op("pair_counts", bins=4, classes=("mm",))]


def test_the_accumulators_of_the_read_scratch_start_from_what_the_call_itself_reset():
    run_reads_row("classic-4133", ACCUMULATORS)


def test_the_accumulators_of_a_ragged_ensemble_start_from_what_the_call_itself_reset():
    t0 = time.perf_counter()
    compared = sd.check(ragged_maker, ACCUMULATORS, ragged_reads_env())
    print(f"[sequence] ragged-reads accumulators: {len(ACCUMULATORS)} operations, {compared} outputs compared, {time.perf_counter() - t0:.2f} s")


def test_the_new_reads_behind_async_adaptive_steps_see_the_state_after_them():
    ops = [op("update_adaptive_async", n=3), op("tidal_map", w=40, h=30), op("profile", bins=64, weights="mass", centre=0),
           op("pair_counts", bins=64, classes="all"), neigh(True), op("adaptive_collect", n=3)]
    run_reads_row("lanes-600", ops)


def test_layouts_that_overlap_in_a_work_buffer_of_a_few_kilobytes():
    """N = 200: the pair-count table (66 rows of three uint64), the energy partials, the neighbour keys and counts and the
    potentials all begin at the start of the same small buffer."""
    ops = [op("pair_counts", bins=64, classes="all"), op("energy"), neigh(True), op("potential"), neigh(False)]
    run_reads_row("chain-200", ops)


@pytest.mark.parametrize("graph", [1, 2])
@pytest.mark.parametrize("n,frac", [(600, 0.5), (4133, 1.0)])
def test_odd_adaptive_steps_then_the_chain_cached_for_the_other_phase(n, frac, graph):
    """An odd number of adaptive steps flips the phase bit; the next 20-step call finds the chain that was captured in the
    other phase, and the step size in device memory is the one the device chose."""
    env, m = pipe_env(n, frac)
    ops = [op("update", n=20, dt=0.01), op("update_adaptive", n=3), op("update", n=20, dt=0.01), op("update_adaptive", n=1),
           op("update", n=20, dt=0.005), op("get_data")]
    sd.check(pipe_maker(n, m, dict(graph=graph)), ops, env)


@pytest.mark.parametrize("row", ["chain-200", "lanes-600", "split3-finish-9000"])
def test_reads_behind_async_adaptive_steps_see_the_state_after_them(row):
    ops = [op("update_adaptive_async", n=3), op("potential_map", w=40, h=30), op("render", w=80, h=45), op("energy"),
           op("adaptive_collect", n=3)]
    run_row(row, ops)


@pytest.mark.parametrize("row", ["chain-200", "classic-4133"])
def test_energy_after_buffers_that_regrew(row):
    ops = [op("render", w=80, h=45), op("energy"), op("acceleration_at", count=300), op("potential"), op("render", w=32, h=18),
           op("energy")]
    run_row(row, ops)


@pytest.mark.parametrize("row", ["chain-200", "classic-4133", "passes2-1500"])
def test_a_new_state_on_an_armed_adaptive_head(row):
    ops = [op("update_adaptive", n=2), op("set_data"), op("timestep"), op("update_adaptive", n=2)]
    run_row(row, ops)
