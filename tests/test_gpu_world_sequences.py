"""A long-lived World / WorldBatch against chains of fresh ones (tests/world_sequence.py), on the MI355X: seeded sequences of
CPU and GPU steps (Euler, leapfrog, adaptive, advance, traced), read-backs, diagnostics, fields and renders on ONE object,
every output bit for bit what a new object gives for the same call from the same state, and every diagnostic answered by the
side the headers name (the device value is a fresh SimPipeline's / SimBatch's, the host value a fresh World's that never
stepped on the GPU).  The layer under test is world.c / world_batch.c: host_is_newer, device_is_newer, cpu_acc_current,
uploaded.  The seeds are the ones tests/test_world_sequence_cpu.py shows to catch every planted fault of its stand-ins."""
import time

import numpy as np
import pytest

import nbody_amd as nb
import sequence_driver as sd
import world_sequence as ws
from gpu_common import synth
from reads_common import assert_the_reads_have_something_to_say, factories
from test_gpu_ragged import MASS as RAGGED_MASS, SIZES as RAGGED_SIZES, world as ragged_world
from test_gpu_sequences import views

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


_points = np.random.default_rng(78).standard_normal((max(sd.POINT_COUNTS), 2)).astype(np.float32) * 1.0e4
_envs = {}


def world_env(n, frac):
    """The start state of a row, two fixed GPU steps in (acc is not zero: the criterion has something to say); once per size."""
    if (n, frac) not in _envs:
        w = nb.World(synth(n, frac_massive=frac, seed=n)[0])
        w.update_gpu(0.01, 2)
        start = w.particles()
        w.close()
        sd.assert_premise(start)          # finite, no -0.0: a skipped priming launch and a made one then agree in bits
        m = int(np.count_nonzero(start[:, 6] > 0))

        def device(state):
            s = nb.SimPipeline(n, m)
            s.set_data(state)
            return s
        _envs[(n, frac)] = ws.Env("world", start, nb.World, device, views(start[0, 0:2]), lambda k: _points[:k])
    return _envs[(n, frac)]


def batch_env(count, n):
    if (count, n) not in _envs:
        w = nb.WorldBatch(np.stack([synth(n, frac_massive=0.5, seed=1000 * n + b)[0] for b in range(count)]))
        w.update_gpu(0.01, 2)
        start = w.particles()
        w.close()
        sd.assert_premise(start)
        ms = [int(np.count_nonzero(start[b, :, 6] > 0)) for b in range(count)]

        def device(state):
            s = nb.SimBatch(n, ms)
            s.set_data(state)
            return s
        _envs[(count, n)] = ws.Env("batch", start, nb.WorldBatch, device, views(start[0, 0, 0:2]), None, members=count)
    return _envs[(count, n)]


def ragged_env():
    if "ragged" not in _envs:
        w = nb.WorldBatch.ragged([ragged_world(b, 0) for b in range(len(RAGGED_SIZES))])
        w.update_gpu(0.01, 2)
        start = w.particles()
        w.close()
        sd.assert_premise(*start)

        def device(state):
            s = nb.SimBatch.ragged(RAGGED_SIZES, RAGGED_MASS)
            s.set_data(state)
            return s
        _envs["ragged"] = ws.Env("ragged", start, nb.WorldBatch.ragged, device, None, None, members=len(RAGGED_SIZES))
    return _envs["ragged"]


def run(tag, env, ops, seed=None):
    t0 = time.perf_counter()
    compared = ws.check(env, ops, seed)
    print(f"[sequence] {tag} seed {seed}: {len(ops)} operations, {compared} outputs compared, {time.perf_counter() - t0:.2f} s")
    return compared


@pytest.mark.parametrize("seed", ws.SEEDS["world"])
@pytest.mark.parametrize("row", list(ws.WORLD_ROWS))
def test_a_long_lived_world_is_a_chain_of_fresh_ones(row, seed):
    ops = ws.generate("world", seed)
    assert run(f"world {row}", world_env(*ws.WORLD_ROWS[row]), ops, seed) > len(ops) // 2


@pytest.mark.parametrize("seed", ws.SEEDS["batch"])
@pytest.mark.parametrize("row", list(ws.BATCH_ROWS))
def test_a_long_lived_world_batch_is_a_chain_of_fresh_ones(row, seed):
    count, n = ws.BATCH_ROWS[row]
    ops = ws.generate("batch", seed, members=count)
    assert run(f"world-batch {row}", batch_env(count, n), ops, seed) > len(ops) // 2


@pytest.mark.parametrize("seed", ws.SEEDS["ragged"])
def test_a_long_lived_ragged_world_batch_is_a_chain_of_fresh_ones(seed):
    """The ensemble of tests/test_gpu_ragged.py; steps, traced steps, energy, potential and the read-backs of the calls
    include/nbody_batch_ragged.h lists ("ragged-reads" below draws the rest)."""
    ops = ws.generate("ragged", seed, members=len(RAGGED_SIZES))
    assert run("world-batch ragged", ragged_env(), ops, seed) > len(ops) // 2


# ---- the reads kinds: tidal calls under the path rule; profile, pair_counts and neighbours bit for bit on either side -----------

_reads = {}


def as_reads(kind, env, worlds):
    """the same start state, makers and seam object under a reads kind, with the arguments of tests/reads_common.py"""
    if (kind, id(env)) not in _reads:
        assert_the_reads_have_something_to_say(worlds)
        f = factories(env.members, env.view)
        _reads[(kind, id(env))] = ws.Env(kind, env.start, env.make, env.device, f["view"], f["points"], members=env.members, edges=f["edges"],
                                         centre=f["centre"], radius=f["radius"])
    return _reads[(kind, id(env))]


def massive(part):
    return int(np.count_nonzero(part[:, 6] > 0))


@pytest.mark.parametrize("seed", ws.SEEDS["world-reads"])
@pytest.mark.parametrize("row", list(ws.WORLD_ROWS))
def test_a_long_lived_world_with_every_read_only_call_is_a_chain_of_fresh_ones(row, seed):
    """tidal_at and tidal_map answered by the side the rule names; profile, pair_counts and neighbours equal to the fresh World's
    and to the seam object's, whichever side answered"""
    env = world_env(*ws.WORLD_ROWS[row])
    ops = ws.generate("world-reads", seed)
    assert run(f"world-reads {row}", as_reads("world-reads", env, [(env.start, massive(env.start))]), ops, seed) > len(ops) // 2


@pytest.mark.parametrize("seed", ws.SEEDS["batch-reads"])
@pytest.mark.parametrize("row", list(ws.BATCH_ROWS))
def test_a_long_lived_world_batch_with_every_read_only_call_is_a_chain_of_fresh_ones(row, seed):
    count, n = ws.BATCH_ROWS[row]
    env = batch_env(count, n)
    ops = ws.generate("batch-reads", seed, members=count)
    assert run(f"world-batch-reads {row}", as_reads("batch-reads", env, [(p, massive(p)) for p in env.start]), ops, seed) > len(ops) // 2


@pytest.mark.parametrize("seed", ws.SEEDS["ragged-reads"])
def test_a_long_lived_ragged_world_batch_with_every_read_only_call_is_a_chain_of_fresh_ones(seed):
    env = ragged_env()
    ops = ws.generate("ragged-reads", seed, members=len(RAGGED_SIZES))
    assert run("world-batch-reads ragged", as_reads("ragged-reads", env, list(zip(env.start, RAGGED_MASS))), ops, seed) > len(ops) // 2
