"""Nearest neighbours and neighbour counts of ensembles on the GPU (nb_hip_ensemble_neighbours, neighbour.hip): every member of a
uniform or ragged SimBatch bit for bit its own SimPipeline.neighbours and the numpy model (neighbour_ref.py), over the nine mask
combinations, with and without a radius and for every forced span length; and WorldBatch.neighbours on the host and on the device.
Every comparison is of raw bits: there is no tolerance."""
import numpy as np
import pytest

import nbody_amd as nb
import neighbour_ref as nr
from paircount_ref import world

pytestmark = pytest.mark.gpu

DT = 0.01
RADIUS = 1.5
COMBOS = [(r, s) for r in nr.MASKS for s in nr.MASKS]


@pytest.fixture(autouse=True)
def needs_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def member(out, b):
    """Member b's arrays of a uniform (B, N) or ragged (lists) result."""
    return tuple(a[b] for a in out)


def check_members(batch, host, states, mass_lens, label, combos=COMBOS):
    """Every member of `batch` against its own pipeline, the model and the host path through the never-stepped WorldBatch `host`."""
    pipes = []
    for a, m in zip(states, mass_lens):
        pipes.append(nb.SimPipeline(a.shape[0], m))
        pipes[-1].set_data(a)
    for r, s in combos:
        names = (nr.NAMES[r], nr.NAMES[s])
        got, bare, on_host = batch.neighbours(RADIUS, *names), batch.neighbours(None, *names), host.neighbours(RADIUS, *names)
        assert len(got) == 3 and len(bare) == 2
        for b, (a, m) in enumerate(zip(states, mass_lens)):
            want = nr.model(a, m, r, s, RADIUS)
            assert nr.same(member(got, b), want), (label, names, b, "ensemble against the model")
            assert nr.same(member(bare, b), want[:2]), (label, names, b, "without the count")
            assert nr.same(member(got, b), pipes[b].neighbours(RADIUS, *names)), (label, names, b, "ensemble against its own pipeline")
            assert nr.same(member(on_host, b), want), (label, names, b, "host path")
    for p in pipes:
        p.close()


@pytest.mark.parametrize("count,n", [(5, 250), (3, 3000)])
def test_every_member_of_a_uniform_ensemble_is_its_own_pipeline_the_model_and_the_host_path(count, n):
    mass_lens = [(0, n // 3, n, 1, n - 1)[b % 5] for b in range(count)]
    states = [world(n, m, seed=200 + 7 * b + n) for b, m in enumerate(mass_lens)]
    batch, host = nb.SimBatch(n, mass_lens), nb.WorldBatch(np.stack(states))
    batch.set_data(np.stack(states))
    got = batch.neighbours(RADIUS)
    assert all(a.shape == (count, n) for a in got) and [a.dtype for a in got] == [np.float32, np.uint32, np.uint32]
    check_members(batch, host, states, mass_lens, (count, n))
    try:          # the spans of an ensemble: N = 3 000 has 12 blocks
        for blocks in (1, 2, 5):
            nb.hip_lib().nb_hip_neighbour_span(blocks)
            assert nr.same(batch.neighbours(RADIUS), got), (count, n, blocks)
    finally:
        nb.hip_lib().nb_hip_neighbour_span(0)
    batch.close()
    host.close()


def test_every_member_of_a_ragged_ensemble_is_its_own_pipeline_the_model_and_the_host_path():
    sizes, mass_lens = (1, 2, 129, 300, 3000), (1, 0, 43, 300, 1000)
    states = [world(n, m, seed=300 + n) for n, m in zip(sizes, mass_lens)]
    batch, host = nb.SimBatch.ragged(sizes, mass_lens), nb.WorldBatch.ragged(states)
    batch.set_data(states)
    got = batch.neighbours(RADIUS)
    assert all(isinstance(a, list) and [x.shape for x in a] == [(n,) for n in sizes] for a in got)
    check_members(batch, host, states, mass_lens, "ragged")
    try:
        for blocks in (1, 5):
            nb.hip_lib().nb_hip_neighbour_span(blocks)
            again = batch.neighbours(RADIUS)
            assert all(nr.same(member(again, b), member(got, b)) for b in range(len(sizes))), blocks
    finally:
        nb.hip_lib().nb_hip_neighbour_span(0)
    batch.close()
    host.close()


def test_a_world_batch_answers_on_the_device_once_it_has_stepped_there():
    sizes = (129, 300, 700)
    states = [world(n, n // 2, seed=400 + n) for n in sizes]
    wb = nb.WorldBatch.ragged(states)
    before = wb.neighbours(RADIUS, "massive", "all")          # the host path
    wb.update_gpu(DT, 2)
    on_device = wb.neighbours(RADIUS, "massive", "all")          # the device holds the newest state
    after = wb.particles()
    for b, n in enumerate(sizes):
        assert nr.same(member(before, b), nr.model(states[b], n // 2, nr.MASSIVE, nr.ALL, RADIUS)), b
        assert nr.same(member(on_device, b), nr.model(after[b], n // 2, nr.MASSIVE, nr.ALL, RADIUS)), b
        assert not nr.same(member(on_device, b), member(before, b)), b
    wb.close()
