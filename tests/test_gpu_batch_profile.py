"""Radial profiles of ensembles on the GPU (nb_hip_ensemble_profile, profile.hip): every member of a uniform or ragged
SimBatch bit for bit its own SimPipeline.profile and the numpy model (profile_ref.py), with shared and per-member centres;
a member full of NaN changes no bit of its neighbours; WorldBatch.profile on the device and on the host."""
import numpy as np
import pytest

import nbody_amd as nb
import profile_ref as pr

pytestmark = pytest.mark.gpu

DT = 0.01
MODES = {pr.BY_MASS: "mass", pr.BY_NUMBER: "number"}
VELOCITY = (0.125, -0.0625)


@pytest.fixture(autouse=True)
def needs_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def centres_of(count, per_member):
    if not per_member:
        return np.array(pr.CENTRE[0:2], dtype=np.float32)
    return (np.array(pr.CENTRE[0:2]) + np.arange(count)[:, None] * np.array([0.75, -1.5])).astype(np.float32)


def check_members(batch, states, mass_lens, edges, label):
    """Every member of `batch` (holding `states`) against its own pipeline and against the model, both weights, both kinds of centre."""
    count = len(states)
    for per_member in (False, True):
        c = centres_of(count, per_member)
        for weights in (pr.BY_MASS, pr.BY_NUMBER):
            got, lost = batch.profile(edges, centre=c, centre_velocity=VELOCITY, weights=MODES[weights], return_unplaced=True)
            assert got.shape == (count, len(edges) + 1, 6) and got.dtype == np.float64 and lost.shape == (count,)
            for b, (a, m) in enumerate(zip(states, mass_lens)):
                cb = tuple(c[b] if per_member else c) + VELOCITY
                want, want_lost = pr.model(a, m, edges, cb, weights)
                assert pr.same(got[b], want) and lost[b] == want_lost, (label, per_member, weights, b, "ensemble against the model")
                sim = nb.SimPipeline(a.shape[0], m)
                sim.set_data(a)
                alone, alone_lost = sim.profile(edges, cb[0:2], cb[2:4], weights=MODES[weights], return_unplaced=True)
                sim.close()
                assert pr.same(got[b], alone) and lost[b] == alone_lost, (label, per_member, weights, b, "ensemble against its own pipeline")


@pytest.mark.parametrize("count,n", [(5, 250), (3, 1025)])
def test_every_member_of_a_uniform_ensemble_is_its_own_pipeline_and_the_model(count, n):
    mass_lens = [(n * (b + 1)) // (count + 1) for b in range(count)]
    states = [pr.world(n, m, seed=100 + 7 * b + n) for b, m in enumerate(mass_lens)]
    batch = nb.SimBatch(n, mass_lens)
    batch.set_data(np.stack(states))
    check_members(batch, states, mass_lens, pr.log_edges(63), (count, n))
    batch.update(3, DT)          # and the state the device steps to
    stepped = list(batch.get_data())
    check_members(batch, stepped, mass_lens, pr.log_edges(7, 0.5, 60.0), (count, n, "stepped"))
    batch.close()


def test_every_member_of_a_ragged_ensemble_is_its_own_pipeline_and_the_model():
    sizes, mass_lens = [1, 333, 1024, 1025, 3000], [1, 0, 1024, 500, 3000]          # no massive particle; all massive
    states = [pr.world(n, m, seed=200 + n) for n, m in zip(sizes, mass_lens)]
    batch = nb.SimBatch.ragged(sizes, mass_lens)
    batch.set_data(states)
    check_members(batch, states, mass_lens, pr.log_edges(254), "ragged")
    assert not batch.profile(pr.log_edges(3))[1].any()          # M = 0 in mass mode: +0 everywhere
    batch.update(2, DT)
    check_members(batch, list(batch.get_data()), mass_lens, pr.log_edges(12, 0.5, 60.0), "ragged, stepped")
    batch.close()


def test_a_member_full_of_nan_changes_no_bit_of_its_neighbours():
    sizes, mass_lens = [700, 1500, 700], [400, 1500, 0]
    states = [pr.world(n, m, seed=300 + i) for i, (n, m) in enumerate(zip(sizes, mass_lens))]
    edges = pr.log_edges(20)
    batch = nb.SimBatch.ragged(sizes, mass_lens)
    batch.set_data(states)
    clean, clean_lost = batch.profile(edges, weights="number", return_unplaced=True)
    bad = [s.copy() for s in states]
    bad[1][:, 0:4] = np.nan
    batch.set_data(bad)
    got, lost = batch.profile(edges, weights="number", return_unplaced=True)
    assert got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[2].tobytes()
    assert list(clean_lost) == [0, 0, 0] and list(lost) == [0, 1500, 0] and not got[1].view(np.uint64).any()          # in no row at all
    batch.close()


def test_a_world_batch_answers_on_the_device_after_gpu_steps_and_on_the_host_before():
    members = [pr.world(n, m, seed=400 + n, spread=40.0) for n, m in ((250, 100), (1025, 1025), (3000, 1))]
    edges = pr.log_edges(16, 0.5, 200.0)
    c = centres_of(3, True)
    wb = nb.WorldBatch.ragged(members)
    before = wb.profile(edges, centre=c, centre_velocity=VELOCITY)          # never stepped: the host, member by member
    for b, a in enumerate(members):
        assert pr.same(before[b], pr.model(a, int(np.count_nonzero(a[:, 6] > 0)), edges, tuple(c[b]) + VELOCITY)[0]), b
    wb.update_gpu(DT, 2)
    got, lost = wb.profile(edges, centre=c, centre_velocity=VELOCITY, weights="number", return_unplaced=True)          # the device
    states = wb.particles()
    assert list(lost) == [0, 0, 0]
    for b, a in enumerate(states):
        m = int(np.count_nonzero(a[:, 6] > 0))
        assert pr.same(got[b], pr.model(a, m, edges, tuple(c[b]) + VELOCITY, pr.BY_NUMBER)[0]), b
        w = nb.World(a)          # the host path on the state the device held
        assert pr.same(got[b], w.profile(edges, c[b], VELOCITY, weights="number")), b
        w.close()
    wb.close()
