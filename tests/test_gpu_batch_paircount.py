"""Pair-separation counts of ensembles on the GPU (nb_hip_ensemble_pair_counts, paircount.hip): every member of a uniform or
ragged SimBatch bit for bit its own SimPipeline.pair_counts and the numpy model (paircount_ref.py), every class subset; a member
full of NaN changes no bit of its neighbours; WorldBatch.pair_counts on the device and on the host.

The call is one launch of one kernel by construction (paircount.hip has a single kernel, and nb_hip_ensemble_pair_counts
enqueues it once for all members).  The seam has no launch counter for the diagnostics (the profile and field batch tests assert
none either), so nothing is asserted about it here."""
import numpy as np
import pytest

import nbody_amd as nb
import paircount_ref as pr

pytestmark = pytest.mark.gpu

DT = 0.01


@pytest.fixture(autouse=True)
def needs_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def check_members(batch, states, mass_lens, edges, label, subsets=pr.SUBSETS):
    """Every member of `batch` (holding `states`) against the model and against its own pipeline, for every class subset."""
    count = len(states)
    want = [pr.model(a, m, edges) for a, m in zip(states, mass_lens)]
    pipes = []
    for a, m in zip(states, mass_lens):
        pipes.append(nb.SimPipeline(a.shape[0], m))
        pipes[-1].set_data(a)
    for classes in subsets:
        got, lost = batch.pair_counts(edges, pr.names(classes), return_unplaced=True)
        assert got.shape == (count, len(edges) + 1, 3) and got.dtype == np.uint64 and lost.shape == (count, 3)
        for b, (a, m) in enumerate(zip(states, mass_lens)):
            w, wl = pr.masked(*want[b], classes)
            assert pr.same(got[b], w) and pr.same(lost[b], wl), (label, classes, b, "ensemble against the model")
            assert pr.sums_to_class_totals(got[b], lost[b], a.shape[0], m, classes), (label, classes, b)
            alone, alone_lost = pipes[b].pair_counts(edges, pr.names(classes), return_unplaced=True)
            assert pr.same(got[b], alone) and pr.same(lost[b], alone_lost), (label, classes, b, "ensemble against its own pipeline")
    for s in pipes:
        s.close()


@pytest.mark.parametrize("count", [1, 3, 256])
@pytest.mark.parametrize("n", [1, 2, 250, 513, 3000])
def test_every_member_of_a_uniform_ensemble_is_its_own_pipeline_and_the_model(count, n):
    mass_lens = [(n * (b % 7 + 1)) // 8 if b % 5 else (0 if b % 2 else n) for b in range(count)]          # 0 and n among them
    states = [pr.world(n, m, seed=100 + 7 * b + n) for b, m in enumerate(mass_lens)]
    batch = nb.SimBatch(n, mass_lens)
    batch.set_data(np.stack(states))
    if count == 256 and n > 250:          # the model of 256 large members takes too long: the first, the last and two between
        keep = [0, 101, 202, 255]
        got, lost = batch.pair_counts(pr.log_edges(64), "all", return_unplaced=True)
        for b in keep:
            want, want_lost = pr.model(states[b], mass_lens[b], pr.log_edges(64))
            assert pr.same(got[b], want) and pr.same(lost[b], want_lost), (count, n, b)
        for b, (a, m) in enumerate(zip(states, mass_lens)):          # every member against its own pipeline
            sim = nb.SimPipeline(n, m)
            sim.set_data(a)
            alone, alone_lost = sim.pair_counts(pr.log_edges(64), "all", return_unplaced=True)
            sim.close()
            assert pr.same(got[b], alone) and pr.same(lost[b], alone_lost), (count, n, b, "ensemble against its own pipeline")
        totals = np.array([[pr.pair_total(c, n, m) for c in range(3)] for m in mass_lens], dtype=np.uint64)
        assert np.array_equal(got.sum(axis=1) + lost, totals)          # and every member sums to its class totals
    else:
        check_members(batch, states, mass_lens, pr.log_edges(64), (count, n), subsets=pr.SUBSETS if count < 256 else (pr.ALL, pr.MM | pr.TT))
    batch.close()


def test_every_member_of_a_ragged_ensemble_is_its_own_pipeline_and_the_model():
    sizes, mass_lens = [1, 2, 65, 250, 1000, 3000], [1, 0, 65, 100, 999, 1500]
    states = [pr.world(n, m, seed=200 + n) for n, m in zip(sizes, mass_lens)]
    batch = nb.SimBatch.ragged(sizes, mass_lens)
    batch.set_data(states)
    check_members(batch, states, mass_lens, pr.log_edges(254), "ragged")
    batch.update(2, DT)          # and the state the device steps to
    check_members(batch, list(batch.get_data()), mass_lens, pr.lin_edges(7), "ragged, stepped", subsets=(pr.ALL, pr.MT))
    batch.close()


def test_a_member_full_of_nan_changes_no_bit_of_its_neighbours():
    sizes, mass_lens = [700, 1500, 700], [400, 800, 0]
    states = [pr.world(n, m, seed=300 + i) for i, (n, m) in enumerate(zip(sizes, mass_lens))]
    edges = pr.log_edges(20)
    batch = nb.SimBatch.ragged(sizes, mass_lens)
    batch.set_data(states)
    clean, clean_lost = batch.pair_counts(edges, "all", return_unplaced=True)
    bad = [s.copy() for s in states]
    bad[1][:, 0:4] = np.nan
    batch.set_data(bad)
    got, lost = batch.pair_counts(edges, "all", return_unplaced=True)
    assert got[0].tobytes() == clean[0].tobytes() and got[2].tobytes() == clean[2].tobytes()
    assert not clean_lost.any() and not lost[0].any() and not lost[2].any() and not got[1].any()          # in no row at all
    assert list(lost[1]) == [pr.pair_total(c, 1500, 800) for c in range(3)]
    batch.close()


def test_a_world_batch_answers_on_the_device_after_gpu_steps_and_on_the_host_before():
    members = [pr.world(n, m, seed=400 + n, spread=40.0) for n, m in ((250, 100), (1025, 1025), (3000, 1))]
    edges = pr.log_edges(16, 0.5, 200.0)
    wb = nb.WorldBatch.ragged(members)
    before = wb.pair_counts(edges, "all")          # never stepped: the host, member by member
    for b, a in enumerate(members):
        assert pr.same(before[b], pr.model(a, int(np.count_nonzero(a[:, 6] > 0)), edges)[0]), b
    wb.update_gpu(DT, 2)
    got, lost = wb.pair_counts(edges, "all", return_unplaced=True)          # the device
    states = wb.particles()
    assert not lost.any()
    for b, a in enumerate(states):
        m = int(np.count_nonzero(a[:, 6] > 0))
        assert pr.same(got[b], pr.model(a, m, edges)[0]), b
        w = nb.World(a)          # the host path on the state the device held
        assert pr.same(got[b], w.pair_counts(edges, "all")), b
        w.close()
    wb.close()
