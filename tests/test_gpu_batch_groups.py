"""Friends-of-friends groups of ensembles on the GPU (nb_hip_ensemble_groups, group.hip): every member of a uniform or ragged
SimBatch bit for bit its own SimPipeline.groups, the numpy model (group_ref.py) and the host path, over the three masks and for
forced span lengths; labels count within the member, members on top of one another share no group, n_groups per member; and
WorldBatch.groups on the host and on the device.  Every comparison is of raw bits: there is no tolerance."""
import numpy as np
import pytest

import group_ref as gr
import nbody_amd as nb
from paircount_ref import world

pytestmark = pytest.mark.gpu

DT = 0.01


@pytest.fixture(autouse=True)
def needs_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def check_members(batch, host, states, mass_lens, length, label):
    """Every member of `batch` against its own pipeline, the model and the host path through the never-stepped WorldBatch `host`."""
    pipes = []
    for a, m in zip(states, mass_lens):
        pipes.append(nb.SimPipeline(a.shape[0], m))
        pipes[-1].set_data(a)
    for members in gr.MASKS:
        name = gr.NAMES[members]
        (got, k), on_host = batch.groups(length, name, return_count=True), host.groups(length, name)
        assert k.dtype == np.uint32 and k.shape == (len(states),)
        for b, (a, m) in enumerate(zip(states, mass_lens)):
            want = gr.model(a, m, members, length)
            assert gr.same(got[b], want), (label, name, b, "ensemble against the model")
            alone, k_alone = pipes[b].groups(length, name, return_count=True)
            assert gr.same(got[b], alone) and k[b] == k_alone == gr.count(want), (label, name, b, "ensemble against its own pipeline")
            assert gr.same(on_host[b], want), (label, name, b, "host path")
            lo, hi = gr.span(members, len(a), m)
            assert np.all(got[b][lo:hi] <= np.arange(lo, hi)), (label, name, b, "labels count within the member")
    for p in pipes:
        p.close()


@pytest.mark.parametrize("count,n", [(5, 300), (256, 250)])
def test_every_member_of_a_uniform_ensemble_is_its_own_pipeline_the_model_and_the_host_path(count, n):
    mass_lens = [(0, n // 3, n, 1, n - 1)[b % 5] for b in range(count)]
    states = [world(n, m, seed=200 + 7 * b + n, spread=3.0) for b, m in enumerate(mass_lens)]
    length = gr.length_for(n)
    batch, host = nb.SimBatch(n, mass_lens), nb.WorldBatch(np.stack(states))
    batch.set_data(np.stack(states))
    got = batch.groups(length)
    assert got.shape == (count, n) and got.dtype == np.uint32
    if count <= 5:
        check_members(batch, host, states, mass_lens, length, (count, n))
    else:          # 256 members: against the model and the host path; their own pipelines are the perf test's loop
        on_host, k = host.groups(length, return_count=True)
        assert gr.same(got, on_host) and all(gr.same(got[b], gr.model(states[b], mass_lens[b], gr.ALL, length)) for b in range(count))
        assert np.array_equal(batch.groups(length, return_count=True)[1], k) and k.shape == (count,)
    try:
        for blocks in (1, 2, 5):
            nb.hip_lib().nb_hip_group_span(blocks)
            assert gr.same(batch.groups(length), got), (count, n, blocks)
    finally:
        nb.hip_lib().nb_hip_group_span(0)
    batch.close()
    host.close()


def test_every_member_of_a_ragged_ensemble_is_its_own_pipeline_the_model_and_the_host_path():
    sizes, mass_lens = (1, 2, 129, 300, 2049), (1, 0, 43, 300, 700)
    states = [world(n, m, seed=300 + n, spread=3.0) for n, m in zip(sizes, mass_lens)]
    length = gr.length_for(300)
    batch, host = nb.SimBatch.ragged(sizes, mass_lens), nb.WorldBatch.ragged(states)
    batch.set_data(states)
    got = batch.groups(length)
    assert isinstance(got, list) and [x.shape for x in got] == [(n,) for n in sizes] and all(x.flags.owndata for x in got)
    check_members(batch, host, states, mass_lens, length, "ragged")
    try:
        for blocks in (1, 5):
            nb.hip_lib().nb_hip_group_span(blocks)
            again = batch.groups(length)
            assert all(gr.same(again[b], got[b]) for b in range(len(sizes))), blocks
    finally:
        nb.hip_lib().nb_hip_group_span(0)
    batch.close()
    host.close()


def test_members_on_top_of_one_another_share_no_group_and_labels_are_member_local():
    n = 300
    chain, _ = gr.chain(n, seed=5)
    states = [chain, chain.copy(), gr.coincident(n), gr.coincident(n)]          # neighbours in the packed arrays, at the same places
    batch = nb.SimBatch(n, [n] * 4)
    batch.set_data(np.stack(states))
    lab, k = batch.groups(gr.above(1.0), return_count=True)
    assert not lab.any() and list(k) == [1, 1, 1, 1]          # each member one group, named by ITS index 0
    want = gr.ensemble(states, [n] * 4, gr.ALL, gr.above(1.0))
    assert all(gr.same(lab[b], want[b]) for b in range(4))
    assert not all(gr.same(lab[b], w) for b, w in enumerate(gr.ensemble(states, [n] * 4, gr.ALL, gr.above(1.0), variant="global_labels")))
    lab, k = batch.groups(1.0, return_count=True)          # on the spacing the chains fall apart, the coincident members do not
    assert list(k) == [n, n, 1, 1] and np.array_equal(lab[0], np.arange(n)) and not lab[2].any()
    batch.close()


def test_a_world_batch_answers_on_the_device_once_it_has_stepped_there():
    sizes = (129, 300, 700)
    states = [world(n, n // 2, seed=400 + n, spread=3.0) for n in sizes]
    length = gr.length_for(300)
    wb = nb.WorldBatch.ragged(states)
    before = wb.groups(length, "massive")          # the host path
    wb.update_gpu(DT, 2)
    on_device, k = wb.groups(length, "massive", return_count=True)          # the device holds the newest state
    after = wb.particles()
    for b, n in enumerate(sizes):
        assert gr.same(before[b], gr.model(states[b], n // 2, gr.MASSIVE, length)), b
        assert gr.same(on_device[b], gr.model(after[b], n // 2, gr.MASSIVE, length)) and k[b] == gr.count(on_device[b]), b
    wb.close()
    uniform = nb.WorldBatch(np.stack([world(250, 100, seed=s, spread=3.0) for s in range(3)]))
    uniform.update_gpu(DT, 1)
    lab, k = uniform.groups(gr.length_for(250), return_count=True)
    state = uniform.particles()
    assert lab.shape == (3, 250) and all(gr.same(lab[b], gr.model(state[b], 100, gr.ALL, gr.length_for(250))) and k[b] == gr.count(lab[b]) for b in range(3))
    uniform.close()
