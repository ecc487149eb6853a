"""Friends-of-friends groups on the GPU (nb_hip_groups, group.hip): SimPipeline.groups bit for bit the numpy model (group_ref.py)
and bit for bit the host path at the tile (128), block (256), slice (32) and fetch (8) edges of the walk, over mass_len and the
three masks; the shuffled chain on both sides of the float32 edge, interleaved chains, the lattice, the all-coincident world
(every pair links: the contention case), non-finite state and a poisoned class; a linking length of zero launches nothing; every
forced span length against auto; a seeded galaxy; the same after steps, through the World on either side, and between the other
read-only calls that share the scratch.  Every comparison is of raw bits: there is no tolerance."""
import numpy as np
import pytest

import group_ref as gr
import nbody_amd as nb
from gpu_common import synth
from paircount_ref import world

pytestmark = pytest.mark.gpu

DT = 0.01
GPU_SIZES = (1, 2, 127, 128, 129, 255, 256, 257, 300, 2049)


@pytest.fixture(autouse=True)
def needs_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def pipeline(a, mass_len):
    sim = nb.SimPipeline(a.shape[0], mass_len)
    sim.set_data(a)
    return sim


def gpu_masses(n):
    return sorted({0, min(1, n), n // 3, n})


def check(sim, a, m, members, length, label, host=None):
    """The device against the model and, when given a never-stepped World, against the host path; the count with it."""
    want = gr.model(a, m, members, length)
    got, k = sim.groups(length, gr.NAMES[members], return_count=True)
    assert gr.same(got, want), (label, members, length, "device against the model")
    assert type(k) is int and k == gr.count(want), (label, members, length, "n_groups")
    if host is not None:
        assert gr.same(host.groups(length, gr.NAMES[members]), want), (label, members, length, "host path against the model")
    return got


def galaxy(n, seed):
    """(partitioned particles, mass_len, b = 0.2 of the mean separation over the bounding box) of a seeded two-galaxy world."""
    w = nb.World(nb.make_galaxies(n, 2, seed=seed, own_rng=True))
    p = w.particles()
    w.close()
    lo, hi = p[:, 0:2].min(axis=0), p[:, 0:2].max(axis=0)
    return p, int(np.count_nonzero(p[:, 6] > 0)), nb.linking_length_for(n, float(np.prod(hi - lo)), 0.2)


@pytest.mark.parametrize("n", GPU_SIZES)
def test_the_device_is_bitwise_the_model_and_the_host_path(n):
    for m in gpu_masses(n):
        a = world(n, m, seed=n, spread=3.0)
        sim, host = pipeline(a, m), nb.World(a)          # never stepped: the host path
        assert host.particles().tobytes() == a.tobytes()
        for members in gr.MASKS:
            for b in (0.5, 1.0, 2.0):
                got = check(sim, a, m, members, gr.length_for(n, b=b), (n, m), host)
                assert got.shape == (n,) and got.dtype == np.uint32
        sim.close()
        host.close()


@pytest.mark.parametrize("n", [300, 2049])
def test_the_shuffled_chain_on_both_sides_of_the_float32_edge(n):
    a, _ = gr.chain(n, seed=n)
    sim = pipeline(a, n)
    assert np.array_equal(check(sim, a, n, gr.ALL, 1.0, ("chain", n)), np.arange(n))          # q = 1 is not < 1
    assert not check(sim, a, n, gr.ALL, gr.above(1.0), ("chain", n)).any()          # one group, labelled 0, diameter n - 1
    sim.close()
    a, _ = gr.chain(n, seed=n + 1, m=n // 2)          # the chain through both classes: each class alone is in pieces
    sim = pipeline(a, n // 2)
    for members in gr.MASKS:
        check(sim, a, n // 2, members, gr.above(1.0), ("chain by class", n))
    sim.close()


def test_interleaved_chains_the_lattice_and_the_all_coincident_world():
    n = 301
    a, k = gr.two_chains(n, seed=4)
    sim = pipeline(a, n)
    lab = check(sim, a, n, gr.ALL, gr.above(2.0), "two chains")
    even, odd = np.nonzero(k % 2 == 0)[0], np.nonzero(k % 2 == 1)[0]
    assert np.all(lab[even] == even.min()) and np.all(lab[odd] == odd.min())
    assert np.array_equal(check(sim, a, n, gr.ALL, 2.0, "two chains, on the spacing"), np.arange(n))
    sim.close()
    side = 20
    a = gr.lattice(side)
    sim = pipeline(a, side * side)
    for length, one in ((0.999, False), (1.0, False), (gr.above(1.0), True), (1.5, True)):
        lab = check(sim, a, side * side, gr.ALL, length, ("lattice", length))
        assert np.array_equal(lab, np.zeros(side * side) if one else np.arange(side * side)), length
    sim.close()
    n, m = 2049, 700          # every pair links: every hook of the launch meets in one tree
    a = gr.coincident(n, m)
    sim = pipeline(a, m)
    for members in gr.MASKS:
        lo, hi = gr.span(members, n, m)
        for length in (1e-45, 1.0):
            lab = check(sim, a, m, members, length, "coincident")
            assert np.all(lab[lo:hi] == lo)
    sim.close()


def test_non_finite_state_and_a_poisoned_class_outside_the_mask():
    n, m = 300, 120
    a = world(n, m, seed=31, spread=3.0)
    length = gr.length_for(n)
    a[7, 0], a[130, 1], a[200, 0], a[201, 0] = np.nan, np.inf, -np.inf, -np.inf
    sim, host = pipeline(a, m), nb.World(a)
    for members in gr.MASKS:
        lab = check(sim, a, m, members, length, "non-finite", host)
        lo, hi = gr.span(members, n, m)
        for i in (7, 130, 200, 201):
            assert lab[i] == (i if lo <= i < hi else gr.NONE) and np.count_nonzero(lab == i) == (1 if lo <= i < hi else 0)
    sim.close()
    host.close()
    n, m = 700, 300
    a = world(n, m, seed=9, spread=3.0)
    length = gr.length_for(n)
    for members, lo, hi in ((gr.MASSIVE, m, n), (gr.MASSLESS, 0, m)):
        poisoned = a.copy()
        poisoned[lo:hi, 0:6] = np.nan          # the class outside the mask
        if members == gr.MASSLESS:
            poisoned[lo:hi, 6] = 3.0e38
        clean, dirty = pipeline(a, m), pipeline(poisoned, m)
        want = check(clean, a, m, members, length, "clean")
        assert gr.same(dirty.groups(length, gr.NAMES[members]), want), members
        clean.close()
        dirty.close()
    bridge = gr.blank(3, 2)
    bridge[:, 0] = [0.0, 2.0, 1.0]          # a massless particle between two massive ones bridges nothing
    sim = pipeline(bridge, 2)
    assert list(sim.groups(1.5, "massive")) == [0, 1, gr.NONE] and list(sim.groups(1.5)) == [0, 0, 0]
    sim.close()


def test_a_linking_length_of_zero_launches_nothing():
    n, m = 600, 200
    a = world(n, m, seed=2, spread=3.0)
    sim = pipeline(a, m)
    sim.groups(1.0)
    assert sim.last_diag_ms() > 0.0
    for members in gr.MASKS:
        lab, k = sim.groups(0.0, gr.NAMES[members], return_count=True)
        lo, hi = gr.span(members, n, m)
        assert gr.same(lab, gr.model(a, m, members, 0.0)) and k == hi - lo
        assert sim.last_diag_ms() == 0.0          # a cleared interval, as for a neighbour call without a receiver
    sim.groups(1.0)
    assert sim.last_diag_ms() > 0.0
    sim.close()
    one = pipeline(a[:1], 1)          # fewer than two particles of the mask: nothing can link
    assert list(one.groups(1.0)) == [0] and one.last_diag_ms() == 0.0
    one.close()


@pytest.mark.parametrize("n", [2049, 6000])
def test_every_forced_span_length_gives_the_bits_of_auto(n):
    """Blocks of 256 sources: N = 2 049 has 9 and N = 6 000 has 24.  A span of 1 block is one workgroup per (tile, block) of the
    triangle, 2, 3 and 5 leave ragged last spans, 1000 is one span for every tile.  The same call three times gives the same bytes."""
    a, m, length = galaxy(n, seed=n)
    sim = pipeline(a, m)
    assert nb.hip_lib().nb_hip_group_span(0) == 0
    auto = {members: sim.groups(length, gr.NAMES[members]) for members in gr.MASKS}
    assert gr.same(auto[gr.ALL], gr.model(a, m, gr.ALL, length)) and nb.group_table(auto[gr.ALL])[1][0] > 1
    last = 0
    try:
        for blocks in (1, 2, 3, 5, 1000):
            assert nb.hip_lib().nb_hip_group_span(blocks) == last
            last = blocks
            for members in gr.MASKS:
                for _ in range(3):
                    assert gr.same(sim.groups(length, gr.NAMES[members]), auto[members]), (n, blocks, members)
    finally:
        assert nb.hip_lib().nb_hip_group_span(0) == last
    sim.close()


@pytest.mark.parametrize("n", [6000, 65536])
def test_a_seeded_galaxy_against_the_host_path(n):
    a, m, length = galaxy(n, seed=7)
    sim, host = pipeline(a, m), nb.World(a)
    assert host.particles().tobytes() == a.tobytes()
    got, k = sim.groups(length, return_count=True)
    want, k_host = host.groups(length, return_count=True)
    sizes = nb.group_table(got)[1]
    print(f"[groups] N = {n}: {k} groups, the largest of {sizes[0]}, linking length {length:.4g}, {sim.last_diag_ms():.3f} ms of kernels")
    assert gr.same(got, want) and k == k_host and 1 < sizes[0] and k > 1
    if n == 6000:
        assert gr.same(got, gr.model(a, m, gr.ALL, length))
    sim.close()
    host.close()


def test_after_steps_after_leapfrog_steps_and_through_the_world_on_both_sides():
    n, m = 1500, 600
    a = world(n, m, seed=4, spread=3.0)
    length = gr.length_for(n)
    sim, plain = pipeline(a, m), pipeline(a, m)
    sim.update(3, DT)
    plain.update(3, DT)
    first = sim.groups(length)
    sim.update(2, DT)          # a call between two updates changes no bit of the later state
    plain.update(2, DT)
    assert sim.get_data().tobytes() == plain.get_data().tobytes()
    sim.update_leapfrog(2, DT)
    after_leapfrog = sim.groups(length, "massless")
    assert gr.same(after_leapfrog, gr.model(sim.get_data(), m, gr.MASSLESS, length))
    sim.close()
    plain.close()
    sim = pipeline(a, m)          # the state of the first call, read back by a pipeline that made none
    sim.update(3, DT)
    assert gr.same(first, gr.model(sim.get_data(), m, gr.ALL, length)) and gr.same(sim.groups(length), first)
    sim.close()
    w = nb.World(a)
    on_host = w.groups(length, "massive")          # the array is the newest state: the host path
    assert gr.same(on_host, gr.model(w.particles(), m, gr.MASSIVE, length))
    w.update_gpu(DT, 2)
    on_device, k = w.groups(length, "massive", return_count=True)          # the device is: the kernels, and no particle is copied back
    state = w.particles()
    assert gr.same(on_device, gr.model(state, m, gr.MASSIVE, length)) and k == gr.count(on_device)
    assert gr.same(w.groups(length, "massive"), on_device)          # now the host again, the same statement
    w.close()


# ---- between the other read-only calls: the table lies at the head of the scratch their tables share ---------------------------

R_MAX, RADIUS, LENGTH, SOFT = 8.0e3, 600.0, 250.0, 1.0


def synth_world(n, m, seed=0):
    part, _ = synth(n, frac_massive=1.1, seed=seed + n)
    part[m:, 6] = 0.0
    part[m:, 7] = 0.5
    return part


def long_lived_pipeline():
    s = nb.SimPipeline(1100, 600)
    s.set_data(synth_world(1100, 600))
    s.update(2, DT)
    return s


def long_lived_ensemble():
    sizes, mass_lens = [100, 600, 2000, 130], [50, 300, 1000, 130]
    s = nb.SimBatch.ragged(sizes, mass_lens)
    s.set_data([synth_world(n, m) for n, m in zip(sizes, mass_lens)])
    s.update(2, DT)
    return s


def long_lived_uniform():
    mass_lens = [120, 250, 1]
    s = nb.SimBatch(250, mass_lens)
    s.set_data(np.stack([synth_world(250, m, seed=b) for b, m in enumerate(mass_lens)]))
    s.update(2, DT)
    return s


def blob(out):
    if isinstance(out, (list, tuple)):
        return b"".join(blob(x) for x in out)
    return np.asarray(out).tobytes()


@pytest.mark.parametrize("make", [long_lived_pipeline, long_lived_ensemble, long_lived_uniform])
def test_groups_directly_before_and_after_the_other_read_only_calls_answer_like_a_fresh_object(make):
    v = nb.RenderView.make((0.0, 0.0), (0.0, 0.0), 0.01, 40, 30, 100.0)
    edges = nb.profile_edges(0.0, R_MAX, 16)
    calls = {
        "groups": lambda s: s.groups(LENGTH, return_count=True),
        "groups_massless": lambda s: s.groups(2 * LENGTH, "massless"),
        "neighbours": lambda s: s.neighbours(RADIUS),
        "pair_counts": lambda s: s.pair_counts(edges, classes="all", return_unplaced=True),
        "profile": lambda s: s.profile(edges, return_unplaced=True),
        "tidal_map": lambda s: s.tidal_map(v, SOFT),
    }
    if make is not long_lived_ensemble:          # ragged ensembles render nothing, by contract
        calls["render_counts"] = lambda s: s.render_counts(v)
    want = {}
    for name, call in calls.items():          # one fresh object per call, in the same state
        fresh = make()
        try:
            want[name] = blob(call(fresh))
        finally:
            fresh.close()
    others = [name for name in calls if not name.startswith("groups")]
    old = make()
    try:
        for seed in range(3):
            order = [others[i] for i in np.random.default_rng(seed).permutation(len(others))]
            for name in order:
                for step in ("groups", name, "groups_massless", name, "groups"):
                    assert blob(calls[step](old)) == want[step], (seed, name, step)
    finally:
        old.close()
