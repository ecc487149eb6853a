"""Nearest neighbours and neighbour counts on the GPU (nb_hip_neighbours, neighbour.hip): SimPipeline.neighbours bit for bit the
numpy model (neighbour_ref.py) and bit for bit the host path at the tile, block and wave-slice edges, over mass_len, the nine mask
combinations, with and without a radius; forced span lengths against auto; the lattice, the coincident world, non-finite state and
a poisoned unrequested class; the same after steps, through the World on either side, between energy() and pair_counts(); and
invisible to the steps.  Every comparison is of raw bits: there is no tolerance."""
import numpy as np
import pytest

import nbody_amd as nb
import neighbour_ref as nr
from paircount_ref import log_edges, world

pytestmark = pytest.mark.gpu

DT = 0.01
RADIUS = 1.5
GPU_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, 2049, 4099)
COMBOS = [(r, s) for r in nr.MASKS for s in nr.MASKS]


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


def check(sim, a, m, r, s, radius, label, host=None):
    """With and without the count against the model and, when given a never-stepped World, against the host path."""
    names = (nr.NAMES[r], nr.NAMES[s])
    want = nr.model(a, m, r, s, radius)
    got = sim.neighbours(radius, *names)
    assert len(got) == 3 and nr.same(got, want), (label, names, "device against the model")
    assert nr.same(sim.neighbours(None, *names), want[:2]), (label, names, "without the count")
    if host is not None:
        assert nr.same(host.neighbours(radius, *names), want), (label, names, "host path against the model")
    return got


@pytest.mark.parametrize("n", GPU_SIZES)
def test_the_device_is_bitwise_the_model_and_the_host_path(n):
    for m in gpu_masses(n):
        a = world(n, m, seed=n)
        sim, host = pipeline(a, m), nb.World(a)          # never stepped: the host path
        assert host.particles().tobytes() == a.tobytes()
        for r, s in COMBOS:
            q, index, count = check(sim, a, m, r, s, RADIUS, (n, m), host)
            assert q.shape == (n,) and q.dtype == np.float32 and index.dtype == np.uint32 and count.dtype == np.uint32
        sim.close()
        host.close()


@pytest.mark.parametrize("n,m", [(1000, 333), (4099, 1366)])
def test_every_forced_span_length_gives_the_bits_of_auto(n, m):
    """Blocks of 256 sources: N = 1 000 has 4 and N = 4 099 has 17.  A span of 1 block is one workgroup per block, 2 and 3 are
    several spans, and 3 leaves a ragged last span at both sizes (4 = 3 + 1, 17 = 5 x 3 + 2).  Massless sources begin inside a
    block, so the first span of theirs does too."""
    a = world(n, m, seed=n + 1)
    sim = pipeline(a, m)
    assert nb.hip_lib().nb_hip_neighbour_span(0) == 0
    auto = {(r, s): sim.neighbours(RADIUS, nr.NAMES[r], nr.NAMES[s]) for r, s in COMBOS}
    assert nr.same(auto[nr.ALL, nr.ALL], nr.model(a, m, nr.ALL, nr.ALL, RADIUS))
    try:
        for blocks in (1, 2, 3):
            nb.hip_lib().nb_hip_neighbour_span(blocks)
            for r, s in COMBOS:
                assert nr.same(sim.neighbours(RADIUS, nr.NAMES[r], nr.NAMES[s]), auto[r, s]), (n, blocks, r, s)
                assert nr.same(sim.neighbours(None, nr.NAMES[r], nr.NAMES[s]), auto[r, s][:2]), (n, blocks, r, s)
    finally:
        assert nb.hip_lib().nb_hip_neighbour_span(0) == 3
    sim.close()


def test_the_lattice_the_coincident_world_and_the_radius_at_a_separation():
    side = 20
    a = nr.lattice(side)
    sim = pipeline(a, side * side)
    q, index, count = check(sim, a, side * side, nr.ALL, nr.ALL, 1.25, "lattice")
    i = np.arange(side * side)
    inner = (i // side > 0) & (i // side < side - 1) & (i % side > 0) & (i % side < side - 1)
    assert np.all(q == 1.0) and np.array_equal(index[inner], (i - side)[inner]) and np.all(count[inner] == 4)          # four at q = 1: the smallest index
    assert index[0] == 1 and count[0] == 2
    assert nb.closest_pairs(q, index, 3) == [(0, 1, 1.0), (0, side, 1.0), (1, 2, 1.0)]
    sim.close()
    n, m = 300, 100
    a = nr.coincident(n, m)
    sim = pipeline(a, m)
    for r, s in COMBOS:
        q, index, count = check(sim, a, m, r, s, 0.5, "coincident")
        r0, r1 = nr.span(r, n, m)
        s0, s1 = nr.span(s, n, m)
        rows = np.arange(r0, r1)
        assert np.all(q[r0:r1] == 0.0) and not np.signbit(q[r0:r1]).any()
        assert np.array_equal(index[r0:r1], np.where(rows == s0, s0 + 1, s0))          # the smallest other index
        assert np.array_equal(count[r0:r1], (s1 - s0) - ((rows >= s0) & (rows < s1)))          # every candidate
    assert not sim.neighbours(0.0)[2].any()          # q = +0 is not < 0
    sim.close()
    a = world(3, 3, seed=2)
    a[:, 0:2] = [[0.0, 0.0], [3.0, 0.0], [0.0, 40.0]]
    sim = pipeline(a, 3)
    three = np.float32(3.0)
    for radius, within in ((np.nextafter(three, np.float32(0)), 0), (three, 0), (np.nextafter(three, np.float32(9)), 1)):
        got = check(sim, a, 3, nr.ALL, nr.ALL, float(radius), ("radius", radius))
        assert list(got[2]) == [within, within, 0] and list(got[0][:2]) == [9.0, 9.0]
    sim.close()


def test_non_finite_state_and_a_poisoned_unrequested_class():
    for name, (a, m) in nr.nonfinite_worlds().items():
        sim, host = pipeline(a, m), nb.World(a)
        for r, s in COMBOS:
            q, index, count = check(sim, a, m, r, s, RADIUS, name, host)
            bad = ~np.isfinite(a[:, 0]) | ~np.isfinite(a[:, 1])
            assert np.all(np.isposinf(q[bad])) and np.all(index[bad] == nr.NONE) and not count[bad].any(), name          # an own NaN or inf
            assert not np.isin(index[index != nr.NONE], np.nonzero(bad)[0]).any(), name          # and nobody's neighbour
        if name == "nobody has a candidate":
            q, index, count = sim.neighbours(RADIUS)
            assert np.all(np.isposinf(q)) and np.all(index == nr.NONE) and not count.any()
        sim.close()
        host.close()
    n, m = 700, 300
    a = world(n, m, seed=9)
    for r, s, lo, hi in ((nr.MASSIVE, nr.MASSIVE, m, n), (nr.MASSLESS, nr.MASSLESS, 0, m)):
        poisoned = a.copy()
        poisoned[lo:hi, 0:6] = np.nan          # the class that is neither receiver nor source
        clean, dirty = pipeline(a, m), pipeline(poisoned, m)
        want = clean.neighbours(RADIUS, nr.NAMES[r], nr.NAMES[s])
        assert nr.same(want, nr.model(a, m, r, s, RADIUS))
        assert nr.same(dirty.neighbours(RADIUS, nr.NAMES[r], nr.NAMES[s]), want), (r, s)
        assert not nr.checker(dirty.neighbours(RADIUS, nr.NAMES[r], nr.NAMES[s]), poisoned, m, r, s, RADIUS, variant="unrequested_read")
        clean.close()
        dirty.close()


def test_after_steps_the_state_comes_from_the_device_and_the_call_is_invisible_to_the_steps():
    n, m = 1500, 600
    a = world(n, m, seed=4)
    sim, plain = pipeline(a, m), pipeline(a, m)
    sim.update(3, DT)
    plain.update(3, DT)
    first = sim.neighbours(RADIUS)
    again = sim.neighbours(RADIUS, "massless", "massive")
    sim.update(2, DT)          # a call between two updates changes no bit of the later state
    plain.update(2, DT)
    assert sim.get_data().tobytes() == plain.get_data().tobytes()
    sim.close()
    plain.close()
    sim = pipeline(a, m)          # the state of the first calls, read back by a pipeline that made none
    sim.update(3, DT)
    state = sim.get_data()
    assert nr.same(first, nr.model(state, m, nr.ALL, nr.ALL, RADIUS)) and nr.same(again, nr.model(state, m, nr.MASSLESS, nr.MASSIVE, RADIUS))
    assert nr.same(sim.neighbours(RADIUS), first)
    sim.close()


def test_through_the_world_on_both_sides_of_its_coherence_and_between_other_read_only_calls():
    n, m = 900, 400
    a = world(n, m, seed=6)
    w = nb.World(a)
    on_host = w.neighbours(RADIUS, "massive", "all")          # the array is the newest state: the host path
    assert nr.same(on_host, nr.model(w.particles(), m, nr.MASSIVE, nr.ALL, RADIUS))
    w.update_gpu(DT, 2)
    on_device = w.neighbours(RADIUS, "massive", "all")          # the device is: the kernel, and no particle is copied back for it
    state = w.particles()
    assert nr.same(on_device, nr.model(state, m, nr.MASSIVE, nr.ALL, RADIUS)) and not nr.same(on_device, on_host)
    assert nr.same(w.neighbours(RADIUS, "massive", "all"), on_device)          # now the host again, the same statement
    w.close()
    sim = pipeline(a, m)          # one scratch serves every read-only call: each reads only what it wrote
    edges = log_edges(16)
    want, energy, pairs = sim.neighbours(RADIUS), sim.energy(), sim.pair_counts(edges, "all")
    for _ in range(2):
        assert nr.same(sim.neighbours(RADIUS), want)
        assert sim.energy() == energy
        assert nr.same(sim.neighbours(None, "massless"), nr.model(a, m, nr.MASSLESS, nr.ALL)[:2])
        assert np.array_equal(sim.pair_counts(edges, "all"), pairs)
        assert sim.last_diag_ms() > 0.0
    sim.close()
