"""Radial profiles on the GPU (nb_hip_profile, profile.hip): SimPipeline.profile bit for bit the numpy model of the statement
and of its order (profile_ref.py) and bit for bit the host path, over the sizes around the chunk boundaries, every mass_len,
bins and weights of the CPU grid, the edge placements and non-finite state; the same after steps on the step routes those
sizes take; through the World on either side; twice in a row; and invisible to the steps."""
import numpy as np
import pytest

import nbody_amd as nb
import profile_ref as pr

pytestmark = pytest.mark.gpu

DT = 0.01
MODES = {pr.BY_MASS: "mass", pr.BY_NUMBER: "number"}


@pytest.fixture(autouse=True)
def needs_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def pipeline(a, mass_len, **knobs):
    sim = nb.SimPipeline(a.shape[0], mass_len)
    sim.configure(**knobs)
    sim.set_data(a)
    return sim


def host(a, edges, centre, weights):
    w = nb.World(a)          # never stepped: the host path
    assert w.particles().tobytes() == a.tobytes()
    out = w.profile(edges, centre[0:2], centre[2:4], weights=MODES[weights], return_unplaced=True)
    w.close()
    return out


def check(sim, a, mass_len, edges, centre, weights, label):
    got, lost = sim.profile(edges, centre[0:2], centre[2:4], weights=MODES[weights], return_unplaced=True)
    want, want_lost = pr.model(a, mass_len, edges, centre, weights)
    assert got.shape == want.shape and got.dtype == np.float64
    assert pr.same(got, want) and lost == want_lost, (label, "device against the model")
    on_host, host_lost = host(a, edges, centre, weights)
    assert pr.same(got, on_host) and lost == host_lost, (label, "device against the host path")
    return got


@pytest.mark.parametrize("n", pr.SIZES)
def test_the_device_is_bitwise_the_model_and_the_host_path(n):
    for mass_len in sorted({0, 1, n // 2, n}):
        a = pr.world(n, mass_len, seed=n + mass_len)
        sim = pipeline(a, mass_len)
        for bins in pr.BINS:
            for weights in (pr.BY_MASS, pr.BY_NUMBER):
                got = check(sim, a, mass_len, pr.log_edges(bins), pr.CENTRE, weights, (n, mass_len, bins, weights))
                assert got[:, 0].sum() == (mass_len if weights == pr.BY_MASS else n)
        sim.close()


def test_sixty_four_chunks_and_a_tail():
    n, mass_len = 65543, 40000
    a = pr.world(n, mass_len, seed=77)
    sim = pipeline(a, mass_len)
    for weights in (pr.BY_MASS, pr.BY_NUMBER):
        check(sim, a, mass_len, pr.log_edges(64), pr.CENTRE, weights, (n, weights))
    sim.close()


@pytest.mark.parametrize("name", list(pr.edge_case_worlds()))
def test_edge_placements_and_non_finite_state(name):
    a, mass_len, edges, centre, weights = pr.edge_case_worlds()[name]
    sim = pipeline(a, mass_len)
    got = check(sim, a, mass_len, edges, centre, weights, name)
    if name == "massless rows of NaN":
        clean = a.copy()
        clean[mass_len:, 0:6] = 0.0
        sim.set_data(clean)
        assert sim.profile(edges, centre[0:2], centre[2:4]).tobytes() == got.tobytes()          # never read: no bit changes
    sim.close()


@pytest.mark.parametrize("n,steps", [(1, 3), (250, 3), (1024, 2), (1025, 2), (3000, 2), (6000, 1)])
def test_the_same_bits_after_steps_on_the_routes_these_sizes_take(n, steps):
    """The one-workgroup chain of small worlds, plain launches, and a chain length's second use (its cached graph)."""
    mass_len = n // 2 + 1
    a = pr.world(n, mass_len, seed=90 + n, spread=40.0)
    sim = pipeline(a, mass_len)
    edges = pr.log_edges(24, 0.5, 200.0)
    for call in range(3):
        sim.update(steps, DT)
        state = sim.get_data()
        assert np.array_equal(state[:, 6:8], a[:, 6:8])
        for weights in (pr.BY_MASS, pr.BY_NUMBER):
            check(sim, state, mass_len, edges, pr.CENTRE, weights, (n, call, weights))
    sim.close()


def test_a_world_answers_from_the_device_after_gpu_steps_and_from_the_host_after_cpu_steps():
    a = pr.world(2049, 1200, seed=5, spread=40.0)
    edges = pr.log_edges(32, 0.5, 200.0)
    w = nb.World(a)
    w.update_gpu(DT, 2)
    got, lost = w.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4], return_unplaced=True)
    ms = float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline()))
    assert ms > 0.0          # the device path ran
    state = w.particles()
    on_host, host_lost = host(state, edges, pr.CENTRE, pr.BY_MASS)
    assert pr.same(got, on_host) and lost == host_lost == 0 and pr.same(got, pr.model(state, 1200, edges, pr.CENTRE)[0])
    w.update_cpu(DT, 1)          # the array is newer now: the same call runs on the host and leaves the timer alone
    after = w.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4], weights="number")
    assert float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline())) == ms
    assert pr.same(after, pr.model(w.particles(), 1200, edges, pr.CENTRE, pr.BY_NUMBER)[0])
    w.update_gpu(DT, 1)          # and back on the device
    again = w.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4], weights="number")
    assert pr.same(again, pr.model(w.particles(), 1200, edges, pr.CENTRE, pr.BY_NUMBER)[0])
    w.close()


def test_two_calls_in_a_row_and_a_call_between_two_updates_change_no_bit():
    a = pr.world(3000, 1700, seed=6, spread=40.0)
    edges = pr.log_edges(40, 0.5, 200.0)
    x, y = pipeline(a, 1700, timing=1), pipeline(a, 1700, timing=1)
    for s in (x, y):
        s.update(2, DT)
        s.update(2, DT)          # the chain length's second use: cached from here on
    step_ms, stats = x.last_step_ms(), x.graph_stats()
    first = x.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4])
    assert x.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4]).tobytes() == first.tobytes()
    other = x.profile(pr.log_edges(254), weights="number")          # another shape of the same buffers in between
    assert x.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4]).tobytes() == first.tobytes() and other.shape == (256, 6)
    assert x.last_step_ms() == step_ms and x.graph_stats() == stats and x.last_diag_ms() > 0.0
    assert x.get_data().tobytes() == y.get_data().tobytes()
    x.update(2, DT)
    y.update(2, DT)
    assert x.get_data().tobytes() == y.get_data().tobytes()          # the trajectory never saw the calls
    assert y.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4]).tobytes() == x.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4]).tobytes()
    x.close()
    y.close()


def test_nothing_to_read_gives_zeros_and_touches_no_timer():
    a = pr.world(300, 0, seed=8)
    sim = pipeline(a, 0)
    rows, lost = sim.profile(pr.log_edges(5), return_unplaced=True)          # mass mode, no massive particle
    assert rows.shape == (7, 6) and not rows.view(np.uint64).any() and lost == 0 and sim.last_diag_ms() == 0.0
    assert sim.profile(pr.log_edges(5), weights="number")[:, 0].sum() == 300 and sim.last_diag_ms() > 0.0
    sim.close()
