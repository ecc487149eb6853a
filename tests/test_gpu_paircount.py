"""Pair-separation counts on the GPU (nb_hip_pair_counts, paircount.hip): SimPipeline.pair_counts bit for bit the numpy model
(paircount_ref.py) and bit for bit the host path over the sizes of the CPU grid and beyond, every mass_len, class subset and
bins; one size at which every loop level of the launch runs more than once and ends in a partial piece; the edge placements and
non-finite state; all particles coincident; the wave-uniform shortcuts; the same after steps on the step routes those sizes
take, through the World on either side, twice in a row, between energy() and profile(); and invisible to the steps."""
import numpy as np
import pytest

import nbody_amd as nb
import paircount_ref as pr

pytestmark = pytest.mark.gpu

DT = 0.01
GPU_BINS = (1, 7, 64, 254)
GPU_SIZES = pr.SIZES + (511, 513, 2049, 6000)


@pytest.fixture(autouse=True)
def needs_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def pipeline(a, mass_len, **knobs):
    sim = nb.SimPipeline(a.shape[0], mass_len)
    sim.configure(**knobs)
    sim.set_data(a)
    return sim


def host(a, edges, classes=pr.ALL):
    w = nb.World(a)          # never stepped: the host path
    assert w.particles().tobytes() == a.tobytes()
    out = w.pair_counts(edges, pr.names(classes), return_unplaced=True)
    w.close()
    return out


def check_all_subsets(sim, n, m, edges, want, want_lost, label):
    """Every class subset on the device against what the result of classes = ALL says of it."""
    for classes in pr.SUBSETS:
        got, lost = sim.pair_counts(edges, pr.names(classes), return_unplaced=True)
        w, wl = pr.masked(want, want_lost, classes)
        assert got.shape == w.shape and pr.same(got, w) and pr.same(lost, wl), (label, classes, "device against the model")
        assert pr.sums_to_class_totals(got, lost, n, m, classes), (label, classes)


def check(sim, a, m, edges, label, classes=pr.ALL):
    """One call against the model and against the host path."""
    got, lost = sim.pair_counts(edges, pr.names(classes), return_unplaced=True)
    want, want_lost = pr.model(a, m, edges, classes)
    assert pr.same(got, want) and pr.same(lost, want_lost), (label, "device against the model")
    on_host, host_lost = host(a, edges, classes)
    assert pr.same(got, on_host) and pr.same(lost, host_lost), (label, "device against the host path")
    assert pr.sums_to_class_totals(got, lost, a.shape[0], m, classes), label
    return got, lost


@pytest.mark.parametrize("n", GPU_SIZES)
def test_the_device_is_bitwise_the_model_and_the_host_path(n):
    sets = [pr.log_edges(b) for b in GPU_BINS]
    grid = pr.model_grid(pr.world(n, 0, seed=n), pr.masses(n), sets)          # the positions do not depend on M: every pair once
    for m in pr.masses(n):
        a = pr.world(n, m, seed=n)
        sim = pipeline(a, m)
        for k, edges in enumerate(sets):
            want, want_lost = grid[m, k]
            check_all_subsets(sim, n, m, edges, want, want_lost, (n, m, GPU_BINS[k]))
            on_host, host_lost = host(a, edges)
            assert pr.same(on_host, want) and pr.same(host_lost, want_lost), (n, m, GPU_BINS[k], "host path against the model")
        sim.close()


def test_every_loop_level_runs_more_than_once_and_ends_in_a_partial_piece():
    """N = 7 777, M = 4 300.  Receiver tiles of 128: 34 massive and 28 massless ones, the last of each partial, and M is no
    multiple of 128, so the massless tiles begin inside a tile.  Source blocks of 256: 17 in MM (the last holds 204), blocks
    16 .. 30 in TT and MT (the first holds 52 sources from an index that is no multiple of 8: single loads before the groups
    of 8; the last holds 97).
    Wave slices: 17 blocks over 8 waves are 3, 3, 3, 3, 3, 2, 0, 0; the 15 of TT and MT 2 x 7 and 1.  The diagonal block is
    masked in every tile of MM and TT, the first tile of a block and the second.  The flush: 96 workgroups add to one table (a
    second span of sources needs N > 2^20, which no model finishes in seconds; the span arithmetic is the tile arithmetic)."""
    n, m = 7777, 4300
    a = pr.world(n, m, seed=7)
    sets = [pr.log_edges(64), pr.lin_edges(7)]
    grid = pr.model_grid(a, [m], sets)
    sim = pipeline(a, m)
    for k, edges in enumerate(sets):
        check_all_subsets(sim, n, m, edges, *grid[m, k], (n, m, k))
        on_host, host_lost = host(a, edges)
        assert pr.same(on_host, grid[m, k][0]) and pr.same(host_lost, grid[m, k][1])
    sim.close()


@pytest.mark.parametrize("name", list(pr.edge_pairs()))
def test_a_pair_on_below_and_above_an_edge(name):
    a, edges, row = pr.edge_pairs()[name]
    sim = pipeline(a, 2)
    got, lost = check(sim, a, 2, edges, name)
    assert got[row, 0] == 1 and got.sum() == 1 and not lost.any(), (name, got[:, 0])
    sim.close()


def test_the_star_of_edge_offsets_the_fused_witness_and_non_finite_state():
    a, m, edges = pr.edge_star()
    sim = pipeline(a, m)
    check(sim, a, m, edges, "star")
    sim.close()
    a, m, edges = pr.fused_world()
    sim = pipeline(a, m)
    got, lost = check(sim, a, m, edges, "fused witness")
    assert not pr.same(got, pr.model(a, m, edges, variant="fused")[0])          # the device did not contract q
    sim.close()
    for name, (a, m, edges, classes) in pr.nonfinite_worlds().items():
        sim = pipeline(a, m)
        got, lost = check(sim, a, m, edges, name, classes)
        if name == "two at +inf on one axis":
            assert list(lost) == [0, 1, 0]
        if name == "massless rows of NaN, mm only":
            clean = a.copy()
            clean[m:, 0:6] = 0.0
            sim.set_data(clean)
            assert sim.pair_counts(edges, "mm").tobytes() == got.tobytes() and not lost.any()          # never read: no bit changes
        sim.close()


def test_all_particles_coincident():
    """N = 2 049 at one place: every pair has q = +0 and falls in one row -- the merged add of a wave, on every wave."""
    n, m = 2049, 1000
    a = pr.world(n, m, seed=12)
    a[:, 0:2] = (3.25, -1.5)
    sim = pipeline(a, m)
    for edges, row in ((pr.log_edges(64), 0), (pr.lin_edges(64), 1), (np.array([0.0, 1.0], dtype=np.float32), 1)):
        got, lost = sim.pair_counts(edges, "all", return_unplaced=True)
        assert list(got[row]) == [pr.pair_total(c, n, m) for c in range(3)] and got.sum() == n * (n - 1) // 2 and not lost.any(), row
    mixed = a.copy()          # half of them a little apart: rows shared by many lanes but not all
    mixed[::2, 0] += np.float32(0.125)
    sim.set_data(mixed)
    check(sim, mixed, m, pr.lin_edges(64, 1.0), "two clumps")
    sim.close()


def test_the_wave_uniform_shortcuts():
    """All pairs inside the first edge, all beyond the last, and a world where only some waves qualify."""
    n, m = 1500, 700
    a = pr.world(n, m, seed=13)
    sim = pipeline(a, m)
    totals = [pr.pair_total(c, n, m) for c in range(3)]
    inside = np.array([1e3, 2e3, 3e3], dtype=np.float32)
    got, lost = check(sim, a, m, inside, "inside the first edge")
    assert list(got[0]) == totals and not got[1:].any()
    beyond = np.array([1e-6, 2e-6, 3e-6], dtype=np.float32)
    got, lost = check(sim, a, m, beyond, "beyond the last edge")
    assert list(got[3]) == totals and not got[:3].any()
    check(sim, a, m, np.array([0.0, 0.5, 1.0], dtype=np.float32), "r_max far below the system size")
    check(sim, a, m, np.array([30.0, 35.0, 60.0], dtype=np.float32), "r_min far above the typical separation")
    sim.close()


@pytest.mark.parametrize("n,steps", [(2, 3), (250, 3), (1025, 2), (3000, 2), (6000, 1)])
def test_the_same_counts_after_steps_on_the_routes_these_sizes_take(n, steps):
    """The one-workgroup chain of small worlds, plain launches, and a chain length's second use (its cached graph)."""
    m = n // 2 + 1
    a = pr.world(n, m, seed=90 + n, spread=40.0)
    sim = pipeline(a, m)
    edges = pr.log_edges(24, 0.5, 200.0)
    for call in range(3):
        sim.update(steps, DT)
        state = sim.get_data()
        check(sim, state, m, edges, (n, call))
    sim.close()


def test_a_world_answers_from_the_device_after_gpu_steps_and_from_the_host_after_cpu_steps():
    a = pr.world(2049, 1200, seed=5, spread=40.0)
    edges = pr.log_edges(32, 0.5, 200.0)
    w = nb.World(a)
    w.update_gpu(DT, 2)
    got, lost = w.pair_counts(edges, "all", return_unplaced=True)
    ms = float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline()))
    assert ms > 0.0          # the device path ran
    state = w.particles()
    on_host, host_lost = host(state, edges)
    assert pr.same(got, on_host) and not lost.any() and not host_lost.any() and pr.same(got, pr.model(state, 1200, edges)[0])
    w.update_cpu(DT, 1)          # the array is newer now: the same call runs on the host and leaves the timer alone
    after = w.pair_counts(edges, ("mm", "tt"))
    assert float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline())) == ms
    assert pr.same(after, pr.model(w.particles(), 1200, edges, pr.MM | pr.TT)[0])
    w.update_gpu(DT, 1)          # and back on the device
    again = w.pair_counts(edges, "mt")
    assert pr.same(again, pr.model(w.particles(), 1200, edges, pr.MT)[0])
    w.close()


def test_two_calls_in_a_row_between_energy_and_profile_and_between_two_updates_change_no_bit():
    a = pr.world(3000, 1700, seed=6, spread=40.0)
    edges = pr.log_edges(40, 0.5, 200.0)
    x, y = pipeline(a, 1700, timing=1), pipeline(a, 1700, timing=1)
    for s in (x, y):
        s.update(2, DT)
        s.update(2, DT)          # the chain length's second use: cached from here on
    step_ms, stats = x.last_step_ms(), x.graph_stats()
    energy, profile = x.energy(), x.profile(edges)
    first = x.pair_counts(edges, "all")
    assert x.pair_counts(edges, "all").tobytes() == first.tobytes()
    assert x.energy() == energy and x.profile(edges).tobytes() == profile.tobytes()
    other = x.pair_counts(pr.log_edges(254), "tt")          # another shape of the same table in between
    assert x.pair_counts(edges, "all").tobytes() == first.tobytes() and other.shape == (256, 3)
    assert x.last_step_ms() == step_ms and x.graph_stats() == stats and x.last_diag_ms() > 0.0
    assert x.get_data().tobytes() == y.get_data().tobytes()
    x.update(2, DT)
    y.update(2, DT)
    assert x.get_data().tobytes() == y.get_data().tobytes()          # the trajectory never saw the calls
    assert y.pair_counts(edges, "all").tobytes() == x.pair_counts(edges, "all").tobytes()
    assert y.energy() == x.energy()
    x.close()
    y.close()


def test_nothing_to_count_gives_zeros_and_touches_no_timer():
    for n, m, classes in ((0, 0, "all"), (1, 1, "all"), (300, 0, ("mm", "mt")), (300, 300, ("mt", "tt")), (300, 1, "mm"), (2, 1, ("mm", "tt"))):
        sim = pipeline(pr.world(n, m, seed=8), m)
        rows, lost = sim.pair_counts(pr.log_edges(5), classes, return_unplaced=True)
        assert rows.shape == (7, 3) and not rows.any() and not lost.any() and sim.last_diag_ms() == 0.0, (n, m, classes)
        if n >= 2:
            assert sim.pair_counts(pr.log_edges(5), "all").sum() == n * (n - 1) // 2 and sim.last_diag_ms() > 0.0
        sim.close()
