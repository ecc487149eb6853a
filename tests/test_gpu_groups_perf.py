"""The cost of the groups call against the routes it replaces: blocking wall clock, best of 3 after one warm-up, both sides in one
process.  Both asserts are the structural floors the project uses for a new read-only call, not expected values; the measured
ratios are printed here and recorded by tools/group_probe.py."""
import time

import numpy as np
import pytest

import group_ref as gr
import nbody_amd as nb
from paircount_ref import world

pytestmark = pytest.mark.gpu

REPEATS = 3


def best_of(fn):
    fn()          # warm-up
    best = float("inf")
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def test_the_groups_of_6000_particles_take_no_longer_than_reading_them_back_and_linking_in_numpy():
    """N = 6 000 (the GUI's size), M = N / 2, all particles, a linking length of about the mean separation.  The old route is
    get_data() followed by the numpy model of the same answer; one groups() call must not take longer."""
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    n, m = 6000, 3000
    a = world(n, m, seed=1, spread=3.0)
    length = gr.length_for(n)
    sim = nb.SimPipeline(n, m)
    sim.set_data(a)
    old_route = lambda: gr.model(sim.get_data(), m, gr.ALL, length)
    assert gr.same(sim.groups(length), old_route())
    t_call = best_of(lambda: sim.groups(length))
    device_ms = sim.last_diag_ms()
    t_old = best_of(old_route)
    sim.close()
    ratio = t_old / t_call
    print(f"[group perf] N = 6000, all particles: groups {t_call * 1e3:.3f} ms wall ({device_ms:.3f} ms of kernels), "
          f"get_data + numpy {t_old * 1e3:.1f} ms, ratio {ratio:.0f}")
    assert ratio >= 1.0, (t_call, t_old)


def test_one_ensemble_call_takes_at_most_half_the_time_of_256_pipelines_one_after_another():
    """256 worlds of N = 250: one SimBatch.groups call (three launches, one copy, one sync) against 256 resident SimPipelines
    calling groups one after another.  The factor 2 is the structural floor tests/test_gpu_neighbours_perf.py uses for the same
    comparison, not the expected ratio."""
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    count, n = 256, 250
    length = gr.length_for(n)
    states = [world(n, n // 2, seed=b, spread=3.0) for b in range(count)]
    batch = nb.SimBatch(n, [n // 2] * count)
    batch.set_data(np.stack(states))
    pipes = []
    for a in states:
        pipes.append(nb.SimPipeline(n, n // 2))
        pipes[-1].set_data(a)
    one_call = lambda: batch.groups(length)
    the_loop = lambda: [s.groups(length) for s in pipes]
    assert gr.same(one_call(), np.stack(the_loop()))
    t_batch, t_loop = best_of(one_call), best_of(the_loop)
    batch.close()
    for s in pipes:
        s.close()
    ratio = t_loop / t_batch
    print(f"[group perf] 256 x N = 250: one call {t_batch * 1e3:.3f} ms, 256 pipelines {t_loop * 1e3:.3f} ms, ratio {ratio:.1f}")
    assert ratio >= 2.0, (t_batch, t_loop)
