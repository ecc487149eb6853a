"""The cost of a radial profile against the routes it replaces: blocking wall clock, fastest of 5 after one warm-up, side by
side in one process.  Both asserts are structural floors, not expected values; the measured ratios are printed here and
recorded by tools/profile_probe.py."""
import time

import numpy as np
import pytest

import nbody_amd as nb
import profile_ref as pr

pytestmark = pytest.mark.gpu

REPEATS = 5


def best_of(fn):
    fn()          # warm-up
    best = float("inf")
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def test_a_profile_of_2_to_the_20_particles_takes_no_longer_than_reading_them_back():
    """N = 2^20, 64 logarithmic bins.  The old route starts with get_data(): 32 MiB over PCIe before numpy sees a particle.
    profile() reads the same 32 MB from HBM and returns 3 KB, so it must not take longer than get_data() ALONE."""
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    n = 1 << 20
    a = pr.world(n, n // 2, seed=1)
    sim = nb.SimPipeline(n, n // 2)
    sim.set_data(a)
    edges = nb.profile_edges(0.05, 40.0, 64, log=True)
    rows = sim.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4])
    assert rows[:, 0].sum() == n // 2
    t_profile = best_of(lambda: sim.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4]))
    device_ms = sim.last_diag_ms()
    t_read = best_of(sim.get_data)
    sim.close()
    ratio = t_read / t_profile
    print(f"[profile perf] N = 2^20, 64 bins: profile {t_profile * 1e3:.3f} ms wall ({device_ms:.3f} ms of kernels), get_data alone "
          f"{t_read * 1e3:.3f} ms, ratio {ratio:.2f}")
    assert ratio >= 1.0, (t_profile, t_read)


def test_one_ensemble_profile_takes_at_most_half_the_time_of_256_pipelines_one_after_another():
    """256 worlds of N = 250: one SimBatch.profile call (one upload, one launch, one copy, one sync) against 256 resident
    SimPipelines calling profile one after another.  The factor 2 is the structural floor tests/test_gpu_batch_field_perf.py
    uses for the same comparison, not the expected ratio."""
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    count, n = 256, 250
    states = [pr.world(n, n // 2, seed=b) for b in range(count)]
    edges = nb.profile_edges(0.05, 40.0, 64, log=True)
    batch = nb.SimBatch(n, [n // 2] * count)
    batch.set_data(np.stack(states))
    pipes = []
    for a in states:
        pipes.append(nb.SimPipeline(n, n // 2))
        pipes[-1].set_data(a)
    one_call = lambda: batch.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4])
    the_loop = lambda: [s.profile(edges, pr.CENTRE[0:2], pr.CENTRE[2:4]) for s in pipes]
    assert pr.same(one_call(), np.stack(the_loop()))
    t_batch, t_loop = best_of(one_call), best_of(the_loop)
    batch.close()
    for s in pipes:
        s.close()
    ratio = t_loop / t_batch
    print(f"[profile perf] 256 x N = 250: one call {t_batch * 1e3:.3f} ms, 256 pipelines {t_loop * 1e3:.3f} ms, ratio {ratio:.1f}")
    assert ratio >= 2.0, (t_batch, t_loop)
