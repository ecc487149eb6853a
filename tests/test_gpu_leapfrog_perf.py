"""Leapfrog steps against the adaptive path with the same launch count per step, on the MI355X (wall clock, one case).  In a
file of its own so that a slow machine leaves the correctness rows of tests/test_gpu_leapfrog.py untouched."""
import time

import pytest

import nbody_amd as nb
from gpu_common import bench_universe

pytestmark = pytest.mark.gpu

N, STEPS, DT, ETA, DT_MAX = 65536, 50, 0.01, 0.1, 0.05


def test_leapfrog_steps_cost_what_adaptive_steps_cost():
    """N = 65 536, 50 steps, best of 5, both sides in this process: update_leapfrog against update_adaptive, the existing path
    with the same launch count per step (one O(N) launch and one force launch).  The bound is 1.15: the margin is for
    run-to-run noise on one box.  Measured: leapfrog 20.339 ms, adaptive 20.209 ms, ratio 1.006; the probe's repeat of it
    (profiles/r16_leapfrog_probe.json, "perf_test_ratio") gave 1.003."""
    _, part, m = bench_universe(N)
    s = nb.SimPipeline(N, m)
    s.set_data(part)
    s.update(2, DT)
    s.update_adaptive(2, ETA, DT_MAX)          # warm both paths
    s.update_leapfrog(2, DT)
    leapfrog, adaptive = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        s.update_leapfrog(STEPS, DT)
        leapfrog.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        s.update_adaptive(STEPS, ETA, DT_MAX)
        adaptive.append(time.perf_counter() - t0)
    s.close()
    ratio = min(leapfrog) / min(adaptive)
    print(f"[leapfrog perf] N={N} {STEPS} steps: leapfrog {min(leapfrog) * 1e3:.3f} ms, adaptive {min(adaptive) * 1e3:.3f} ms, ratio {ratio:.3f}")
    assert ratio <= 1.15, (leapfrog, adaptive)
