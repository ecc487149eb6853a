"""Adaptive steps against the host loop they replace, on the MI355X (wall clock, one case).  In a file of its own so that a slow
machine leaves the correctness rows of tests/test_gpu_adaptive.py untouched."""
import time

import numpy as np
import pytest

import nbody_amd as nb
import timestep_ref as tr
from gpu_common import bench_universe

pytestmark = pytest.mark.gpu

N, STEPS, ETA, DT_MAX = 65536, 20, 0.1, 0.05


def test_adaptive_call_beats_the_host_loop_it_replaces():
    """N = 65 536, 20 steps, fastest of three, both sides in this process: nb_hip_adaptive_steps against the loop of get_data +
    host criterion + update(1, dt).  Only the ratio's side of 1 is asserted; the figures are tools/adaptive_probe.py's to record."""
    _, part, m = bench_universe(N)
    s = nb.SimPipeline(N, m)
    s.set_data(part)
    s.update(2, 0.01)
    s.update_adaptive(2, ETA, DT_MAX)          # warm both paths
    s.update(1, float(tr.timestep(s.get_data(), ETA, DT_MAX)))
    adaptive, loop = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        s.update_adaptive(STEPS, ETA, DT_MAX)
        adaptive.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for _ in range(STEPS):
            s.update(1, float(tr.timestep(s.get_data(), ETA, DT_MAX)))
        loop.append(time.perf_counter() - t0)
    s.close()
    print(f"[adaptive perf] N={N} {STEPS} steps: adaptive {min(adaptive) * 1e3:.3f} ms, host loop {min(loop) * 1e3:.3f} ms, "
          f"ratio {min(adaptive) / min(loop):.3f}")
    assert min(adaptive) < min(loop), (adaptive, loop)
