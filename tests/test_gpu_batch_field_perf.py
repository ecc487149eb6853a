"""One SimBatch.potential_map call against the loop it replaces, wall clock, side by side in one process."""
import time

import numpy as np
import pytest

import nbody_amd as nb
import render_ref as rr
from gpu_common import synth

pytestmark = pytest.mark.gpu

COUNT, N, SIZE = 256, 250, 64
SOFT = 0.75
FLOOR = 2.0          # structural: 256 uploads, launches, copies and syncs against one of each; not the expected value


def test_one_ensemble_potential_map_takes_at_most_half_the_time_of_256_pipelines_one_after_another():
    """B = 256 worlds of N = 250, a 64 x 64 Phi map each, one warm-up of either side, then the fastest of 5 alternating
    runs: one SimBatch.potential_map call (one upload, one launch, one copy, one sync) must take at most half the wall time
    of 256 resident SimPipelines each calling potential_map on the same views -- the route that existed before the ensemble
    call did.  Both move the same bytes over PCIe.  The factor 2 is a floor that follows from the structure alone, not the
    expected ratio; the measured one is printed here (41.6 on an MI355X: 0.260 ms against 10.81 ms) and recorded by
    tools/batch_field_probe.py (profiles/r22_batch_field_probe.json, the 64 x 64 row: 45.4, 0.243 ms against 11.04 ms), in
    README.md and in STATUS.md."""
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    made = [synth(N, 0.5, seed=b) for b in range(COUNT)]
    views = [rr.fit_view(p, SIZE, SIZE) for p, _ in made]
    batch = nb.SimBatch(N, [m for _, m in made])
    batch.set_data(np.stack([p for p, _ in made]))
    pipes = []
    for p, m in made:
        pipes.append(nb.SimPipeline(N, m))
        pipes[-1].set_data(p)

    def one_call():
        return batch.potential_map(views, SOFT)

    def the_loop():
        return [s.potential_map(v, SOFT) for s, v in zip(pipes, views)]

    maps, alone = one_call(), the_loop()          # warm-up
    t_batch = t_loop = float("inf")
    for _ in range(5):
        t0 = time.perf_counter()
        maps = one_call()
        t1 = time.perf_counter()
        alone = the_loop()
        t2 = time.perf_counter()
        t_batch, t_loop = min(t_batch, t1 - t0), min(t_loop, t2 - t1)
    assert np.array_equal(maps, np.stack(alone))
    ratio = t_loop / t_batch
    print(f"[batch field] one call {t_batch * 1e3:.3f} ms, {COUNT} pipelines {t_loop * 1e3:.3f} ms, ratio {ratio:.1f}")
    assert ratio >= FLOOR, (t_batch, t_loop)
    batch.close()
    for s in pipes:
        s.close()
