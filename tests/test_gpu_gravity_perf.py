"""The cost of the gravity kernel against the route that existed before it (one assertion, device time only).

acceleration_map at 256 x 128 over a resident world of M = N = 4 096 does the 32 768 x 4 096 pairs that one dt = 0 step of
the augmented pipeline (the same 32 768 probes appended as massless particles of radius s, plus that pipeline's own 4 096
receivers) does with the same pair statement: 8/9 of the yardstick's pairs, so it must not cost more.  The map is measured
by nb_hip_last_diag_ms, the step by nb_hip_last_step_ms, in one process, five repeats each, alternating; the allowance is the
yardstick's own relative spread in that run, (max - min) / min of its five repeats, not a constant chosen in advance."""
import numpy as np
import pytest

import nbody_amd as nb
import render_ref as rr
from gpu_common import acc_bound, synth
from gravity_ref import augmented, g_at_f64, pixel_points

pytestmark = pytest.mark.gpu

SOFT = 0.75
REPEATS = 5


def test_the_map_costs_no_more_than_a_step_of_the_augmented_pipeline():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    part, _ = synth(4096, frac_massive=1.1, seed=12)          # every particle massive: M = N = 4 096
    m = int(np.count_nonzero(part[:, 6] > 0))
    assert m == part.shape[0] == 4096
    view = rr.fit_view(part, 256, 128)
    pts = pixel_points(view)
    sim = nb.SimPipeline(4096, m)
    sim.set_data(part)
    both = augmented(part, pts, SOFT)
    aug = nb.SimPipeline(both.shape[0], m)
    aug.configure(timing=1)
    aug.set_data(both)
    img = sim.acceleration_map(view, SOFT)          # warm-up of both, and the two sides agree
    aug.update(1, 0.0)
    step = aug.get_data()[4096:, 4:6]
    g64, mag = g_at_f64(part, m, pts, SOFT)
    bound = acc_bound(g64, mag)
    diff = np.abs(img.reshape(-1, 2).astype(np.float64) - step.astype(np.float64))
    assert np.all(diff <= 2.0 * bound), float(np.max(diff / bound))
    t_map, t_ref = [], []
    for _ in range(REPEATS):
        sim.acceleration_map(view, SOFT)
        t_map.append(sim.last_diag_ms())
        aug.update(1, 0.0)
        t_ref.append(aug.last_step_ms()[0])
    sim.close()
    aug.close()
    best_map, best_ref = min(t_map), min(t_ref)
    margin = (max(t_ref) - min(t_ref)) / min(t_ref)
    print(f"[gravity perf] map {best_map:.4f} ms (all {[round(t, 4) for t in t_map]}), dt = 0 step of the augmented pipeline "
          f"{best_ref:.4f} ms (all {[round(t, 4) for t in t_ref]}), ratio {best_map / best_ref:.4f}, allowance {margin:.4f}")
    assert best_map <= best_ref * (1.0 + margin), (best_map, best_ref, margin)
