"""The cost of the tidal kernel against the route it replaces (one assertion, device time only).

Before nb_hip_tidal_map a caller took central differences of g: acceleration_at of the four offset points p +- h e_x,
p +- h e_y per sample.  tidal_map at 256 x 128 over a resident world of M = N = 4 096 must cost no more than that ONE
acceleration_at call of the 4 * 32 768 points.  Both are measured by nb_hip_last_diag_ms in one process, five repeats each,
alternating; the allowance is the yardstick's own relative spread in that run, (max - min) / min of its five repeats, not a
constant chosen in advance (tests/test_gpu_gravity_perf.py's rule).  The ratio to a single acceleration_map of the same view
is printed for the record, not asserted."""
import numpy as np
import pytest

import nbody_amd as nb
import render_ref as rr
from gpu_common import synth
from tidal_ref import pixel_points

pytestmark = pytest.mark.gpu

SOFT = 0.75
REPEATS = 5


def test_the_map_costs_no_more_than_the_central_differences_it_replaces():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    part, _ = synth(4096, frac_massive=1.1, seed=12)          # every particle massive: M = N = 4 096
    m = int(np.count_nonzero(part[:, 6] > 0))
    assert m == part.shape[0] == 4096
    view = rr.fit_view(part, 256, 128)
    pts = pixel_points(view)
    h = np.float32(2.0 ** -4)          # what a float32 caller can afford: the step must survive the rounding of p + h
    offsets = np.array([[h, 0], [-h, 0], [0, h], [0, -h]], dtype=np.float32)
    fd_pts = np.ascontiguousarray((pts[:, None, :] + offsets[None, :, :]).reshape(-1, 2))
    assert fd_pts.shape == (4 * 32768, 2)
    sim = nb.SimPipeline(4096, m)
    sim.set_data(part)
    img = sim.tidal_map(view, SOFT)          # warm-up of all three
    sim.acceleration_at(fd_pts, SOFT)
    sim.acceleration_map(view, SOFT)
    assert img.shape == (128, 256, 3) and np.all(np.isfinite(img))
    t_map, t_ref, t_g = [], [], []
    for _ in range(REPEATS):
        sim.tidal_map(view, SOFT)
        t_map.append(sim.last_diag_ms())
        sim.acceleration_at(fd_pts, SOFT)
        t_ref.append(sim.last_diag_ms())
        sim.acceleration_map(view, SOFT)
        t_g.append(sim.last_diag_ms())
    sim.close()
    best_map, best_ref = min(t_map), min(t_ref)
    margin = (max(t_ref) - min(t_ref)) / min(t_ref)
    print(f"[tidal perf] map {best_map:.4f} ms (all {[round(t, 4) for t in t_map]}), acceleration_at of the 4 x 32 768 offset points "
          f"{best_ref:.4f} ms (all {[round(t, 4) for t in t_ref]}), ratio {best_map / best_ref:.4f}, allowance {margin:.4f}; "
          f"over one acceleration_map ({min(t_g):.4f} ms): {best_map / min(t_g):.4f} (recorded, not asserted)")
    assert best_map <= best_ref * (1.0 + margin), (best_map, best_ref, margin)
