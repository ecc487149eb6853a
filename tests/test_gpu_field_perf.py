"""The cost of the field kernel per pair against the kernel it restates (one assertion, device time only).

potential_map at 256 x 128 over a resident world of M = N = 4 096 does the 32 768 x 4 096 pairs that nb_hip_potential does
for the same 32 768 probes appended as massless particles (plus that pipeline's own 4 096 receivers, which only makes the
yardstick's job larger), with cheaper receiver loads: it must not cost more.  Both sides are measured in one process by
nb_hip_last_diag_ms, five repeats each, alternating; the allowance is the yardstick's own relative spread in that run,
(max - min) / min of its five repeats, not a constant chosen in advance."""
import numpy as np
import pytest

import nbody_amd as nb
import render_ref as rr
from field_ref import augmented, pixel_points
from gpu_common import synth

pytestmark = pytest.mark.gpu

SOFT = 0.75
REPEATS = 5


def test_the_map_costs_no_more_per_pair_than_nb_hip_potential():
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
    aug.set_data(both)
    img, want = sim.potential_map(view, SOFT), aug.potential()          # warm-up of both, and the same bits
    assert img.reshape(-1).tobytes() == want[4096:].tobytes()
    t_map, t_ref = [], []
    for _ in range(REPEATS):
        sim.potential_map(view, SOFT)
        t_map.append(sim.last_diag_ms())
        aug.potential()
        t_ref.append(aug.last_diag_ms())
    sim.close()
    aug.close()
    best_map, best_ref = min(t_map), min(t_ref)
    margin = (max(t_ref) - min(t_ref)) / min(t_ref)
    print(f"[field perf] map {best_map:.4f} ms (all {[round(t, 4) for t in t_map]}), potential() of the augmented pipeline "
          f"{best_ref:.4f} ms (all {[round(t, 4) for t in t_ref]}), ratio {best_map / best_ref:.4f}, allowance {margin:.4f}")
    assert best_map <= best_ref * (1.0 + margin), (best_map, best_ref, margin)
