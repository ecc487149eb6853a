"""The one wall-clock assertion of the ensemble feature: members run SIDE BY SIDE.

B = 256 worlds of N = 250.  Device time per world-step of the ensemble (one 10 000-step call) must be at most 1/8 of the
device time per world-step of the same 256 worlds stepped one after another in 256 SimPipelines on auto (1 000-step
calls), both warmed by one call, best of 3, alternating.  The ideal is 1/256 (one workgroup per compute unit, all
concurrent); 1/8 is a floor that only fails when the members do not run concurrently, with a factor 32 left for clocks
and dispatch.  Not a performance target."""
import numpy as np
import pytest

import nbody_amd as nb
from gpu_common import synth

pytestmark = pytest.mark.gpu

B, N, DT = 256, 250, 0.01
ENSEMBLE_STEPS, LOOP_STEPS = 10000, 1000


def test_256_small_worlds_run_side_by_side():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    worlds = [synth(N, frac_massive=0.3 + 0.4 * (b % 7) / 7.0, seed=b) for b in range(B)]
    batch = nb.SimBatch(N, [m for _, m in worlds])
    batch.set_data(np.stack([p for p, _ in worlds]))
    sims = []
    for p, m in worlds:
        s = nb.SimPipeline(N, m)      # auto; the binding turns the step timer on
        s.set_data(p)
        sims.append(s)

    def ensemble_us():
        batch.update(ENSEMBLE_STEPS, DT)
        return batch.last_ms() * 1e3 / (ENSEMBLE_STEPS * B)

    def loop_us():
        total = 0.0
        for s in sims:
            s.update(LOOP_STEPS, DT)
            total += s.last_step_ms()[0]
        return total * 1e3 / (LOOP_STEPS * B)

    ensemble_us(), loop_us()          # warm-up call each
    e, l = [], []
    for _ in range(3):
        e.append(ensemble_us())
        l.append(loop_us())
    batch.close()
    for s in sims:
        s.close()
    ratio = min(e) / min(l)
    print(f"[batch] N={N} B={B}: ensemble {min(e):.4f} us per world-step, one-after-another {min(l):.4f}, ratio 1/{1 / ratio:.1f}")
    assert ratio <= 1.0 / 8.0, (e, l)
