"""The one wall-clock assertion of ragged ensembles: worlds of different sizes run SIDE BY SIDE in one launch.

8 sizes (200, 230, ..., 410) x 32 members, 64 steps.  Device time (the ensembles' own event pairs) of ONE ragged call must
be at most HALF that of the same worlds as eight uniform ensembles stepped one after another in the same process; fastest of
5, alternating.  The eight-launch loop is eight rounds of 32 workgroups on 256 compute units, the ragged call one round of
256: 8x by structure, so the floor of 2 leaves a fourfold margin -- the style of tests/test_gpu_batch_perf.py's 1/8 floor
against an ideal of 1/256.  Not a performance target."""
import numpy as np
import pytest

import nbody_amd as nb
from gpu_common import synth

pytestmark = pytest.mark.gpu

SIZES = [200 + 30 * i for i in range(8)]
PER_SIZE, STEPS, DT = 32, 64, 0.01


def test_eight_sizes_run_in_one_round_not_eight():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    worlds = {n: [synth(n, frac_massive=0.3 + 0.4 * (b % 7) / 7.0, seed=1000 * i + b) for b in range(PER_SIZE)]
              for i, n in enumerate(SIZES)}
    uniform = []
    for n in SIZES:
        u = nb.SimBatch(n, [m for _, m in worlds[n]])
        u.set_data(np.stack([p for p, _ in worlds[n]]))
        uniform.append(u)
    # member order interleaved across the sizes
    order = [(n, b) for b in range(PER_SIZE) for n in SIZES]
    ragged = nb.SimBatch.ragged([n for n, _ in order], [worlds[n][b][1] for n, b in order])
    ragged.set_data([worlds[n][b][0] for n, b in order])
    assert len(ragged.launch_shape()["groups"]) == 1

    def ragged_ms():
        ragged.update(STEPS, DT)
        return ragged.last_ms()

    def loop_ms():
        total = 0.0
        for u in uniform:
            u.update(STEPS, DT)
            total += u.last_ms()
        return total

    ragged_ms(), loop_ms()            # warm-up call each
    r, l = [], []
    for _ in range(5):
        r.append(ragged_ms())
        l.append(loop_ms())
    ragged.close()
    for u in uniform:
        u.close()
    ratio = min(r) / min(l)
    print(f"[ragged] {len(SIZES)} sizes x {PER_SIZE} members, {STEPS} steps: one ragged call {min(r) * 1e3:.1f} us, "
          f"eight uniform ensembles one after another {min(l) * 1e3:.1f} us, ratio {ratio:.3f} (1/{1 / ratio:.1f})")
    assert ratio <= 0.5, (r, l)
