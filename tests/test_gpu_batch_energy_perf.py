"""The one wall-clock assertion of the ensemble diagnostics: members are processed SIDE BY SIDE.

B = 256 worlds of N = 250 (the worlds of tests/test_gpu_batch_perf.py).  The blocking wall time of ONE SimBatch.energy()
must be at most 1/8 of the summed blocking wall time of the same 256 worlds' SimPipeline.energy() one after another in the
same process; both warmed by one call, best of 3, alternating.  One ensemble call is two launches, a 16 KiB copy and a sync;
the loop is 256 x (two launches, a copy, a sync).  1/8 is the project's side-by-side floor: it only fails when members are
processed serially.  Not a performance target; the measured ratio is printed."""
import time

import numpy as np
import pytest

import nbody_amd as nb
from gpu_common import synth

pytestmark = pytest.mark.gpu

B, N = 256, 250


def test_256_small_worlds_get_their_energy_in_one_call():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")
    worlds = [synth(N, frac_massive=0.3 + 0.4 * (b % 7) / 7.0, seed=b) for b in range(B)]
    batch = nb.SimBatch(N, [m for _, m in worlds])
    batch.set_data(np.stack([p for p, _ in worlds]))
    sims = []
    for p, m in worlds:
        s = nb.SimPipeline(N, m)
        s.set_data(p)
        sims.append(s)

    def ensemble_us():
        t0 = time.perf_counter()
        e = batch.energy()
        return (time.perf_counter() - t0) * 1e6, e

    def loop_us():
        total, e = 0.0, []
        for s in sims:
            t0 = time.perf_counter()
            e.append(s.energy())
            total += time.perf_counter() - t0
        return total * 1e6, e

    ensemble_us(), loop_us()          # warm-up call each
    e, l = [], []
    for _ in range(3):
        t, got = ensemble_us()
        e.append(t)
        t, want = loop_us()
        l.append(t)
        assert got == want            # and they are the same numbers, bit for bit
    device_us = batch.last_diag_ms() * 1e3
    batch.close()
    for s in sims:
        s.close()
    ratio = min(e) / min(l)
    print(f"[batch energy] N={N} B={B}: one ensemble call {min(e):.1f} us wall ({device_us:.1f} us on the device), "
          f"{B} pipelines one after another {min(l):.1f} us, ratio 1/{1 / ratio:.1f}")
    assert ratio <= 1.0 / 8.0, (e, l)
