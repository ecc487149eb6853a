"""Wall clock of a traced ensemble update against what it replaces (B = 256 worlds of N = 250, 2 000 steps).

Two conditions that follow from structure, not targets:
  * the auto trace at every = 10 is no slower than the host loop of update(10) + energy(): the same or fewer launches, and
    R - 1 fewer stream syncs and copies;
  * the fused trace at every = 1 is no slower than the interleaved one: the same arithmetic, and two launches and one
    reload of the chain's state fewer per record.
The numbers of record are tools/batch_trace_probe.py's committed profile; the ratios measured here are printed."""
import time

import numpy as np
import pytest

import nbody_amd as nb
from gpu_common import synth

pytestmark = pytest.mark.gpu

B, N, STEPS, DT = 256, 250, 2000, 0.01


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def host_loop(batch, every):
    rows = [batch.energy()]
    for _ in range(STEPS // every):
        batch.update(every, DT)
        rows.append(batch.energy())
    return rows


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def test_a_traced_call_is_no_slower_than_what_it_replaces():
    worlds = [synth(N, frac_massive=0.25 + 0.5 * (b % 7) / 6, seed=b) for b in range(8)]
    start = np.stack([worlds[b % 8][0] for b in range(B)])
    ms = [worlds[b % 8][1] for b in range(B)]

    def fresh(mode):
        batch = nb.SimBatch(N, ms)
        batch.set_data(start)
        batch.trace_mode(mode)
        batch.trace(20, DT, 1)          # warm: code objects, the row buffer, the diagnostics slab
        batch.energy()
        batch.set_data(start)
        return batch

    auto, forced, loop = fresh(0), fresh(1), fresh(0)
    best = {"loop10": np.inf, "auto10": np.inf, "fused1": np.inf, "inter1": np.inf}
    for _ in range(3):                  # best of three, alternating
        for batch in (auto, forced, loop):
            batch.set_data(start)
        t, want = timed(lambda: host_loop(loop, 10))
        best["loop10"] = min(best["loop10"], t)
        t, rows = timed(lambda: auto.trace(STEPS, DT, 10))
        best["auto10"] = min(best["auto10"], t)
        assert auto.last_trace_info() == {"fused": 1, "launches": 1}
        assert [[nb.energy_row(x) for x in r] for r in rows] == want
        auto.set_data(start)
        t, fused = timed(lambda: auto.trace(STEPS, DT, 1))
        best["fused1"] = min(best["fused1"], t)
        t, inter = timed(lambda: forced.trace(STEPS, DT, 1))
        best["inter1"] = min(best["inter1"], t)
        assert forced.last_trace_info() == {"fused": 0, "launches": STEPS + 2 * (STEPS + 1)}
        assert fused.tobytes() == inter.tobytes()
        assert fused[::10].tobytes() == rows.tobytes()
    for batch in (auto, forced, loop):
        batch.close()
    print(f"[batch trace perf] B = {B}, N = {N}, {STEPS} steps: host loop every 10 {best['loop10'] * 1e3:.2f} ms, "
          f"auto trace every 10 {best['auto10'] * 1e3:.2f} ms (ratio {best['auto10'] / best['loop10']:.3f}); "
          f"fused every 1 {best['fused1'] * 1e3:.2f} ms, interleaved every 1 {best['inter1'] * 1e3:.2f} ms "
          f"(ratio {best['fused1'] / best['inter1']:.3f})")
    assert best["auto10"] <= best["loop10"], best
    assert best["fused1"] <= best["inter1"], best
