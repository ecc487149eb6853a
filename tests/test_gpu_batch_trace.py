"""Traced ensemble updates on the GPU (nb_hip_ensemble_trace / _dts, UpdateWorldBatch_GPU_Traced): n steps with every
member's energy recorded on entry and after every `every`-th step, in one call.

Everything is bitwise.  The rows are what SimBatch.energy() returns after the same steps made by separate update(every)
calls; the trajectory, the step sizes on the device and the upload count are what update(n) leaves.  N <= 512 records
inside the one chain launch (fused), above it the diagnostics launches are interleaved with the step launches; the
`trace_mode` hook forces the interleaved path where both exist, and the two must agree bit for bit."""
import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
from energy_ref import energy_f64
from test_gpu_batch_energy import DT, dts_of, ensemble, members

pytestmark = pytest.mark.gpu

FUSED_N = [130, 250, 512]        # two tiles with a ragged second one; two tiles; four tiles and two source blocks
INTERLEAVED_N = [513, 1000]
CALLS = [(7, 1), (10, 3), (3, 10), (0, 1)]
CHAIN_MAX_STEPS = 65536          # steps one launch of the chain runs (pipeline_internal.h)


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def host_loop(worlds, n, every, dts):
    """The rows a traced call must give, by the loop it replaces: energy(), then update(every) + energy() n // every times,
    then the n % every unrecorded steps.  Returns (rows as dicts [R][count], final particles, dt uploads)."""
    batch = ensemble(worlds)
    rows = [batch.energy()]
    for _ in range(n // every):
        batch.update(every, dts)
        rows.append(batch.energy())
    if n % every:
        batch.update(n % every, dts)
    out = rows, batch.get_data(), batch.dt_uploads()
    batch.close()
    return out


def as_dicts(rows):
    return [[nb.energy_row(rows[r, b]) for b in range(rows.shape[1])] for r in range(rows.shape[0])]


def step_launches(n_particles, n):
    """Launches update(n) makes: one per step on the lane-split path, one per 65 536 steps on the chain path."""
    return n if n_particles > 512 else -(-n // CHAIN_MAX_STEPS)


@pytest.mark.parametrize("n_steps,every", CALLS)
@pytest.mark.parametrize("n", FUSED_N + INTERLEAVED_N)
def test_rows_are_the_separate_calls_and_the_trajectory_is_the_untraced_update(n, n_steps, every):
    count = 5
    worlds = members(n, count, seed=n)
    dts = dts_of(count)
    want_rows, _, _ = host_loop(worlds, n_steps, every, dts)
    plain = ensemble(worlds)
    plain.update(n_steps, dts)

    batch = ensemble(worlds)
    rows = batch.trace(n_steps, dts, every)
    records = 1 + n_steps // every
    assert rows.shape == (records, count, 8) and rows.dtype == np.float64
    got = as_dicts(rows)
    for r in range(records):
        for b in range(count):
            assert got[r][b] == want_rows[r][b], (r, b, got[r][b], want_rows[r][b])
    assert batch.get_data().tobytes() == plain.get_data().tobytes()
    assert batch.dt_uploads() == plain.dt_uploads()
    info = batch.last_trace_info()
    if n <= 512:
        assert info == {"fused": 1, "launches": 1}, info
    else:
        assert info == {"fused": 0, "launches": step_launches(n, n_steps) + 2 * records}, info
    # the step sizes on the device are the untraced call's: the next call with the same ones uploads nothing, and ends
    # on the same bits
    if n_steps:
        before = batch.dt_uploads()
        batch.update(2, dts)
        plain.update(2, dts)
        assert batch.dt_uploads() == before and batch.get_data().tobytes() == plain.get_data().tobytes()
    # M_b = 0: every sum is zero; the lone mass of member 1 has no potential
    assert all(v == 0.0 for v in rows[:, 0].ravel())
    assert all(x == 0.0 for x in rows[:, 1, 1])
    plain.close()
    batch.close()


@pytest.mark.parametrize("n", FUSED_N)
def test_fused_and_interleaved_give_the_same_bits(n):
    count = 5
    worlds = members(n, count, seed=n + 1)
    out = []
    for mode in (0, 1):
        batch = ensemble(worlds)
        batch.trace_mode(mode)
        rows = batch.trace(11, dts_of(count), 2)
        info = batch.last_trace_info()
        assert info["fused"] == 1 - mode
        assert info["launches"] == (1 if mode == 0 else 6 + 2 * 6), info   # five update(2) and one update(1), six records
        out.append((rows, batch.get_data(), batch.last_ms()))
        batch.close()
    assert out[0][0].tobytes() == out[1][0].tobytes()
    assert out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2] > 0.0 and out[1][2] > 0.0          # the update's timer brackets the traced call


def test_uniform_dt_and_the_timer_and_the_diagnostics_timer():
    worlds = members(250, 5, seed=77)
    batch = ensemble(worlds)
    assert batch.last_ms() == 0.0
    rows = batch.trace(6, DT, 2)
    assert batch.last_ms() > 0.0 and batch.last_diag_ms() == 0.0      # the diagnostics' own event pair is not touched
    assert batch.dt_uploads() == 1
    want, final, uploads = host_loop(worlds, 6, 2, DT)
    assert as_dicts(rows) == want and batch.get_data().tobytes() == final.tobytes() and uploads == 1
    batch.close()


@pytest.mark.parametrize("n", [250, 1000], ids=["fused", "interleaved"])
def test_a_member_does_not_depend_on_the_ensemble(n):
    worlds = members(n, 5, seed=n + 2)
    dts = dts_of(5)
    batch = ensemble(worlds)
    rows = batch.trace(9, dts, 4)
    state = batch.get_member(2)
    batch.close()
    single = ensemble([worlds[2]])
    alone = single.trace(9, [dts[2]], 4)
    assert alone.shape == (3, 1, 8)
    assert alone[:, 0].tobytes() == rows[:, 2].tobytes()
    assert single.get_member(0).tobytes() == state.tobytes()
    single.close()


def test_record_indices_carry_across_a_launch_split():
    """65 540 steps are two chain launches (65 536 + 4); with a record every 16 385 steps row 4 = the final state is
    recorded by the second one."""
    n, n_steps, every = 64, 65540, 16385
    worlds = [members(n, 5, seed=5)[b] for b in (2, 3, 4)]
    dts = [1.0e-4, 2.0e-4, 3.0e-4]
    batch = ensemble(worlds)
    rows = batch.trace(n_steps, dts, every)
    assert rows.shape == (5, 3, 8)
    assert batch.last_trace_info() == {"fused": 1, "launches": 2}
    other = ensemble(worlds)
    want = [other.energy()]
    for _ in range(4):
        other.update(every, dts)
        want.append(other.energy())
    assert as_dicts(rows) == want
    assert batch.get_data().tobytes() == other.get_data().tobytes()          # n % every == 0: the same steps
    other.close()
    batch.close()


@pytest.mark.parametrize("n", [250, 1000], ids=["fused", "interleaved"])
def test_the_row_buffer_grows_and_is_reused(n):
    worlds = members(n, 5, seed=n + 6)
    dts = dts_of(5)
    batch = ensemble(worlds)
    first = batch.trace(4, dts, 2)           # 3 records
    second = batch.trace(12, dts, 1)         # 13: the buffer is regrown
    third = batch.trace(3, dts, 3)           # 2: and reused
    other = ensemble(worlds)
    want = [other.energy()]
    for k in [2, 2] + [1] * 12 + [3]:
        other.update(k, dts)
        want.append(other.energy())
    assert as_dicts(first) == want[0:3]
    assert as_dicts(second) == want[2:15]
    assert as_dicts(third) == want[14:16]
    assert batch.get_data().tobytes() == other.get_data().tobytes()
    other.close()
    batch.close()


@pytest.mark.parametrize("n", [250, 1000], ids=["fused", "interleaved"])
def test_a_traced_call_queues_behind_async_steps(n):
    worlds = members(n, 5, seed=n + 7)
    dts = dts_of(5)
    batch = ensemble(worlds)
    batch.step_async(5, dts)
    rows = batch.trace(4, dts, 2)            # row 0 is the state behind the five queued steps
    other = ensemble(worlds)
    other.update(5, dts)
    want = [other.energy()]
    for _ in range(2):
        other.update(2, dts)
        want.append(other.energy())
    assert as_dicts(rows) == want
    assert batch.get_data().tobytes() == other.get_data().tobytes()
    other.close()
    batch.close()


@pytest.mark.parametrize("n", [333, 600], ids=["fused", "interleaved"])
def test_world_batch_first_call_on_unpartitioned_input(n):
    count = 5
    raw = np.stack([p for p, _ in members(n, count, seed=9)])[:, ::-1].copy()      # not partitioned: CreateWorldBatch does it
    dts = dts_of(count)
    wb = nb.WorldBatch(raw)
    start = wb.particles()
    ms = [int(np.count_nonzero(start[b, :, 6] > 0)) for b in range(count)]
    rows = wb.update_gpu_traced(dts, 6, 3)           # the first call: the array is still on the host
    same = nb.SimBatch(n, ms)
    same.set_data(start)
    want = same.trace(6, dts, 3)
    assert rows.shape == (3, count, 8) and rows.tobytes() == want.tobytes()
    # n % every == 0: the last row is the state (asked before a read refreshes the host array: then the host computes)
    assert wb.energy() == as_dicts(rows)[-1]
    for b in range(count):
        assert wb.member(b).tobytes() == same.get_member(b).tobytes(), b      # the stepped particles
    # a traced call of no steps: one row, the device's value, and nothing moves
    again = wb.update_gpu_traced(0.5, 0, 1)
    assert again.shape == (1, count, 8) and again[0].tobytes() == rows[-1].tobytes()
    assert wb.particles().tobytes() == same.get_data().tobytes()
    # uniform dt
    more = wb.update_gpu_traced(DT, 2, 1)
    assert more.tobytes() == same.trace(2, DT, 1).tobytes()
    same.close()
    wb.close()


def test_a_world_batch_that_never_stepped_records_the_devices_row_zero():
    """n = 0 as the FIRST call: the array is uploaded, row 0 is the device's value (the bits of a SimBatch holding the
    partitioned particles), and the host array stays the newest state."""
    raw = np.stack([p for p, _ in members(200, 5, seed=10)])[:, ::-1].copy()
    wb = nb.WorldBatch(raw)
    start = wb.particles()
    row0 = wb.update_gpu_traced(DT, 0, 4)
    same = nb.SimBatch(200, [int(np.count_nonzero(start[b, :, 6] > 0)) for b in range(5)])
    same.set_data(start)
    assert as_dicts(row0)[0] == same.energy()
    assert wb.particles().tobytes() == start.tobytes()
    same.close()
    wb.close()


def test_a_sweep_over_dt_through_one_traced_call():
    """The two-body sweep of test_a_sweep_over_dt_compared_by_energy_drift (tests/test_gpu_batch_energy.py) with its ten
    host round trips replaced by ONE traced call (n = 1000, every = 100); the bound is that test's."""
    g = float(np.float32(nb.NB_G))
    mass, d, r = 1000.0, 20.0, 0.25
    v = np.sqrt(g * mass * d / (2.0 * (d * d + r) ** 1.5))
    a = np.zeros((2, 8), dtype=np.float32)
    a[0, 0], a[1, 0], a[0, 3], a[1, 3] = -d / 2, d / 2, -v, v
    a[:, 6], a[:, 7] = mass, r
    part, m = ob.partition(a)
    segments, seg, count = 10, 100, 8
    dts = [DT * 2.0 ** -b for b in range(count)]

    def drift(totals):
        return max(abs(x - totals[0]) / abs(totals[0]) for x in totals)

    def f64(dt):
        state, es = part, [energy_f64(part, m)[0]]
        for _ in range(segments):
            state = ob.step(state, m, dt, seg, kind="f64")
            es.append(energy_f64(state, m)[0])
        return drift([e["kinetic"] + e["potential"] for e in es])

    batch = ensemble([(part, m)] * count)
    rows = batch.trace(segments * seg, dts, seg)
    assert batch.last_trace_info() == {"fused": 1, "launches": 1}
    batch.close()
    assert rows.shape == (segments + 1, count, 8)
    for b in range(count):
        de_gpu, de_f64 = drift([rows[r, b, 0] + rows[r, b, 1] for r in range(segments + 1)]), f64(dts[b])
        print(f"[batch trace] two-body dt = {dts[b]:.3e}: drift {de_gpu:.3e}, float64 stepper {de_f64:.3e}")
        assert de_gpu <= 2 * de_f64 + 1e-6, (b, de_gpu, de_f64)
