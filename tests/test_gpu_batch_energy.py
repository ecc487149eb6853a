"""Energy / momentum / potential diagnostics of world ensembles on the GPU (nb_hip_ensemble_energy,
nb_hip_ensemble_potential, GetWorldBatchEnergy / GetWorldBatchPotential).

The contract is bitwise: member b's result is what nb_hip_energy / nb_hip_potential give for a SimPipeline holding the same
particles, whatever B is and whatever the other members hold.  Then: float64 accuracy with tests/test_gpu_energy.py's own
bounds, that the calls change nothing a step, a read-back or a timer can observe, the WorldBatch layer, and the use the
feature is for (a sweep over dt compared by energy drift).  No wall-clock assertions here."""
import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
from energy_ref import assert_energy_close, energy_f64, phi_f64
from gpu_common import synth

pytestmark = pytest.mark.gpu

DT = 0.01


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def members(n, count, seed=0):
    """count worlds of n particles, frac_massive spread over 0 .. 1; from 5 members on M_b = 0, 1 and N are among them."""
    out = []
    for b in range(count):
        frac = 0.5 if count == 1 else b / (count - 1)
        part, m = synth(n, frac_massive=frac, seed=1000 * seed + b)
        if count >= 5 and b == 1:                     # one lone mass among massless receivers
            part, _ = synth(n, frac_massive=0.0, seed=1000 * seed + b)
            part[0, 6], m = 5.0e3, 1
        out.append((part, m))
    if count >= 5:
        ms = [m for _, m in out]
        assert ms[0] == 0 and ms[1] == 1 and ms[-1] == n
    return out


def ensemble(worlds):
    batch = nb.SimBatch(worlds[0][0].shape[0], [m for _, m in worlds])
    batch.set_data(np.stack([p for p, _ in worlds]))
    return batch


def dts_of(count):
    return [DT * (0.5 + 0.01 * b) for b in range(count)]


def alone(state, m):
    """nb_hip_energy / nb_hip_potential of the same particles alone in a SimPipeline on auto."""
    sim = nb.SimPipeline(state.shape[0], m)
    sim.set_data(state)
    e, phi = sim.energy(), sim.potential()
    sim.close()
    return e, phi


@pytest.mark.parametrize("count", [1, 5, 64])
@pytest.mark.parametrize("n", [250, 512, 513, 1000, 2049, 3000])
def test_every_member_is_bitwise_the_single_pipeline(n, count):
    """Both ensemble paths (chain: N <= 512), per = 1 (M <= 2048) and per = 2, ragged tiles and ragged 8-source fetches."""
    worlds = members(n, count, seed=n)
    batch = ensemble(worlds)
    batch.update(7, dts_of(count))
    energies, phis = batch.energy(), batch.potential()
    assert len(energies) == count and phis.shape == (count, n) and phis.dtype == np.float32
    for b, (_, m) in enumerate(worlds):
        state = batch.get_member(b)
        e, phi = alone(state, m)
        assert energies[b] == e, (n, count, b, m)
        assert phis[b].tobytes() == phi.tobytes(), (n, count, b, m)
    batch.close()


@pytest.mark.parametrize("n", [250, 1000, 3000])
def test_two_calls_give_the_same_bits_and_a_member_does_not_depend_on_the_others(n):
    worlds = members(n, 64, seed=n + 1)
    batch = ensemble(worlds)
    batch.update(3, dts_of(64))
    first = (batch.energy(), batch.potential().tobytes())
    assert (batch.energy(), batch.potential().tobytes()) == first
    energies, phis = batch.energy(), batch.potential()
    for b in (0, 1, 17, 40, 63):
        one = nb.SimBatch(n, [worlds[b][1]])
        one.set_data(batch.get_member(b)[None])
        assert one.energy() == [energies[b]], b
        assert one.potential().tobytes() == phis[b].tobytes(), b
        one.close()
    batch.close()


@pytest.mark.parametrize("n", [250, 513, 3000])
def test_members_against_f64(n):
    """tests/test_gpu_energy.py's own bounds: Phi within 1e-5 |Phi|, the sums with assert_energy_close(rel_u=1e-5)."""
    worlds = members(n, 5, seed=n + 2)
    batch = ensemble(worlds)
    batch.update(2, DT)
    energies, phis = batch.energy(), batch.potential()
    for b, (_, m) in enumerate(worlds):
        state = batch.get_member(b)
        want_phi = phi_f64(state, m)
        err = np.abs(phis[b].astype(np.float64) - want_phi)
        assert np.all(err <= 1e-5 * np.abs(want_phi)), (b, float(np.max(err)))
        want, scale = energy_f64(state, m, want_phi)
        assert_energy_close(energies[b], want, scale, rel_u=1e-5)
    assert np.all(phis[0] == 0.0) and energies[0]["mass"] == 0.0 and energies[0]["potential"] == 0.0   # M_b = 0
    assert phis[1][0] == 0.0 and energies[1]["potential"] == 0.0                                       # M_b = 1
    batch.close()


def trajectory(worlds, calls, with_diag):
    batch = ensemble(worlds)
    out = []
    for i, steps in enumerate(calls):
        batch.update(steps, dts_of(len(worlds)) if i % 2 == 0 else DT)
        if with_diag:
            batch.energy()
            batch.potential()
        out.append(batch.get_data())
    batch.close()
    return out


@pytest.mark.parametrize("n", [250, 1000], ids=["chain", "lanes"])
def test_diagnostics_do_not_change_trajectories(n):
    worlds = members(n, 5, seed=n + 3)
    calls = [1, 3, 20, 1, 40]
    plain, diag = trajectory(worlds, calls, False), trajectory(worlds, calls, True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain, diag))


@pytest.mark.parametrize("n", [250, 1000], ids=["chain", "lanes"])
def test_uploads_timers_and_async_steps(n):
    worlds = members(n, 5, seed=n + 4)
    batch = ensemble(worlds)
    assert batch.last_diag_ms() == 0.0
    batch.update(4, dts_of(5))
    uploads, last = batch.dt_uploads(), batch.last_ms()
    batch.energy()
    assert batch.last_diag_ms() > 0.0
    batch.potential()
    assert batch.last_diag_ms() > 0.0
    assert batch.dt_uploads() == uploads and batch.last_ms() == last
    batch.update(1, dts_of(5))                      # the same step sizes: still on the device, no upload
    assert batch.dt_uploads() == uploads
    batch.step_async(5, dts_of(5))
    energies, phis = batch.energy(), batch.potential()   # enqueued behind the steps
    for b, (_, m) in enumerate(worlds):
        e, phi = alone(batch.get_member(b), m)
        assert energies[b] == e and phis[b].tobytes() == phi.tobytes(), b
    batch.close()


def test_world_batch_takes_the_host_path_before_and_the_device_path_after_an_update():
    n, count = 333, 5
    raw = np.stack([p for p, _ in members(n, count, seed=9)])[:, ::-1].copy()      # not partitioned: CreateWorldBatch does it
    wb = nb.WorldBatch(raw)
    start = wb.particles()
    energies, phis = wb.energy(), wb.potential()
    for b in range(count):
        w = nb.World(raw[b])
        assert energies[b] == w.energy() and phis[b].tobytes() == w.potential().tobytes(), b
        w.close()
    ms = [int(np.count_nonzero(start[b, :, 6] > 0)) for b in range(count)]
    wb.update_gpu(dts_of(count), 3)
    energies, phis = wb.energy(), wb.potential()          # the device holds the newest state: computed there
    same = nb.SimBatch(n, ms)                              # the same steps on the same partitioned particles
    same.set_data(start)
    same.update(3, dts_of(count))
    assert energies == same.energy() and phis.tobytes() == same.potential().tobytes()
    for b in range(count):
        assert wb.member(b).tobytes() == same.get_member(b).tobytes(), b   # still the stepped particles
    same.close()
    wb.close()


def test_a_sweep_over_dt_compared_by_energy_drift():
    """Eight copies of the two-body orbit of test_two_body_orbit_conserves_like_the_cpu_steppers, member b stepping by
    DT * 2^-b: each member's energy drift, sampled every 100 steps, is at most 2 x the float64 stepper's at that dt + 1e-6."""
    g = float(np.float32(nb.NB_G))
    mass, d, r = 1000.0, 20.0, 0.25
    v = np.sqrt(g * mass * d / (2.0 * (d * d + r) ** 1.5))
    a = np.zeros((2, 8), dtype=np.float32)
    a[0, 0], a[1, 0], a[0, 3], a[1, 3] = -d / 2, d / 2, -v, v
    a[:, 6], a[:, 7] = mass, r
    part, m = ob.partition(a)
    segments, seg, count = 10, 100, 8
    dts = [DT * 2.0 ** -b for b in range(count)]

    def drift(energies):
        e0 = energies[0]["kinetic"] + energies[0]["potential"]
        return max(abs(x["kinetic"] + x["potential"] - e0) / abs(e0) for x in energies)

    def f64(dt):
        state, es = part, [energy_f64(part, m)[0]]
        for _ in range(segments):
            state = ob.step(state, m, dt, seg, kind="f64")
            es.append(energy_f64(state, m)[0])
        return drift(es)

    batch = ensemble([(part, m)] * count)
    samples = [batch.energy()]
    for _ in range(segments):
        batch.update(seg, dts)
        samples.append(batch.energy())
    batch.close()
    for b in range(count):
        de_gpu, de_f64 = drift([s[b] for s in samples]), f64(dts[b])
        print(f"[batch energy] two-body dt = {dts[b]:.3e}: drift {de_gpu:.3e}, float64 stepper {de_f64:.3e}")
        assert de_gpu <= 2 * de_f64 + 1e-6, (b, de_gpu, de_f64)
