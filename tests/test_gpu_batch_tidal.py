"""The tidal tensor of world ensembles on the GPU (nb_hip_ensemble_tidal_at / nb_hip_ensemble_tidal_map;
include/nbody_batch_tidal.h of a WorldBatch whose device holds the newest state).  The oracle is the single world: member b's
values are, bit for bit, what nb.SimPipeline(n, mass_len) holding the same particles gives on either of its kernel shapes
(tests/test_gpu_tidal.py holds that pipeline to float64).  Uniform ensembles on the chain path and on the lane-split path,
ragged ones with a member without a source.  No wall-clock assertions here."""
import numpy as np
import pytest

import nbody_amd as nb
from tidal_ref import pixel_points, ratio_to_bound, t_at_f64, tidal_bound

pytestmark = pytest.mark.gpu

DT = 0.01
SOFT = 0.75
SPLIT, WAVE = 1, 2          # the "tidal_shape" tuning hook of a pipeline


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def world(n, m, seed):
    """n particles, the first m of them massive: partitioned as built"""
    rng = np.random.default_rng(7000 + seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * 1.0e3
    a[:, 2:4] = rng.standard_normal((n, 2))
    a[:, 7] = 0.5 + rng.random(n)
    a[:m, 6] = 10.0 + 990.0 * rng.random(m)
    return a


def points(n, seed):
    return (np.random.default_rng(seed).standard_normal((n, 2)) * 1.2e3).astype(np.float32)


def views(count, width, height):
    """a different view per member; member 0's has negative offsets and a zoom that is no power of two"""
    return [nb.RenderView.make((120.0 - 300.0 * b, -40.0 + 90.0 * b), (-3.5 + 7.0 * b, -11.25 + 6.5 * b), 0.037 * (1 + b), width, height, 1.0)
            for b in range(count)]


def same(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int(np.count_nonzero(got != want)))


N_PROBES = 130          # across a tile edge: a full tile of 128 and two samples of a second one


def check_against_pipelines(batch_like, state, mass_lens, what):
    """every tidal call of a SimBatch or a WorldBatch -- probes with shared and with per-member points, maps under one view and
    under per-member views, 64 x 64 and 37 x 7 -- against a SimPipeline per member on both of its shapes"""
    count = len(state)
    shared, own = points(N_PROBES, seed=31), np.stack([points(N_PROBES, seed=40 + b) for b in range(count)])
    for b in range(count):
        if mass_lens[b] > 0:
            own[b, 5] = state[b][mass_lens[b] - 1, 0:2]          # a point exactly on a source
    maps = [(views(1, 64, 64)[0], None), (None, views(count, 37, 7))]
    got_shared, got_own = batch_like.tidal_at(shared, SOFT), batch_like.tidal_at(own, SOFT)
    assert got_shared.shape == got_own.shape == (count, N_PROBES, 3) and np.all(np.isfinite(got_own))
    got_maps = [batch_like.tidal_map(one if one is not None else each, SOFT) for one, each in maps]
    assert got_maps[0].shape == (count, 64, 64, 3) and got_maps[1].shape == (count, 7, 37, 3)
    for b, (part, m) in enumerate(zip(state, mass_lens)):
        sim = nb.SimPipeline(part.shape[0], int(m))
        sim.set_data(part)
        for shape in (SPLIT, WAVE):
            sim.configure(tidal_shape=shape)
            same(got_shared[b], sim.tidal_at(shared, SOFT), (what, "shared points", b, shape))
            same(got_own[b], sim.tidal_at(own[b], SOFT), (what, "own points", b, shape))
            for got, (one, each) in zip(got_maps, maps):
                same(got[b], sim.tidal_map(one if one is not None else each[b], SOFT), (what, "map", b, shape))
        sim.close()
        if m == 0:
            assert not got_own[b].view(np.uint32).any() and not got_maps[1][b].view(np.uint32).any()          # three +0
    # a map is the probes product at the member's pixel centres
    centres = np.stack([pixel_points(v) for v in maps[1][1]])
    same(got_maps[1].reshape(count, -1, 3), batch_like.tidal_at(centres, SOFT), (what, "map = probes"))
    return got_own, own


# ---- uniform ensembles -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [250, 700])          # the chain path, which never moves `cur`, and the lane-split path, which does
def test_every_member_of_a_uniform_ensemble_has_its_pipelines_bits(n):
    mass_lens = [n // 2, n, 0, 257 if n > 257 else 7]
    parts = [world(n, m, seed=n + b) for b, m in enumerate(mass_lens)]
    batch = nb.SimBatch(n, mass_lens)
    batch.set_data(np.stack(parts))
    check_against_pipelines(batch, parts, mass_lens, f"N = {n} before any step")
    batch.update(1, DT)          # odd: the lane-split members now sit in the other position buffer
    state = batch.get_data()
    assert not np.array_equal(state[:, :, 0:2], np.stack(parts)[:, :, 0:2])
    got, pts = check_against_pipelines(batch, list(state), mass_lens, f"N = {n} after a step")
    assert batch.last_diag_ms() > 0.0
    # one case against float64 guards against an ensemble and its pipelines being wrong together
    t64, mag = t_at_f64(state[1], n, pts[1], SOFT)
    worst = ratio_to_bound(got[1], t64, mag)
    print(f"[batch tidal] N = {n}, member 1: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    batch.close()


# ---- ragged ensembles ------------------------------------------------------------------------------------------------------------

RAGGED_SIZES = [1, 7, 333, 700, 1582, 40]          # the chain group and both lane-split groups
RAGGED_MASS = [1, 7, 300, 513, 1582, 0]            # one member without a source


def test_every_member_of_a_ragged_ensemble_has_its_pipelines_bits():
    parts = [world(n, m, seed=400 + n) for n, m in zip(RAGGED_SIZES, RAGGED_MASS)]
    batch = nb.SimBatch.ragged(RAGGED_SIZES, RAGGED_MASS)
    batch.set_data(parts)
    check_against_pipelines(batch, parts, RAGGED_MASS, "ragged before any step")
    batch.update(3, DT)
    state = batch.get_data()
    assert not np.array_equal(state[4][:, 0:2], parts[4][:, 0:2])
    check_against_pipelines(batch, state, RAGGED_MASS, "ragged after 3 steps")
    batch.close()


# ---- through the WorldBatch --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_a_world_batch_answers_on_the_device_after_gpu_steps_and_on_the_host_before(ragged):
    sizes, mass_lens = (RAGGED_SIZES, RAGGED_MASS) if ragged else ([300] * 3, [150, 300, 1])
    parts = [world(n, m, seed=850 + b) for b, (n, m) in enumerate(zip(sizes, mass_lens))]
    count = len(parts)
    pts, vs = np.stack([points(129, seed=860 + b) for b in range(count)]), views(count, 33, 5)
    make = (lambda: nb.WorldBatch.ragged(parts)) if ragged else (lambda: nb.WorldBatch(np.stack(parts)))
    # never stepped: the host path, and member b is nb.World(member b) bit for bit
    fresh = make()
    host_at, host_map = fresh.tidal_at(pts, SOFT), fresh.tidal_map(vs, SOFT)
    fresh.close()
    for b in range(count):
        w = nb.World(parts[b])
        same(host_at[b], w.tidal_at(pts[b], SOFT), ("host probes", b))
        same(host_map[b], w.tidal_map(vs[b], SOFT), ("host map", b))
        w.close()
    # after GPU steps: the device path, with the bits of the seam holding the same state
    wb = make()
    wb.update_gpu(DT, 2)
    dev_at, dev_map = wb.tidal_at(pts, SOFT), wb.tidal_map(vs, SOFT)
    state = wb.particles()          # reads the device back: from here on the host answers
    state = state if ragged else list(state)
    after_at = wb.tidal_at(pts, SOFT)
    wb.close()
    seam = nb.SimBatch.ragged(sizes, mass_lens) if ragged else nb.SimBatch(sizes[0], mass_lens)
    seam.set_data(state if ragged else np.stack(state))
    same(dev_at, seam.tidal_at(pts, SOFT), "WorldBatch on the device = the seam, probes")
    same(dev_map, seam.tidal_map(vs, SOFT), "WorldBatch on the device = the seam, maps")
    seam.close()
    for b in range(count):
        if mass_lens[b] == 0:
            continue
        t64, mag = t_at_f64(state[b], mass_lens[b], pts[b], SOFT)
        err = np.abs(dev_at[b].astype(np.float64) - after_at[b].astype(np.float64))
        assert np.all(err <= tidal_bound(t64, mag)), (b, float(np.max(err / tidal_bound(t64, mag))))
    assert not np.array_equal(dev_at, after_at)          # two paths: float32 sums against float64 ones


# ---- one launch, and what the calls leave alone -------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 40])
def test_a_call_is_one_timed_launch_for_any_count_and_changes_nothing_a_step_can_observe(count):
    """No launch counter is exposed for the field calls; what is observable is the one event pair around the launch
    (nb_hip_ensemble_last_diag_ms): it covers every member's samples, is cleared by a call that runs nothing, and the call
    leaves the step timer, the step-size uploads and the state alone."""
    n = 250
    parts = [world(n, n - b, seed=900 + b) for b in range(count)]
    mass_lens = [n - b for b in range(count)]
    a, b = nb.SimBatch(n, mass_lens), nb.SimBatch(n, mass_lens)
    for s in (a, b):
        s.set_data(np.stack(parts))
        s.update(1, DT)
    step_ms, uploads = a.last_ms(), a.dt_uploads()
    pts, view = points(N_PROBES, seed=count), views(1, 33, 5)[0]
    first = a.tidal_map(view, SOFT)
    assert a.last_diag_ms() > 0.0
    same(a.tidal_map(view, SOFT), first, "two consecutive maps")
    at = a.tidal_at(pts, SOFT)
    assert at.shape == (count, N_PROBES, 3) and a.last_diag_ms() > 0.0
    assert a.last_ms() == step_ms and a.dt_uploads() == uploads
    assert a.tidal_at(np.zeros((0, 2), dtype=np.float32), SOFT).shape == (count, 0, 3) and a.last_diag_ms() == 0.0
    assert a.get_data().tobytes() == b.get_data().tobytes()
    a.update(1, DT)
    b.update(1, DT)
    assert a.get_data().tobytes() == b.get_data().tobytes()          # step / calls / step == step / step
    # the last member is its own pipeline: nothing in a call depends on how many members there are
    sim = nb.SimPipeline(n, mass_lens[-1])
    sim.set_data(b.get_data()[-1])
    same(a.tidal_at(pts, SOFT)[-1], sim.tidal_at(pts, SOFT), "the last of %d members" % count)
    sim.close()
    a.close()
    b.close()


def test_non_finite_points_give_nan_exactly_there():
    parts = [world(350, 300, seed=300 + b) for b in range(3)]
    batch = nb.SimBatch(350, [300] * 3)
    batch.set_data(np.stack(parts))
    pts = np.stack([points(N_PROBES, seed=800 + b) for b in range(3)])
    clean = batch.tidal_at(pts, SOFT)
    bad = pts.copy()
    hit = np.zeros((3, N_PROBES), dtype=bool)
    for b, i, p in ((0, 1, (np.nan, 0.0)), (1, 64, (0.0, np.inf)), (2, 129, (-np.inf, np.nan)), (2, 0, (np.nan, np.nan))):
        bad[b, i] = p
        hit[b, i] = True
    t = batch.tidal_at(bad, SOFT)
    assert np.array_equal(np.isnan(t), np.repeat(hit[:, :, None], 3, axis=2)) and t[~hit].tobytes() == clean[~hit].tobytes()
    batch.close()
