"""The potential and the acceleration field of world ensembles on the GPU (nb_hip_ensemble_potential_at / _potential_map /
_acceleration_at / _acceleration_map; include/nbody_batch_field.h of a WorldBatch whose device holds the newest state).  The
oracle is the single world: member b's values are, bit for bit, what nb.SimPipeline(n, mass_len) holding the same particles
gives, on either of its kernel shapes; one case against float64 guards against both being wrong together.  No wall-clock
assertions here (tests/test_gpu_batch_field_perf.py)."""
import numpy as np
import pytest

import nbody_amd as nb
from field_ref import phi_at_f64, pixel_points
from gpu_common import acc_bound
from gravity_ref import g_at_f64
from test_gpu_lifecycle import returns_what_it_took

pytestmark = pytest.mark.gpu

DT = 0.01
SOFT = 0.75
SPLIT, WAVE = 1, 2          # the "field_shape" / "gravity_shape" tuning hooks of a pipeline
CALLS = ("potential_at", "acceleration_at", "potential_map", "acceleration_map")


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


def uniform(parts, mass_lens):
    batch = nb.SimBatch(parts[0].shape[0], mass_lens)
    batch.set_data(np.stack(parts))
    return batch


def alone(part, m, pts=None, view=None, **knobs):
    """what a SimPipeline holding the same particles gives: (Phi, g) at pts, or the two maps under view"""
    sim = nb.SimPipeline(part.shape[0], m)
    sim.configure(**knobs)
    sim.set_data(part)
    out = (sim.potential_at(pts, SOFT), sim.acceleration_at(pts, SOFT)) if view is None else \
          (sim.potential_map(view, SOFT), sim.acceleration_map(view, SOFT))
    sim.close()
    return out


def same(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, int(np.count_nonzero(got != want)))


def check_members_at(batch, parts, mass_lens, pts, **knobs):
    """every member's probes against its pipeline; pts: (B, n, 2)"""
    phi, g = batch.potential_at(pts, SOFT), batch.acceleration_at(pts, SOFT)
    assert phi.shape == pts.shape[:2] and g.shape == pts.shape
    for b, (part, m) in enumerate(zip(parts, mass_lens)):
        want_phi, want_g = alone(part, int(m), pts=pts[b], **knobs)
        same(phi[b], want_phi, ("phi", b, int(m), knobs))
        same(g[b], want_g, ("g", b, int(m), knobs))
    return phi, g


def check_members_map(batch, parts, mass_lens, vs):
    phi, g = batch.potential_map(vs, SOFT), batch.acceleration_map(vs, SOFT)
    for b, (part, m) in enumerate(zip(parts, mass_lens)):
        want_phi, want_g = alone(part, int(m), view=vs[b])
        same(phi[b], want_phi, ("phi map", b, int(m)))
        same(g[b], want_g, ("g map", b, int(m)))
    return phi, g


# ---- the edges of the source walk ------------------------------------------------------------------------------------------

# nothing; the single-source tail alone; the 8-wide fetch with and without a tail; a block edge; one block per slice (2 048 =
# 8 blocks) and two in the first (9); 12 blocks, where slices 6 and 7 are empty
SOURCES = [0, 1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 3000]


@pytest.mark.parametrize("m", SOURCES)
def test_every_member_has_its_pipelines_bits_at_every_edge_of_the_source_walk(m):
    n = min(max(m, 1) + 5, 3000)
    parts = [world(n, m, seed=10 * m + b) for b in range(3)]
    pts = np.stack([points(129, seed=m + b) for b in range(3)])
    if m > 0:
        for b in range(3):
            pts[b, 5] = parts[b][m - 1, 0:2]          # a point exactly on a source: a finite value, a zero term in g
    batch = uniform(parts, [m] * 3)
    phi, g = check_members_at(batch, parts, [m] * 3, pts, field_shape=SPLIT, gravity_shape=SPLIT)
    check_members_at(batch, parts, [m] * 3, pts, field_shape=WAVE, gravity_shape=WAVE)
    batch.close()
    assert np.all(np.isfinite(phi)) and np.all(np.isfinite(g))
    if m == 0:
        assert np.all(phi == 0.0) and np.all(g == 0.0)
    else:
        assert np.all(phi < 0.0)


# ---- the edges of the sample tiles -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def three_of_300():
    parts = [world(350, 300, seed=300 + b) for b in range(3)]
    batch = uniform(parts, [300] * 3)
    yield batch, parts
    batch.close()


@pytest.mark.parametrize("n", [1, 127, 128, 129, 513])          # tail lanes, a second wave, a second workgroup
def test_probe_counts_at_the_tile_edges(three_of_300, n):
    batch, parts = three_of_300
    check_members_at(batch, parts, [300] * 3, np.stack([points(n, seed=n + b) for b in range(3)]))


@pytest.mark.parametrize("width,height", [(33, 5), (64, 3)])
def test_a_map_is_its_pipelines_map_and_the_probes_product_at_the_pixel_centres(three_of_300, width, height):
    batch, parts = three_of_300
    vs = views(3, width, height)
    phi, g = check_members_map(batch, parts, [300] * 3, vs)
    assert phi.shape == (3, height, width) and g.shape == (3, height, width, 2)
    centres = np.stack([pixel_points(v) for v in vs])
    same(phi.reshape(3, -1), batch.potential_at(centres, SOFT), "phi map = probes")
    same(g.reshape(3, -1, 2), batch.acceleration_at(centres, SOFT), "g map = probes")
    # one view for all members is that view given to each
    same(batch.potential_map(vs[0], SOFT), batch.potential_map([vs[0]] * 3, SOFT), "one view for all")
    same(batch.potential_map(vs[0], SOFT)[1], alone(parts[1], 300, view=vs[0])[0], "one view for all, member 1")


# ---- members that differ, and members that do not matter ------------------------------------------------------------------------

MIXED = [120, 0, 300, 7, 257]


def test_members_of_different_mass_len_with_their_own_points():
    parts = [world(300, m, seed=50 + b) for b, m in enumerate(MIXED)]
    batch = uniform(parts, MIXED)
    phi, g = check_members_at(batch, parts, MIXED, np.stack([points(130, seed=60 + b) for b in range(5)]))
    check_members_map(batch, parts, MIXED, views(5, 17, 9))
    batch.close()
    assert np.all(phi[1] == 0.0) and np.all(g[1] == 0.0) and np.all(phi[[0, 2, 3, 4]] < 0.0)


def test_a_members_values_depend_on_nothing_but_its_own_particles_and_points():
    mine, m, pts, view = world(300, 257, seed=77), 257, points(200, seed=78), views(1, 21, 6)[0]

    def member_in(parts, mass_lens, at):
        batch = uniform(parts, mass_lens)
        every = np.stack([points(200, seed=900 + b) for b in range(len(parts))])
        every[at] = pts
        out = (batch.potential_at(every, SOFT)[at], batch.acceleration_at(every, SOFT)[at],
               batch.potential_map(view, SOFT)[at], batch.acceleration_map(view, SOFT)[at])
        batch.close()
        return out

    first = member_in([world(300, k, seed=80 + b) for b, k in enumerate(MIXED[:2])] + [mine] + [world(300, 9, seed=83), world(300, 300, seed=84)],
                      MIXED[:2] + [m, 9, 300], 2)
    others = member_in([world(300, 300, seed=90), world(300, 1, seed=91), mine, world(300, 0, seed=93), world(300, 40, seed=94)],
                       [300, 1, m, 0, 40], 2)
    moved = member_in([world(300, 11, seed=95)] * 4 + [mine], [11] * 4 + [m], 4)
    pair = member_in([mine, world(300, 300, seed=96)], [m, 300], 0)
    single = member_in([mine], [m], 0)
    for name, got in (("other neighbours", others), ("another index", moved), ("B = 2", pair), ("B = 1", single)):
        for call, x, y in zip(CALLS, got, first):
            same(x, y, (name, call))


# ---- ragged ensembles ------------------------------------------------------------------------------------------------------------

RAGGED_SIZES = [1, 129, 513, 3000]          # the chain group and both lane-split groups
RAGGED_MASS = [1, 60, 513, 1467]


def four_calls(batch_like, count):
    """the four calls of a SimBatch or a WorldBatch with per-member points and views: (results, points, views)"""
    pts, vs = np.stack([points(130, seed=40 + b) for b in range(count)]), views(count, 33, 5)
    got = (batch_like.potential_at(pts, SOFT), batch_like.acceleration_at(pts, SOFT),
           batch_like.potential_map(vs, SOFT), batch_like.acceleration_map(vs, SOFT))
    return got, pts, vs


def compare_ragged(got, pts, vs, state, mass_lens, what):
    for b, (part, m) in enumerate(zip(state, mass_lens)):
        want = alone(part, int(m), pts=pts[b]) + alone(part, int(m), view=vs[b])
        for call, g, x in zip(CALLS, got, want):
            same(g[b], x, (what, call, b))


def test_ragged_members_before_any_step_and_after_an_odd_number_of_steps():
    parts = [world(n, m, seed=400 + n) for n, m in zip(RAGGED_SIZES, RAGGED_MASS)]
    batch = nb.SimBatch.ragged(RAGGED_SIZES, RAGGED_MASS)
    batch.set_data(parts)
    got, pts, vs = four_calls(batch, len(parts))
    compare_ragged(got, pts, vs, parts, RAGGED_MASS, "before any step")
    batch.update(3, DT)          # odd: the lane-split members now sit in the other position buffer
    got, pts, vs = four_calls(batch, len(parts))
    state = batch.get_data()
    assert not np.array_equal(state[3][:, 0:2], parts[3][:, 0:2])
    compare_ragged(got, pts, vs, state, RAGGED_MASS, "after 3 steps")
    batch.close()


def test_a_ragged_world_batch_after_steps_answers_on_the_device_with_each_members_bits():
    parts = [world(n, m, seed=500 + n) for n, m in zip(RAGGED_SIZES, RAGGED_MASS)]
    wb = nb.WorldBatch.ragged(parts)
    wb.update_gpu(DT, 3)
    got, pts, vs = four_calls(wb, len(parts))
    state = wb.particles()          # reads the device back: from here on the host would answer
    wb.close()
    compare_ragged(got, pts, vs, state, RAGGED_MASS, "WorldBatch.ragged after 3 steps")


# ---- after steps on a uniform ensemble ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [250, 600])          # the chain path, which never moves `cur`, and the lane-split path, which does
def test_after_one_and_two_steps_the_latest_state_is_what_is_sampled(n):
    mass_lens = [n // 2, n, n // 3]
    parts = [world(n, m, seed=n + b) for b, m in enumerate(mass_lens)]
    batch = uniform(parts, mass_lens)
    pts, vs = np.stack([points(130, seed=n + 10 + b) for b in range(3)]), views(3, 33, 5)
    for _ in range(2):          # after 1 step, after 2 steps
        batch.update(1, DT)
        state = batch.get_data()
        assert not np.array_equal(state[:, :, 0:2], np.stack(parts)[:, :, 0:2])
        check_members_at(batch, list(state), mass_lens, pts)
        check_members_map(batch, list(state), mass_lens, vs)
    batch.close()


# ---- float64 ---------------------------------------------------------------------------------------------------------------------

def test_probes_against_float64(three_of_300):
    """the tolerances tests/test_gpu_field.py and tests/test_gpu_gravity.py hold the single world to"""
    batch, parts = three_of_300
    pts = np.stack([points(129, seed=600 + b) for b in range(3)])
    phi, g = batch.potential_at(pts, SOFT), batch.acceleration_at(pts, SOFT)
    for b in range(3):
        want = phi_at_f64(parts[b], 300, pts[b], SOFT)
        assert np.all(want < 0.0)
        err = np.abs(phi[b].astype(np.float64) - want)
        g64, mag = g_at_f64(parts[b], 300, pts[b], SOFT)
        bound = acc_bound(g64, mag)
        worst = float(np.max(np.abs(g[b].astype(np.float64) - g64) / bound))
        print(f"[batch field] member {b}: Phi worst relative error {np.max(err / np.abs(want)):.3e}, g worst error / bound {worst:.3f}")
        assert np.all(err <= 1e-5 * np.abs(want))
        assert worst <= 1.0


# ---- changes nothing ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [250, 600])
def test_calls_between_two_steps_change_nothing_a_step_a_read_back_or_a_timer_can_observe(n):
    mass_lens = [n // 2, n, 0]
    parts = [world(n, m, seed=700 + n + b) for b, m in enumerate(mass_lens)]
    a, b = uniform(parts, mass_lens), uniform(parts, mass_lens)
    a.update(1, DT)
    b.update(1, DT)
    step_ms, uploads = a.last_ms(), a.dt_uploads()
    vs, pts = views(3, 33, 5), points(130, seed=n)
    first = a.potential_map(vs, SOFT)
    assert a.last_diag_ms() > 0.0
    same(a.potential_map(vs, SOFT), first, "two consecutive maps")
    a.acceleration_map(vs, SOFT)
    a.potential_at(pts, SOFT)
    a.acceleration_at(pts, SOFT)
    assert a.last_diag_ms() > 0.0 and a.last_ms() == step_ms and a.dt_uploads() == uploads
    assert a.get_data().tobytes() == b.get_data().tobytes()
    assert a.energy() == b.energy()
    a.update(1, DT)
    b.update(1, DT)
    assert a.get_data().tobytes() == b.get_data().tobytes()          # step / calls / step == step / step
    assert a.dt_uploads() == b.dt_uploads()
    a.close()
    b.close()


# ---- edge values ----------------------------------------------------------------------------------------------------------------

def test_non_finite_points_give_nan_exactly_there_and_no_points_give_an_empty_array(three_of_300):
    batch, parts = three_of_300
    pts = np.stack([points(130, seed=800 + b) for b in range(3)])
    clean_phi, clean_g = batch.potential_at(pts, SOFT), batch.acceleration_at(pts, SOFT)
    bad = pts.copy()
    hit = np.zeros((3, 130), dtype=bool)
    for b, i, p in ((0, 1, (np.nan, 0.0)), (1, 64, (0.0, np.inf)), (2, 129, (-np.inf, np.nan)), (2, 0, (np.nan, np.nan))):
        bad[b, i] = p
        hit[b, i] = True
    phi, g = batch.potential_at(bad, SOFT), batch.acceleration_at(bad, SOFT)
    assert np.array_equal(np.isnan(phi), hit) and np.array_equal(np.isnan(g), np.stack([hit, hit], axis=-1))
    assert phi[~hit].tobytes() == clean_phi[~hit].tobytes() and g[~hit].tobytes() == clean_g[~hit].tobytes()
    img = batch.potential_map([nb.RenderView.make((0.0, 0.0), (0.0, 0.0), 1.0, 5, 3, 1.0), nb.RenderView.make((np.nan, 0.0), (0.0, 0.0), 1.0, 5, 3, 1.0),
                               nb.RenderView.make((0.0, 0.0), (0.0, 0.0), 1.0, 5, 3, 1.0)], SOFT)
    assert np.isnan(img[1]).all() and np.isfinite(img[[0, 2]]).all()
    assert batch.last_diag_ms() > 0.0
    empty = batch.potential_at(np.zeros((0, 2), dtype=np.float32), SOFT)
    assert empty.shape == (3, 0) and empty.dtype == np.float32 and batch.last_diag_ms() == 0.0      # nothing ran: the timer is cleared
    assert batch.acceleration_at(np.zeros((3, 0, 2), dtype=np.float32), SOFT).shape == (3, 0, 2)


# ---- through the WorldBatch --------------------------------------------------------------------------------------------------------

def test_a_world_batch_answers_on_the_device_after_gpu_steps_and_on_the_host_after_a_read_back():
    mass_lens = [150, 300, 1]
    parts = [world(300, m, seed=850 + b) for b, m in enumerate(mass_lens)]
    wb = nb.WorldBatch(np.stack(parts))
    wb.update_gpu(DT, 2)
    pts, vs = np.stack([points(129, seed=860 + b) for b in range(3)]), views(3, 33, 5)

    def four():
        return (wb.potential_at(pts, SOFT), wb.acceleration_at(pts, SOFT), wb.potential_map(vs, SOFT), wb.acceleration_map(vs, SOFT))

    device = four()
    state = wb.particles()          # the host array is current from here on
    host = four()
    wb.close()
    seam = uniform(list(state), mass_lens)
    for call, d, x in zip(CALLS, device, (seam.potential_at(pts, SOFT), seam.acceleration_at(pts, SOFT),
                                          seam.potential_map(vs, SOFT), seam.acceleration_map(vs, SOFT))):
        same(d, x, ("WorldBatch on the device = the seam", call))
    seam.close()
    for b in range(3):
        where = {"potential_at": pts[b], "acceleration_at": pts[b], "potential_map": pixel_points(vs[b]), "acceleration_map": pixel_points(vs[b])}
        for call, d, h in zip(CALLS, device, host):
            d64, h64 = d[b].astype(np.float64), h[b].astype(np.float64)
            if call.startswith("potential"):
                assert np.all(np.abs(d64 - h64) <= 1e-5 * np.abs(h64)), (call, b)
            else:
                g64, mag = g_at_f64(state[b], mass_lens[b], where[call], SOFT)
                assert np.all(np.abs(d64.reshape(-1, 2) - h64.reshape(-1, 2)) <= acc_bound(g64, mag)), (call, b)
    assert any(not np.array_equal(d, h) for d, h in zip(device, host))          # two paths: float32 sums against float64 ones


# ---- life cycle -----------------------------------------------------------------------------------------------------------------

def test_an_ensemble_that_made_all_four_calls_returns_every_buffer_and_event():
    def make_and_use():
        parts = [world(n, m, seed=950 + n) for n, m in zip(RAGGED_SIZES[:3], RAGGED_MASS[:3])]
        batch = nb.SimBatch.ragged(RAGGED_SIZES[:3], RAGGED_MASS[:3])
        batch.set_data(parts)
        batch.update(1, DT)
        pts, view = points(200, seed=951), views(1, 40, 9)[0]
        batch.potential_at(pts, SOFT)
        batch.acceleration_map(view, SOFT)          # the result buffer grows
        batch.potential_map(view, SOFT)
        batch.acceleration_at(pts, SOFT)
        return batch

    returns_what_it_took(make_and_use)
