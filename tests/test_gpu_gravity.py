"""The acceleration at probe points and as a map on the GPU (nb_hip_acceleration_at / nb_hip_acceleration_map,
GetWorldAccelerationAt / RenderWorldAcceleration of a World whose device holds the newest state): both kernel shapes give the
same bits, a sample's result depends on its place and the world alone, map = probes, accuracy against float64 and against
the step kernel within the project's force tolerance, and the calls change nothing a step, a read-back or a timer can
observe.  No wall-clock assertions here."""
import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
import render_ref as rr
from gpu_common import acc_bound, synth
from gravity_ref import augmented, g_at_f64, pixel_points, probes

pytestmark = pytest.mark.gpu

DT = 0.01
SOFT = 0.75
SPLIT, WAVE = 1, 2          # the "gravity_shape" tuning hook: source split / one wave per tile


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def pipeline(part, m, **knobs):
    sim = nb.SimPipeline(part.shape[0], m)
    sim.configure(**knobs)
    sim.set_data(part)
    return sim


def world(m, extra=50, seed=0):
    """m massive particles followed by `extra` massless ones: partitioned as built (tests/test_gpu_field.py's builder)."""
    rng = np.random.default_rng(1000 + seed)
    a = np.zeros((m + extra, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((m + extra, 2)) * 1.0e3
    a[:, 2:4] = rng.standard_normal((m + extra, 2))
    a[:, 7] = 0.5 + rng.random(m + extra)
    a[:m, 6] = 10.0 + 990.0 * rng.random(m)
    return a


def offset_view(width, height):
    return nb.RenderView.make((120.0, -40.0), (-3.5, -11.25), 0.37, width, height, 1.0)


def points_for(part, m):
    pts = probes(part, max(COUNTS), seed=m)
    if m > 0:
        pts[0] = part[m - 1, 0:2]          # a probe exactly on a source: a zero term, a finite result
    return pts


# a ragged tail only, a block edge, one block per wave (2 048 = 8 blocks), per = 2 with empty trailing slices
SOURCES = [0, 1, 7, 255, 256, 257, 300, 2048, 2049, 4500]
COUNTS = [1, 127, 128, 129, 1000]          # the tile edges


# ---- the kernel shapes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", SOURCES)
def test_both_shapes_and_auto_give_the_same_bytes(m):
    part = world(m, seed=m)
    pts = points_for(part, m)
    sim = pipeline(part, m)
    for n in COUNTS:
        got = {}
        for shape in (SPLIT, WAVE, 0):
            sim.configure(gravity_shape=shape)
            got[shape] = sim.acceleration_at(pts[:n], SOFT)
            assert got[shape].dtype == np.float32 and got[shape].shape == (n, 2) and np.all(np.isfinite(got[shape])), (m, n, shape)
        for shape in (WAVE, 0):
            assert got[shape].tobytes() == got[SPLIT].tobytes(), (m, n, shape, int(np.count_nonzero(got[shape] != got[SPLIT])))
        if m == 0:
            assert not got[SPLIT].view(np.uint32).any()          # (+0, +0)
        if m == 1 and n == 1:
            assert got[SPLIT].tolist() == [[0.0, 0.0]]          # the probe on the only source feels nothing
    sim.close()


@pytest.mark.parametrize("m", SOURCES)
def test_a_samples_result_depends_on_nothing_but_its_place_and_the_world(m):
    part = world(m, seed=m)
    pts = points_for(part, m)
    sim = pipeline(part, m)
    rng = np.random.default_rng(m)
    for shape in (SPLIT, WAVE):
        sim.configure(gravity_shape=shape)
        whole = sim.acceleration_at(pts, SOFT)
        for n in COUNTS:
            assert sim.acceleration_at(pts[:n], SOFT).tobytes() == whole[:n].tobytes(), (m, n, shape, "prefix")
            perm = rng.permutation(n)
            assert sim.acceleration_at(pts[:n][perm], SOFT).tobytes() == whole[:n][perm].tobytes(), (m, n, shape, "permuted")
    sim.close()


# ---- map = probes ---------------------------------------------------------------------------------------------------------

IMAGES = [(1, 1), (128, 1), (1, 129), (37, 7), (64, 64)]


@pytest.mark.parametrize("m", [300, 2049])
def test_a_map_is_the_probes_product_at_the_pixel_centres(m):
    part = world(m, seed=7)
    sim = pipeline(part, m)
    # 1280 x 720 over the small world is where "auto" takes one wave per tile (7 200 tiles, 2 source blocks)
    for width, height in IMAGES + ([(1280, 720)] if m == 300 else []):
        for view in (rr.fit_view(part, width, height), offset_view(width, height)):
            pts = pixel_points(view)
            sim.configure(gravity_shape=SPLIT)
            want = sim.acceleration_at(pts, SOFT)
            for shape in (0, SPLIT, WAVE):
                sim.configure(gravity_shape=shape)
                img = sim.acceleration_map(view, SOFT)
                assert img.dtype == np.float32 and img.shape == (height, width, 2)
                assert img.tobytes() == want.tobytes(), (width, height, shape, int(np.count_nonzero(img.reshape(-1, 2) != want)))
            sim.configure(gravity_shape=0)
    sim.close()


# ---- accuracy ---------------------------------------------------------------------------------------------------------------

def ratio_to_bound(got, g64, mag):
    """worst |got - g64| / acc_bound per component; acc_bound = 1e-4 |g| + 1e-6 sum |terms| (tests/gpu_common.py)."""
    bound = acc_bound(g64, mag)
    assert np.all(bound > 0.0)
    return float(np.max(np.abs(got.astype(np.float64) - g64) / bound))


def check_map(part, m, width, height):
    """A purely relative bound would be wrong here: a component cancels to 1e-3 of its terms at some pixels.  A numpy
    emulation of the kernels' summation order with a correctly rounded rsq stays at <= 0.29 of this bound."""
    view = rr.fit_view(part, width, height)
    g64, mag = g_at_f64(part, m, pixel_points(view), SOFT)
    assert m > 0 and np.all(np.isfinite(g64))
    sim = pipeline(part, m)
    img = sim.acceleration_map(view, SOFT)
    sim.close()
    worst = ratio_to_bound(img.reshape(-1, 2), g64, mag)
    print(f"[gravity] {part.shape[0]} particles, {width} x {height}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, f"worst error / bound {worst:.3f}"


def test_map_of_the_1024_fixture_against_f64(golden):
    part, m = ob.partition(golden("ic_1024.bin"))
    check_map(part, m, 32, 32)


def test_map_of_a_synthetic_world_of_4096_against_f64():
    part, m = synth(4096, seed=4096)
    check_map(part, m, 64, 32)


@pytest.mark.parametrize("m", [300, 2049])
def test_probes_against_the_step_kernels_acc_of_massless_particles_of_radius_s(m):
    part = world(m, seed=m)
    n_part = part.shape[0]
    pts = points_for(part, m)
    sim = pipeline(part, m)
    got = sim.acceleration_at(pts, SOFT)
    sim.close()
    both = augmented(part, pts, SOFT)
    aug = pipeline(both, m)
    aug.update(1, 0.0)
    after = aug.get_data()
    aug.close()
    assert np.array_equal(after[:, 0:2], both[:, 0:2])          # dt = 0: nothing moved
    step = after[n_part:, 4:6]
    g64, mag = g_at_f64(part, m, pts, SOFT)
    bound = acc_bound(g64, mag)
    print(f"[gravity] M = {m}: probes / bound {ratio_to_bound(got, g64, mag):.3f}, step / bound {ratio_to_bound(step, g64, mag):.3f}")
    diff = np.abs(got.astype(np.float64) - step.astype(np.float64))
    assert np.all(diff <= 2.0 * bound), float(np.max(diff / bound))          # each side within its own acc_bound of g64


# ---- through the World ------------------------------------------------------------------------------------------------------

def test_world_map_after_gpu_steps_runs_on_the_device_and_agrees_with_the_host_path(golden):
    w = nb.World(golden("ic_1024.bin"))
    w.update_gpu(DT, 3)
    view = w.fit_view(48, 20)
    pts = probes(golden("ic_1024.bin"), 300, seed=5)
    img = w.acceleration_map(view, SOFT)
    ms_map = float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline()))
    at = w.acceleration_at(pts, SOFT)
    ms_at = float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline()))
    assert ms_map > 0.0 and ms_at > 0.0          # the device path ran
    state = w.particles()
    m = int(np.count_nonzero(state[:, 6] > 0))
    # after a CPU step the array is newer than the device: the same call runs on the host and leaves the timer alone
    w.update_cpu(DT, 1)
    stepped = w.particles()
    host_img = w.acceleration_map(view, SOFT)
    assert float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline())) == ms_at
    w.close()
    g64, mag = g_at_f64(stepped, m, pixel_points(view), SOFT)
    assert np.all(np.abs(host_img.reshape(-1, 2).astype(np.float64) - g64) <= 6e-8 * np.abs(g64) + 1e-30)
    host = nb.World(state)                       # never stepped: the host path, on the state the device held
    assert host.particles().tobytes() == state.tobytes()
    want_img, want_at = host.acceleration_map(view, SOFT), host.acceleration_at(pts, SOFT)
    host.close()
    for got, want, where in ((img, want_img, pixel_points(view)), (at, want_at, pts)):
        g64, mag = g_at_f64(state, m, where, SOFT)
        err = np.abs(got.reshape(-1, 2).astype(np.float64) - want.reshape(-1, 2).astype(np.float64))
        bound = acc_bound(g64, mag)
        assert np.all(err <= bound), f"worst error / bound {np.max(err / bound):.3f}"


# ---- changes nothing ----------------------------------------------------------------------------------------------------------

def test_a_map_between_two_steps_changes_nothing_a_step_a_read_back_or_a_timer_can_observe(golden):
    part, m = ob.partition(golden("ic_1024.bin"))
    view = rr.fit_view(part, 40, 24)
    pts = probes(part, 200, seed=6)
    a, b = pipeline(part, m, timing=1), pipeline(part, m, timing=1)
    a.update(2, DT)
    b.update(2, DT)
    a.update(2, DT)          # the chain length's second use: cached from here on
    b.update(2, DT)
    step_ms = a.last_step_ms()
    stats = a.graph_stats()
    assert step_ms[0] > 0.0
    first = a.acceleration_map(view, SOFT)
    assert a.acceleration_map(view, SOFT).tobytes() == first.tobytes()          # two consecutive maps
    at = a.acceleration_at(pts, SOFT)
    assert a.acceleration_at(pts, SOFT).tobytes() == at.tobytes()
    assert a.last_step_ms() == step_ms and a.graph_stats() == stats and a.last_diag_ms() > 0.0
    assert a.get_data().tobytes() == b.get_data().tobytes()
    # the step knobs do not reach the gravity kernels
    for knobs in (dict(variant=0), dict(variant=1), dict(graph=0), dict(graph=1)):
        a.configure(**knobs)
        assert a.acceleration_map(view, SOFT).tobytes() == first.tobytes(), knobs
    a.configure(variant=1, graph=2)          # back to the defaults b never left
    a.update(2, DT)
    b.update(2, DT)
    assert a.get_data().tobytes() == b.get_data().tobytes()                  # step / map / step == step / step
    a.close()
    b.close()


# ---- edge values ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SPLIT, WAVE])
def test_non_finite_points_give_nan_pairs_and_no_points_give_an_empty_array(shape):
    part = world(300, seed=3)
    sim = pipeline(part, 300, gravity_shape=shape)
    pts = probes(part, 130, seed=2)
    bad = {1: (np.nan, 0.0), 64: (0.0, np.inf), 129: (-np.inf, np.nan)}
    for i, p in bad.items():
        pts[i] = p
    g = sim.acceleration_at(pts, SOFT)
    nan = np.isnan(g)
    assert np.array_equal(nan[:, 0], nan[:, 1]) and sorted(np.flatnonzero(nan[:, 0]).tolist()) == sorted(bad)
    good = np.array([i for i in range(130) if i not in bad])
    assert g[good].tobytes() == sim.acceleration_at(pts[good], SOFT).tobytes()      # the neighbours are untouched
    empty = sim.acceleration_at(np.zeros((0, 2), dtype=np.float32), SOFT)
    assert empty.shape == (0, 2) and empty.dtype == np.float32 and sim.last_diag_ms() == 0.0
    img = sim.acceleration_map(nb.RenderView.make((np.nan, 0.0), (0.0, 0.0), 1.0, 5, 3, 1.0), SOFT)
    assert img.shape == (3, 5, 2) and np.isnan(img).all()
    sim.close()
