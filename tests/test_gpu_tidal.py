"""The tidal tensor at probe points and as a map on the GPU (nb_hip_tidal_at / nb_hip_tidal_map, GetWorldTidalAt /
RenderWorldTidal of a World whose device holds the newest state): both kernel shapes give the same bits, a sample's result
depends on its place and the world alone, map = probes, accuracy against float64 within the project's force tolerance form,
and the calls change nothing a step, a read-back or a timer can observe.  No wall-clock assertions here."""
import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
import render_ref as rr
from gpu_common import synth
from tidal_ref import pixel_points, probes, ratio_to_bound, t_at_f64, tidal_bound

pytestmark = pytest.mark.gpu

DT = 0.01
SOFT = 0.75
SPLIT, WAVE = 1, 2          # the "tidal_shape" tuning hook: source split / one wave per tile


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
    """m massive particles followed by `extra` massless ones: partitioned as built (tests/test_gpu_gravity.py's builder)."""
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
        pts[0] = part[m - 1, 0:2]          # a probe exactly on a source: its term is diag(-G m s^-1.5), finite
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
            sim.configure(tidal_shape=shape)
            got[shape] = sim.tidal_at(pts[:n], SOFT)
            assert got[shape].dtype == np.float32 and got[shape].shape == (n, 3) and np.all(np.isfinite(got[shape])), (m, n, shape)
        for shape in (WAVE, 0):
            assert got[shape].tobytes() == got[SPLIT].tobytes(), (m, n, shape, int(np.count_nonzero(got[shape] != got[SPLIT])))
        if m == 0:
            assert not got[SPLIT].view(np.uint32).any()          # three +0
        if m == 1 and n == 1:
            # the probe on the only source: diag(-G m s^-1.5) from a v_rsq_f32 of s (1 ulp) cubed, and +0 beside it
            t = got[SPLIT][0]
            want = -float(np.float32(nb.NB_G) * part[0, 6]) * SOFT ** -1.5
            assert t[0] == t[2] and abs(float(t[0]) - want) <= 1e-6 * abs(want) and t[1] == 0.0 and not np.signbit(t[1]), t
    sim.close()


@pytest.mark.parametrize("m", SOURCES)
def test_a_samples_result_depends_on_nothing_but_its_place_and_the_world(m):
    part = world(m, seed=m)
    pts = points_for(part, m)
    sim = pipeline(part, m)
    rng = np.random.default_rng(m)
    for shape in (SPLIT, WAVE):
        sim.configure(tidal_shape=shape)
        whole = sim.tidal_at(pts, SOFT)
        for n in COUNTS:
            assert sim.tidal_at(pts[:n], SOFT).tobytes() == whole[:n].tobytes(), (m, n, shape, "prefix")
            perm = rng.permutation(n)
            assert sim.tidal_at(pts[:n][perm], SOFT).tobytes() == whole[:n][perm].tobytes(), (m, n, shape, "permuted")
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
            sim.configure(tidal_shape=SPLIT)
            want = sim.tidal_at(pts, SOFT)
            for shape in (0, SPLIT, WAVE):
                sim.configure(tidal_shape=shape)
                img = sim.tidal_map(view, SOFT)
                assert img.dtype == np.float32 and img.shape == (height, width, 3)
                assert img.tobytes() == want.tobytes(), (width, height, shape, int(np.count_nonzero(img.reshape(-1, 3) != want)))
            sim.configure(tidal_shape=0)
    sim.close()


# ---- accuracy ---------------------------------------------------------------------------------------------------------------

def check_map(part, m, width, height):
    """1e-4 |T| + 1e-6 mag per component, mag the sum of the absolute parts (tests/tidal_ref.py): a purely relative bound
    would be wrong where a diagonal component cancels.  The numpy model of the statement (tests/test_tidal_cpu.py) stays at
    0.60 - 0.69 of this bound on the 1024 fixture and at 0.30 - 0.41 on synth(4096), rsq exact or one ulp off."""
    view = rr.fit_view(part, width, height)
    t64, mag = t_at_f64(part, m, pixel_points(view), SOFT)
    assert m > 0 and np.all(np.isfinite(t64))
    sim = pipeline(part, m)
    img = sim.tidal_map(view, SOFT)
    sim.close()
    worst = ratio_to_bound(img, t64, mag)
    print(f"[tidal] {part.shape[0]} particles, {width} x {height}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, f"worst error / bound {worst:.3f}"


def test_map_of_the_1024_fixture_against_f64(golden):
    part, m = ob.partition(golden("ic_1024.bin"))
    check_map(part, m, 32, 32)


def test_map_of_a_synthetic_world_of_4096_against_f64():
    part, m = synth(4096, seed=4096)
    check_map(part, m, 64, 32)


# ---- through the World ------------------------------------------------------------------------------------------------------

def test_world_map_after_gpu_steps_runs_on_the_device_and_agrees_with_the_host_path(golden):
    w = nb.World(golden("ic_1024.bin"))
    w.update_gpu(DT, 3)
    view = w.fit_view(48, 20)
    pts = probes(golden("ic_1024.bin"), 300, seed=5)
    img = w.tidal_map(view, SOFT)
    ms_map = float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline()))
    at = w.tidal_at(pts, SOFT)
    ms_at = float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline()))
    assert ms_map > 0.0 and ms_at > 0.0          # the device path ran
    state = w.particles()
    m = int(np.count_nonzero(state[:, 6] > 0))
    # after a CPU step the array is newer than the device: the same call runs on the host and leaves the timer alone
    w.update_cpu(DT, 1)
    stepped = w.particles()
    host_img = w.tidal_map(view, SOFT)
    assert float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline())) == ms_at
    w.close()
    t64, mag = t_at_f64(stepped, m, pixel_points(view), SOFT)
    assert np.all(np.abs(host_img.reshape(-1, 3).astype(np.float64) - t64) <= 6e-8 * np.abs(t64) + 1e-12 * mag + 1e-30)
    host = nb.World(state)                       # never stepped: the host path, on the state the device held
    assert host.particles().tobytes() == state.tobytes()
    want_img, want_at = host.tidal_map(view, SOFT), host.tidal_at(pts, SOFT)
    host.close()
    for got, want, where in ((img, want_img, pixel_points(view)), (at, want_at, pts)):
        t64, mag = t_at_f64(state, m, where, SOFT)
        err = np.abs(got.reshape(-1, 3).astype(np.float64) - want.reshape(-1, 3).astype(np.float64))
        bound = tidal_bound(t64, mag)
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
    first = a.tidal_map(view, SOFT)
    assert a.tidal_map(view, SOFT).tobytes() == first.tobytes()          # two consecutive maps
    at = a.tidal_at(pts, SOFT)
    assert a.tidal_at(pts, SOFT).tobytes() == at.tobytes()
    assert a.last_step_ms() == step_ms and a.graph_stats() == stats and a.last_diag_ms() > 0.0
    assert a.get_data().tobytes() == b.get_data().tobytes()
    # the step knobs do not reach the tidal kernels
    for knobs in (dict(variant=0), dict(variant=1), dict(graph=0), dict(graph=1)):
        a.configure(**knobs)
        assert a.tidal_map(view, SOFT).tobytes() == first.tobytes(), knobs
    a.configure(variant=1, graph=2)          # back to the defaults b never left
    a.update(2, DT)
    b.update(2, DT)
    assert a.get_data().tobytes() == b.get_data().tobytes()                  # step / map / step == step / step
    a.close()
    b.close()


# ---- edge values ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SPLIT, WAVE])
def test_non_finite_points_give_nan_triples_and_no_points_give_an_empty_array(shape):
    part = world(300, seed=3)
    sim = pipeline(part, 300, tidal_shape=shape)
    pts = probes(part, 130, seed=2)
    bad = {1: (np.nan, 0.0), 64: (0.0, np.inf), 129: (-np.inf, np.nan)}
    for i, p in bad.items():
        pts[i] = p
    t = sim.tidal_at(pts, SOFT)
    nan = np.isnan(t)
    assert np.array_equal(nan[:, 0], nan[:, 1]) and np.array_equal(nan[:, 0], nan[:, 2])
    assert sorted(np.flatnonzero(nan[:, 0]).tolist()) == sorted(bad)
    good = np.array([i for i in range(130) if i not in bad])
    assert t[good].tobytes() == sim.tidal_at(pts[good], SOFT).tobytes()      # the neighbours are untouched
    empty = sim.tidal_at(np.zeros((0, 2), dtype=np.float32), SOFT)
    assert empty.shape == (0, 3) and empty.dtype == np.float32 and sim.last_diag_ms() == 0.0
    img = sim.tidal_map(nb.RenderView.make((np.nan, 0.0), (0.0, 0.0), 1.0, 5, 3, 1.0), SOFT)
    assert img.shape == (3, 5, 3) and np.isnan(img).all()
    sim.close()
