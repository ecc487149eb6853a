"""The potential at probe points and as a map on the GPU (nb_hip_potential_at / nb_hip_potential_map, GetWorldPotentialAt /
RenderWorldPotential of a World whose device holds the newest state): bitwise against nb_hip_potential of the same world
with the probes appended as massless particles, on both kernel shapes; map = probes; accuracy against float64; and that the
calls change nothing a step, a read-back or a timer can observe.  No wall-clock assertions here."""
import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
import render_ref as rr
from field_ref import augmented, phi_at_f64, pixel_points, probes
from gpu_common import synth

pytestmark = pytest.mark.gpu

DT = 0.01
SOFT = 0.75
SPLIT, WAVE = 1, 2          # the "field_shape" tuning hook: source split / one wave per tile


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
    """m massive particles followed by `extra` massless ones: partitioned as built."""
    rng = np.random.default_rng(1000 + seed)
    a = np.zeros((m + extra, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((m + extra, 2)) * 1.0e3
    a[:, 2:4] = rng.standard_normal((m + extra, 2))
    a[:, 7] = 0.5 + rng.random(m + extra)
    a[:m, 6] = 10.0 + 990.0 * rng.random(m)
    return a


def offset_view(width, height):
    return nb.RenderView.make((120.0, -40.0), (-3.5, -11.25), 0.37, width, height, 1.0)


# ---- bitwise against the existing kernel -----------------------------------------------------------------------------------

# a ragged tail only, a block edge, one block per wave (2 048 = 8 blocks), per = 2 with empty trailing waves
SOURCES = [0, 1, 7, 255, 256, 257, 300, 2048, 2049, 4500]
COUNTS = [1, 127, 128, 129, 1000]          # the tile edges


@pytest.mark.parametrize("m", SOURCES)
def test_probes_have_the_bits_of_massless_particles_in_nb_hip_potential(m):
    part = world(m, seed=m)
    n_part = part.shape[0]
    pts = probes(part, max(COUNTS), seed=m)
    if m > 0:
        pts[0] = part[m - 1, 0:2]          # a probe exactly on a source: finite, and the augmented pipeline's value
    sim = pipeline(part, m)
    for n in COUNTS:
        aug = pipeline(augmented(part, pts[:n], SOFT), m)
        want = aug.potential()[n_part:]
        aug.close()
        assert want.shape == (n,) and np.all(np.isfinite(want))
        got = {}
        for shape in (SPLIT, WAVE):
            sim.configure(field_shape=shape)
            got[shape] = sim.potential_at(pts[:n], SOFT)
            assert got[shape].dtype == np.float32 and got[shape].tobytes() == want.tobytes(), \
                (m, n, shape, int(np.count_nonzero(got[shape] != want)))
        assert got[SPLIT].tobytes() == got[WAVE].tobytes()
        sim.configure(field_shape=0)
        assert sim.potential_at(pts[:n], SOFT).tobytes() == want.tobytes(), (m, n, "auto")
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
            want = sim.potential_at(pts, SOFT)
            for shape in (0, SPLIT, WAVE):
                sim.configure(field_shape=shape)
                img = sim.potential_map(view, SOFT)
                assert img.dtype == np.float32 and img.shape == (height, width)
                assert img.tobytes() == want.tobytes(), (width, height, shape, int(np.count_nonzero(img.reshape(-1) != want)))
            sim.configure(field_shape=0)
    sim.close()


# ---- accuracy ---------------------------------------------------------------------------------------------------------------

def check_map(part, m, width, height):
    view = rr.fit_view(part, width, height)
    want = phi_at_f64(part, m, pixel_points(view), SOFT)
    # Phi is strictly negative with M > 0: there is no pixel at which a relative bound is meaningless
    assert m > 0 and np.all(want < 0.0) and np.all(np.isfinite(want))
    sim = pipeline(part, m)
    img = sim.potential_map(view, SOFT)
    sim.close()
    err = np.abs(img.reshape(-1).astype(np.float64) - want)
    print(f"[field] {part.shape[0]} particles, {width} x {height}: worst relative error {np.max(err / np.abs(want)):.3e}")
    assert np.all(err <= 1e-5 * np.abs(want)), f"worst {np.max(err / np.abs(want)):.3e}"


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
    img = w.potential_map(view, SOFT)
    ms_map = float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline()))
    phi = w.potential_at(pts, SOFT)
    ms_at = float(nb.hip_lib().nb_hip_last_diag_ms(w.pipeline()))
    assert ms_map > 0.0 and ms_at > 0.0          # the device path ran
    state = w.particles()
    w.close()
    host = nb.World(state)                       # never stepped: the host path, on the state the device held
    assert host.particles().tobytes() == state.tobytes()
    want_img, want_phi = host.potential_map(view, SOFT), host.potential_at(pts, SOFT)
    host.close()
    for got, want in ((img, want_img), (phi, want_phi)):
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert np.all(err <= 1e-5 * np.abs(want)), f"worst {np.max(err / np.abs(want)):.3e}"


# ---- changes nothing ----------------------------------------------------------------------------------------------------------

def test_a_map_between_two_steps_changes_nothing_a_step_a_read_back_or_a_timer_can_observe(golden):
    part, m = ob.partition(golden("ic_1024.bin"))
    view = rr.fit_view(part, 40, 24)
    pts = probes(part, 200, seed=6)
    a, b = pipeline(part, m), pipeline(part, m)
    a.update(2, DT)
    b.update(2, DT)
    step_ms = a.last_step_ms()
    stats = a.graph_stats()
    first = a.potential_map(view, SOFT)
    assert a.potential_map(view, SOFT).tobytes() == first.tobytes()          # two consecutive maps
    at = a.potential_at(pts, SOFT)
    assert a.potential_at(pts, SOFT).tobytes() == at.tobytes()
    assert a.last_step_ms() == step_ms and a.graph_stats() == stats and a.last_diag_ms() > 0.0
    assert a.get_data().tobytes() == b.get_data().tobytes()
    # the step knobs do not reach the field kernels
    for knobs in (dict(variant=0), dict(variant=1), dict(graph=0), dict(graph=1)):
        a.configure(**knobs)
        assert a.potential_map(view, SOFT).tobytes() == first.tobytes(), knobs
    a.configure(variant=1, graph=2)          # back to the defaults b never left
    a.update(2, DT)
    b.update(2, DT)
    assert a.get_data().tobytes() == b.get_data().tobytes()                  # step / map / step == step / step
    a.close()
    b.close()


# ---- edge values ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SPLIT, WAVE])
def test_non_finite_points_give_nan_and_no_points_give_an_empty_array(shape):
    part = world(300, seed=3)
    sim = pipeline(part, 300, field_shape=shape)
    pts = probes(part, 130, seed=2)
    bad = {1: (np.nan, 0.0), 64: (0.0, np.inf), 129: (-np.inf, np.nan)}
    for i, p in bad.items():
        pts[i] = p
    phi = sim.potential_at(pts, SOFT)
    assert sorted(np.flatnonzero(np.isnan(phi)).tolist()) == sorted(bad)
    good = np.array([i for i in range(130) if i not in bad])
    assert phi[good].tobytes() == sim.potential_at(pts[good], SOFT).tobytes()      # the neighbours are untouched
    empty = sim.potential_at(np.zeros((0, 2), dtype=np.float32), SOFT)
    assert empty.shape == (0,) and sim.last_diag_ms() == 0.0
    img = sim.potential_map(nb.RenderView.make((np.nan, 0.0), (0.0, 0.0), 1.0, 5, 3, 1.0), SOFT)
    assert np.isnan(img).all()
    sim.close()
