"""Rendering on the GPU (nb_hip_bounds / nb_hip_render_counts / nb_hip_render_rgba, and the World calls of
include/nbody_render.h when the device holds the newest state): BITWISE against the numpy restatement (tests/render_ref.py)
and against the host path, reproducibility, and that a render changes nothing a step, a read-back or a timer can observe.
No wall-clock assertions here."""
import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
import render_ref as rr
from gpu_common import bench_universe

pytestmark = pytest.mark.gpu

DT = 0.01
VIEWS = {"fitted": lambda p: rr.fit_view(p, 1280, 720), "edge": rr.edge_view, "mixed": rr.mixed_view, "collapsed": rr.collapsed_view,
         "nothing": rr.empty_view, "1x1": lambda p: rr.fit_view(p, 1, 1), "37x53": lambda p: rr.fit_view(p, 37, 53)}


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def pipeline(part, m, **knobs):
    sim = nb.SimPipeline(part.shape[0], m)
    sim.configure(**knobs)
    sim.set_data(part)
    return sim


def host(part, view, palette=None):
    w = nb.World(part)            # CPU only: the host path
    out = w.render_counts(view), w.render(view, palette), w.bounds()
    w.close()
    return out


def check_mix(part, name, view):
    return rr.check_mix(part, view, want_points=name in ("fitted", "edge", "mixed", "37x53"), want_discs=name == "mixed",
                        want_off_centre_disc=name == "edge")


@pytest.mark.parametrize("fixture", ["ic_333.bin", "ic_1024.bin", "ic_4096.bin"])
def test_fixtures_against_the_numpy_restatement(golden, fixture):
    part, m = ob.partition(golden(fixture))
    sim = pipeline(part, m)
    assert sim.bounds().tobytes() == rr.bounds(part).tobytes()
    pal = nb.default_palette()
    for name, make in VIEWS.items():
        view = make(part)
        check_mix(part, name, view)
        want = rr.counts(part, view)
        got = sim.render_counts(view)
        assert np.array_equal(got, want), (name, int(np.count_nonzero(got != want)))
        assert np.array_equal(sim.render(view), rr.shade_with(want, pal)), name
    custom = nb.RenderPalette.make((10, 20, 30, 40), ((200, 100, 0, 255), (1, 2, 3, 4), (255, 254, 253, 128)), 3)
    view = VIEWS["mixed"](part)
    assert np.array_equal(sim.render(view, custom), rr.shade_with(rr.counts(part, view), custom))
    sim.close()


@pytest.mark.parametrize("n", [65536, 1 << 20])
def test_galaxy_worlds_against_the_host_path(n):
    _, part, m = bench_universe(n)
    sim = pipeline(part, m)
    assert sim.bounds().tobytes() == host(part, rr.fit_view(part, 8, 8))[2].tobytes() == rr.bounds(part).tobytes()
    for name in ("fitted", "edge", "mixed", "collapsed"):
        view = VIEWS[name](part)
        d = check_mix(part, name, view)
        cnt, img, _ = host(part, view)
        got = sim.render_counts(view)
        print(f"[render] N={n} {name}: points {d['points']}, discs on screen {d['discs_on_screen']}, max count {int(got.max())}")
        assert np.array_equal(got, cnt), (name, int(np.count_nonzero(got != cnt)))
        assert np.array_equal(sim.render(view), img), name
        if name == "collapsed":
            assert int(got.sum(dtype=np.uint64)) == n and int(got[:, 360, 640].sum()) == n
        if n == 65536:
            assert np.array_equal(cnt, rr.counts(part, view)), name
        sim.configure(render_merge=0)           # the one-atomic-per-lane build of the splat: the same bits
        assert np.array_equal(sim.render_counts(view), cnt), name
        sim.configure(render_merge=1)
    sim.close()


def test_hand_made_edges_and_non_finite_particles():
    below = float(np.nextafter(np.float32(8.0), np.float32(0.0)))
    rows = [(0.0, 0.0, 1.0, 0.5), (8.0, 1.0, 1.0, 0.5), (below, 1.0, 1.0, 0.5), (-0.0, 2.0, 1.0, 0.5), (3.0, -0.0, 1.0, 0.5),
            (6.0, 2.0, 1.0, 1.0), (2.5, 1.5, 1.0, float(np.nextafter(np.float32(1.0), np.float32(0.0)))), (np.nan, 1.0, 1.0, 0.5),
            (1.0, np.inf, 1.0, 0.5), (2.0, 2.0, 1.0, np.nan), (2.0, 2.0, 1.0, np.inf), (-np.inf, 0.0, 500.0, 0.5), (-40.0, 2.0, 500.0, 42.0),
            (5.0, 3.0, 0.0, 0.5), (-1.0, 1.0, 0.0, 2.0)]
    a = np.zeros((len(rows), 8), dtype=np.float32)
    a[:, 0], a[:, 1], a[:, 6], a[:, 7] = [np.array(c, dtype=np.float32) for c in zip(*rows)]
    part, m = ob.partition(a)
    view = rr.make_view((0.0, 0.0), (0.0, 0.0), 1.0, 8, 4, 100.0)
    sim = pipeline(part, m)
    want = rr.counts(part, view)
    assert want[2].any() and want[0].any() and want[1].any()      # an off-screen core disc, a massless disc and points all show
    assert np.array_equal(sim.render_counts(view), want) and np.array_equal(host(part, view)[0], want)
    assert sim.bounds().tobytes() == rr.bounds(part).tobytes() == host(part, view)[2].tobytes()
    sim.close()
    # N = 0: an all-zero count image, a background frame, empty bounds
    sim = nb.SimPipeline(0, 0)
    sim.set_data(np.zeros((0, 8), dtype=np.float32))
    assert not sim.render_counts(view).any() and sim.bounds().tolist() == [np.inf, np.inf, -np.inf, -np.inf]
    bg = np.array(list(nb.default_palette().background), dtype=np.uint8)
    assert np.array_equal(sim.render(view), np.broadcast_to(bg, (4, 8, 4)))
    sim.close()


def test_world_renders_on_the_device_and_a_twin_that_never_rendered_ends_the_same(golden):
    ic = golden("ic_4096.bin")
    w, twin = nb.World(ic), nb.World(ic)
    frames = []
    for steps in (3, 20, 1):
        w.update_gpu(DT, steps)
        twin.update_gpu(DT, steps)
        view = w.fit_view(640, 360)                     # bounds on the device
        frames.append((view, w.bounds(), w.render_counts(view), w.render(view)))
        state = w.particles()                            # only now does the array come back
        assert state.tobytes() == twin.particles().tobytes()
        view_host = rr.fit_view(state, 640, 360)
        assert bytes(view) == bytes(view_host)
        cnt, img, b = host(state, view)
        assert frames[-1][1].tobytes() == b.tobytes() and np.array_equal(frames[-1][2], cnt) and np.array_equal(frames[-1][3], img)
        assert np.array_equal(cnt, rr.counts(state, view))
    # after a CPU step the host array is newer: the host path answers, and still equals the restatement
    w.update_cpu(DT, 1)
    twin.update_cpu(DT, 1)
    view = w.fit_view(640, 360)
    assert np.array_equal(w.render_counts(view), rr.counts(w.particles(), view))
    assert w.particles().tobytes() == twin.particles().tobytes()
    w.close()
    twin.close()


def test_nothing_observable_moves(golden):
    part, m = ob.partition(golden("ic_4096.bin"))
    sim, twin = pipeline(part, m, graph=1), pipeline(part, m, graph=1)
    view = rr.mixed_view(part)
    for s in (sim, twin):
        s.update(20, DT)
        s.update(20, DT)              # the cached 20-step chain, replayed
    stats, last = sim.graph_stats(), sim.last_step_ms()
    sim.bounds()
    sim.render_counts(view)
    sim.render(view)
    assert sim.graph_stats() == stats and sim.last_step_ms() == last
    assert sim.last_render_ms()[0] > 0.0
    for s in (sim, twin):
        s.update(20, DT)
        s.update(3, 0.02)
    assert sim.graph_stats() == twin.graph_stats()
    assert sim.get_data().tobytes() == twin.get_data().tobytes()
    sim.close()
    twin.close()


def test_render_behind_async_steps_sees_the_stepped_state(golden):
    part, m = ob.partition(golden("ic_1024.bin"))
    view = rr.fit_view(part, 320, 200)
    a, b = pipeline(part, m), pipeline(part, m)
    a.step_async(7, DT)
    got = a.render_counts(view), a.render(view), a.bounds()      # no explicit sync
    b.step_async(7, DT)
    b.sync()
    want = b.render_counts(view), b.render(view), b.bounds()
    state = b.get_data()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
    assert np.array_equal(got[0], rr.counts(state, view)) and a.get_data().tobytes() == state.tobytes()
    a.close()
    b.close()


def test_same_call_twice_and_regrowing_buffers(golden):
    part, m = ob.partition(golden("ic_4096.bin"))
    sim = pipeline(part, m)
    small, large = rr.fit_view(part, 64, 48), rr.mixed_view(part, 1920, 1080)
    first = {}
    for name, view in (("small", small), ("large", large), ("small", small), ("large", large), ("large", large), ("small", small)):
        got = sim.render_counts(view).tobytes(), sim.render(view).tobytes()
        assert first.setdefault(name, got) == got, name
    assert np.array_equal(np.frombuffer(first["large"][0], dtype=np.uint32).reshape(3, 1080, 1920), rr.counts(part, large))
    sim.configure(render_detail=1)
    sim.render(large)
    total, parts = sim.last_render_ms()
    assert total > 0.0 and all(p >= 0.0 for p in parts) and abs(sum(parts[1:]) - total) <= 0.05 * total + 0.01
    sim.close()
