"""Rendering an ensemble on the GPU (nb_hip_ensemble_bounds / _render_counts / _render_rgba, and the WorldBatch calls of
include/nbody_batch_render.h when the device holds the newest state): every member BITWISE against the host path (a
WorldBatch that never stepped, pinned to numpy by tests/test_batch_render_cpu.py) and against tests/render_ref.py, on the
tile path and on the global path, and that a render changes nothing a step, a read-back or a timer can observe.
No wall-clock assertions here."""
import numpy as np
import pytest

import nbody_amd as nb
import render_ref as rr
from batch_render_common import CUSTOM, KINDS, hand_made, make_view
from gpu_common import synth

pytestmark = pytest.mark.gpu

DT = 0.01
CASES = [(n, c) for n in (1, 64, 65, 250, 512, 513, 1000, 3000) for c in (1, 3, 64)] + [(250, 300)]


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if nb.device_count() < 1:
        pytest.skip("needs an MI355X")


def ensemble(n, count, seed=0):
    """count synthetic members of n particles: mixed, massless only, massive only, in turn"""
    made = [synth(n, (0.5, 0.0, 1.0)[b % 3], seed=seed + b) for b in range(count)]
    return np.stack([p for p, _ in made]), [m for _, m in made]


def batch_of(start, ms):
    s = nb.SimBatch(start.shape[1], ms)
    s.set_data(start)
    return s


def host(state, views, palette=None):
    wb = nb.WorldBatch(state)        # never stepped: the host path
    out = wb.bounds(), wb.render_counts(views), wb.render(views, palette)
    wb.close()
    return out


@pytest.fixture(scope="module")
def tiles():
    """1 x 1, 37 x 53, the last size on the tile path and the first on the global path (found from what the library reports,
    W x 64 with the shipped threshold at W = 64), and 320 x 200."""
    start, ms = ensemble(1, 1)
    s = batch_of(start, ms)

    def on_tile_path(w):
        s.render_counts(rr.fit_view(start[0], w, 64))
        return s.last_render_info()["tile_path"] == 1

    lo, hi = 1, 4096
    assert on_tile_path(lo) and not on_tile_path(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if on_tile_path(mid) else (lo, mid)
    s.close()
    return [(1, 1), (37, 53), (lo, 64), (hi, 64), (320, 200)]


PATHS = set()


def check_against_host(s, state, views, palette=None, direct=()):
    """bounds / counts / frames of the ensemble == the host path for ALL members, in both modes where the tile path applies;
    members in `direct` also against numpy.  Returns the count images; PATHS collects the paths that "auto" took."""
    want_b, want_c, want_f = host(state, views, palette)
    assert s.bounds().tobytes() == want_b.tobytes()
    got = s.render_counts(views)
    info = s.last_render_info()
    PATHS.add(info["tile_path"])
    assert np.array_equal(got, want_c), [b for b in range(s.count) if not np.array_equal(got[b], want_c[b])][:8]
    assert np.array_equal(s.render(views, palette), want_f)
    frame_info = s.last_render_info()
    assert frame_info["tile_path"] == info["tile_path"]
    if info["tile_path"]:
        assert info["launches"] == 1 and frame_info["launches"] == 1     # one launch per counts call, one per frame call
        s.render_mode(1)
        assert np.array_equal(s.render_counts(views), want_c) and s.last_render_info() == {"tile_path": 0, "launches": 3}
        assert np.array_equal(s.render(views, palette), want_f) and s.last_render_info() == {"tile_path": 0, "launches": 4}
        s.render_mode(0)
    else:
        assert info["launches"] == 3 and frame_info["launches"] == 4      # clear, splat, disc pass (+ shade): not per member
    per_member = [views] * s.count if isinstance(views, nb.RenderView) else views
    for b in direct:
        assert np.array_equal(got[b], rr.counts(state[b], per_member[b])), b
    return got


@pytest.mark.parametrize("n,count", CASES, ids=[f"N{n}-B{c}" for n, c in CASES])
def test_every_member_against_the_host_path(tiles, n, count):
    start, ms = ensemble(n, count, seed=n)
    s = batch_of(start, ms)
    direct = sorted({0, min(1, count - 1), min(2, count - 1), count - 1})
    PATHS.clear()
    for steps in (0, 1, 4):          # one step on the lane-split path: the latest state sits in the OTHER position buffer
        s.set_data(start)
        s.update(steps, DT)
        state = s.get_data()
        for width, height in tiles:
            if count * width * height > rr.MAX_PIXELS:       # 300 members: the largest tile one call may hold, still global
                width, height = 240, 200
            fitted = [rr.fit_view(p, width, height) for p in state]
            check_against_host(s, state, fitted, direct=direct)
            kinds = [KINDS[1 + b % 4] for b in range(count)]           # mixed / edge / collapsed / nothing, by member index
            cycling = [make_view(k, p, width, height) for k, p in zip(kinds, state)]
            got = check_against_host(s, state, cycling, nb.RenderPalette.make(**CUSTOM), direct=direct)
            for b, k in enumerate(kinds):
                if k == "collapsed":
                    assert int(got[b].sum()) == n == int(got[b][:, height // 2, width // 2].sum()), b
                if k == "nothing":
                    assert not got[b].any(), b
        assert s.get_data().tobytes() == state.tobytes()
    assert PATHS == {0, 1}
    s.close()


def test_hand_made_edges_and_non_finite_particles_as_one_member():
    hand, view = hand_made()
    n = hand.shape[0]
    state = np.stack([synth(n, 0.5, seed=3, extent=3.0)[0], hand, np.full((n, 8), np.nan, dtype=np.float32), synth(n, 1.0, seed=4, extent=3.0)[0]])
    s = batch_of(state, [int((p[:, 6] > 0).sum()) for p in state])
    got = check_against_host(s, state, view, direct=range(4))
    assert got[1][0].any() and got[1][1].any() and got[1][2].any() and not got[2].any()
    assert s.bounds()[2].tolist() == [np.inf, np.inf, -np.inf, -np.inf]
    big = rr.make_view((0.0, 0.0), (100.0, 100.0), 30.0, 320, 200, 100.0)       # the global path, every disc large
    check_against_host(s, state, big, direct=range(4))
    s.close()


@pytest.mark.parametrize("n", [250, 513])
def test_members_do_not_depend_on_each_other(tiles, n):
    start, ms = ensemble(n, 5, seed=40)
    s = batch_of(start, ms)
    order = [3, 0, 4, 1, 2]
    t = batch_of(start[order], [ms[b] for b in order])
    pair = batch_of(np.stack([start[3], start[3]]), [ms[3], ms[3]])
    crowd = batch_of(np.concatenate([start[3:4], ensemble(n, 8, seed=90)[0]]), [ms[3]] + ensemble(n, 8, seed=90)[1])
    for x in (s, t, pair, crowd):
        x.update(3, DT)
    state = s.get_data()
    for width, height in tiles[1:]:
        views = [make_view(KINDS[b % 5], p, width, height) for b, p in enumerate(state)]
        cnt, img, bounds = s.render_counts(views), s.render(views), s.bounds()
        permuted = [views[b] for b in order]
        assert np.array_equal(t.render_counts(permuted), cnt[order]) and np.array_equal(t.render(permuted), img[order])
        assert t.bounds().tobytes() == bounds[order].tobytes()
        for other in (pair, crowd):      # member 3 alone twice, and in front of eight strangers: the same image
            assert np.array_equal(other.render_counts(views[3])[0], cnt[3]) and np.array_equal(other.render(views[3])[0], img[3])
            assert other.bounds()[0].tobytes() == bounds[3].tobytes()
    for x in (s, t, pair, crowd):
        x.close()


@pytest.mark.parametrize("n", [250, 1000])
def test_a_member_equals_the_same_world_rendered_alone(tiles, n):
    start, ms = ensemble(n, 3, seed=7)
    s = batch_of(start, ms)
    s.update(3, DT)
    state = s.get_data()
    for width, height in tiles[1:]:
        views = [make_view(KINDS[b % 2], p, width, height) for b, p in enumerate(state)]      # fitted / mixed
        cnt, img, bounds = s.render_counts(views), s.render(views), s.bounds()
        for b in range(3):
            one = nb.SimPipeline(n, ms[b])
            one.set_data(state[b])
            assert np.array_equal(one.render_counts(views[b]), cnt[b]) and np.array_equal(one.render(views[b]), img[b])
            assert one.bounds().tobytes() == bounds[b].tobytes()
            one.close()
    s.close()


@pytest.mark.parametrize("n", [250, 1000])
def test_render_behind_async_steps_sees_the_stepped_state(tiles, n):
    start, ms = ensemble(n, 4, seed=11)
    dts = np.array([0.01, 0.02, 0.005, 0.01], dtype=np.float32)
    for width, height in (tiles[2], tiles[4]):
        views = [rr.fit_view(p, width, height) for p in start]
        a, b = batch_of(start, ms), batch_of(start, ms)
        a.step_async(7, dts)
        got = a.render_counts(views), a.render(views), a.bounds()       # no explicit sync
        b.step_async(7, dts)
        b.sync()
        want = b.render_counts(views), b.render(views), b.bounds()
        state = b.get_data()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        assert all(np.array_equal(got[0][m], rr.counts(state[m], views[m])) for m in range(4))
        assert a.get_data().tobytes() == state.tobytes() and not np.array_equal(state, start)
        a.close()
        b.close()


@pytest.mark.parametrize("n", [250, 1000])
def test_nothing_observable_moves(tiles, n):
    start, ms = ensemble(n, 6, seed=21)
    s, twin = batch_of(start, ms), batch_of(start, ms)
    dts = np.linspace(0.005, 0.02, 6).astype(np.float32)
    for i, (steps, dt) in enumerate(((3, DT), (1, dts), (4, DT), (2, 0.02))):
        for x in (s, twin):
            x.update(steps, dt)
        last, uploads = s.last_ms(), s.dt_uploads()
        width, height = tiles[1 + i]
        views = [rr.fit_view(p, width, height) for p in start]
        s.bounds()
        s.render_counts(views)
        s.render(views)
        assert s.last_render_ms() > 0.0
        assert s.last_ms() == last and s.dt_uploads() == uploads == twin.dt_uploads()
    assert twin.last_render_ms() == 0.0 and twin.last_render_info() == {"tile_path": 0, "launches": 0}
    assert s.get_data().tobytes() == twin.get_data().tobytes()
    s.close()
    twin.close()


def test_regrowing_buffers_and_a_larger_ensemble(tiles):
    start, ms = ensemble(250, 7, seed=31)
    s, larger = batch_of(start[:3], ms[:3]), batch_of(start, ms)
    small = [rr.fit_view(p, 37, 53) for p in start]
    large = [make_view("mixed", p, 320, 200) for p in start]
    first = {}
    for name, views in (("small", small), ("large", large), ("small", small), ("large", large), ("large", large), ("small", small)):
        got = s.render_counts(views[:3]).tobytes(), s.render(views[:3]).tobytes()
        assert first.setdefault(name, got) == got, name
    for name, views in (("large", large), ("small", small)):          # more views than any call before, in another ensemble
        got = larger.render_counts(views), larger.render(views)
        assert got[0][:3].tobytes() == first[name][0] and got[1][:3].tobytes() == first[name][1], name
    assert np.array_equal(np.frombuffer(first["large"][0], dtype=np.uint32).reshape(3, 3, 200, 320)[1], rr.counts(start[1], large[1]))
    s.close()
    larger.close()


@pytest.mark.parametrize("n", [250, 1000])
def test_world_batch_renders_on_the_device_and_a_twin_that_never_rendered_ends_the_same(tiles, n):
    start, _ = ensemble(n, 5, seed=51)
    rng = np.random.default_rng(1)
    start = np.stack([p[rng.permutation(n)] for p in start])         # caller order: CreateWorldBatch partitions
    wb, twin = nb.WorldBatch(start), nb.WorldBatch(start)
    # created, never stepped: the host path answers and equals numpy
    parts = [wb.member(b) for b in range(5)]
    views = wb.fit_views(37, 53)
    assert all(bytes(views[b]) == bytes(rr.fit_view(parts[b], 37, 53)) for b in range(5))
    assert all(np.array_equal(wb.render_counts(views)[b], rr.counts(parts[b], views[b])) for b in range(5))
    for steps, (width, height) in zip((3, 1, 4), (tiles[1], tiles[2], tiles[4])):
        wb.update_gpu(DT, steps)
        twin.update_gpu(DT, steps)
        views = wb.fit_views(width, height)                           # bounds on the device
        got = wb.bounds(), wb.render_counts(views), wb.render(views)
        state = wb.particles()                                        # only now does the array come back
        assert state.tobytes() == twin.particles().tobytes()
        assert all(bytes(views[b]) == bytes(rr.fit_view(state[b], width, height)) for b in range(5))
        want = host(state, views)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        assert np.array_equal(got[1][4], rr.counts(state[4], views[4]))
    wb.close()
    twin.close()
