"""The tidal tensor at probe points and as a map (include/nbody_tidal.h, include/nbody_batch_tidal.h) without a GPU: the host
path of GetWorldTidalAt / RenderWorldTidal and of the two WorldBatch calls against the float64 numpy restatement
(tests/tidal_ref.py), the analytic cases, the reference itself against central differences of g, the argument checks of all
eight C entry points, the header / binding / export agreement, static checks on the ISA of nbody_amd/csrc/tidal.hip, and the
numpy model of the device statement with the two defective variants its checkers must reject.  Every child process hides the
devices."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import nbody_amd as nb
import tidal_ref as tr
from gpu_common import synth
from isa_common import check_rsq_wait_states, compile_isa, functions, kernel_meta
from test_abi import declared_functions, exported
from test_gravity_cpu import loops
from tidal_ref import ulps_off

ROOT = nb.ROOT
WORLD_FUNCS = ["GetWorldTidalAt", "RenderWorldTidal"]
BATCH_FUNCS = ["GetWorldBatchTidalAt", "RenderWorldBatchTidal"]
HIP_FUNCS = ["nb_hip_tidal_at", "nb_hip_tidal_map", "nb_hip_ensemble_tidal_at", "nb_hip_ensemble_tidal_map"]
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")
HIDDEN = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
SOFT = 0.75


def child(code, **env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **HIDDEN)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def host_world(a):
    """A CPU-only World (never touches a device), its partitioned particles and its mass_len."""
    w = nb.World(a)
    p = w.particles()
    return w, p, int(np.count_nonzero(p[:, 6] > 0))


def within(got, want, mag):
    """Each component is a float64 sum rounded once to float32: half an ulp of the result (6e-8 relative), plus what the
    float64 sums themselves may lose where a diagonal component cancels (M additions of parts: 1e-12 of their sum covers
    M = 1e4 at 1.1e-16 each), plus 1e-30 for the exact zeros a component can be."""
    return np.all(np.abs(got.astype(np.float64) - want) <= 6e-8 * np.abs(want) + 1e-12 * mag + 1e-30)


def worst(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)))


def offset_view(width, height):
    return nb.RenderView.make((120.0, -40.0), (-3.5, -11.25), 0.37, width, height, 1.0)


def one_source(at=(3.0, -2.0), mass=1.0):
    a = np.zeros((1, 8), dtype=np.float32)
    a[0, 0:2], a[0, 6], a[0, 7] = at, mass, 0.25
    return a


# ---- the host path against float64 ---------------------------------------------------------------------------------------

def world_cases(golden):
    yield "ic_333", golden("ic_333.bin")
    yield "synthetic 3000", synth(3000, seed=21)[0]


def test_host_probes_and_map_match_f64(golden):
    for name, a in world_cases(golden):
        w, p, m = host_world(a)
        pts = tr.probes(p, 257, seed=3)
        pts[0] = p[0, 0:2]                          # a probe exactly on a source
        got = w.tidal_at(pts, SOFT)
        view = w.fit_view(19, 11)
        img = w.tidal_map(view, SOFT)
        before = w.particles().tobytes()
        w.close()
        assert got.dtype == np.float32 and got.shape == (257, 3) and before == p.tobytes(), name
        assert img.dtype == np.float32 and img.shape == (11, 19, 3), name
        want, mag = tr.t_at_f64(p, m, pts, SOFT)
        assert np.all(np.isfinite(got)) and within(got, want, mag), (name, worst(got, want))
        want_img, mag_img = tr.t_at_f64(p, m, tr.pixel_points(view), SOFT)
        assert within(img.reshape(-1, 3), want_img, mag_img), (name, worst(img.reshape(-1, 3), want_img))


def test_a_map_is_the_probes_product_at_the_pixel_centres_bit_for_bit(golden):
    w, p, m = host_world(golden("ic_333.bin"))
    for view in (w.fit_view(37, 7), offset_view(37, 7)):
        pts = tr.pixel_points(view)
        img = w.tidal_map(view, SOFT)
        assert img.dtype == np.float32 and img.shape == (7, 37, 3)
        assert img.tobytes() == w.tidal_at(pts, SOFT).tobytes()
    w.close()


def test_the_single_source_cases_are_the_analytic_ones():
    w, p, m = host_world(one_source())
    a = 4.0
    t = w.tidal_at([[3.0, -2.0], [3.0 + a, -2.0], [3.0, -2.0 - a]], SOFT)
    w.close()
    gm = float(np.float32(nb.NB_G) * np.float32(1.0))
    # on the source: the finite term diag(-G m s^-1.5), and the off-diagonal component is +0
    assert t[0, 1] == 0.0 and not np.signbit(t[0, 1])
    assert t[0, 0] == t[0, 2] and within(t[0, [0, 2]], np.full(2, -gm * SOFT ** -1.5), np.zeros(2))
    # at (a, 0) from it: xx = G m (3 a^2 u^5 - u^3), xy = 0, yy = -G m u^3
    u = (a * a + SOFT) ** -0.5
    assert t[1, 1] == 0.0 and within(t[1, [0, 2]], np.array([gm * (3 * a * a * u ** 5 - u ** 3), -gm * u ** 3]), np.zeros(2)), t[1]
    assert t[1, 0] > 0.0 > t[1, 2]                  # stretched along the line to the source, compressed across it
    # and at (0, -a): the same with x and y exchanged
    assert t[2, 0] == t[1, 2] and t[2, 2] == t[1, 0] and t[2, 1] == 0.0


def test_the_in_plane_trace_is_the_stated_sum_and_not_zero(golden):
    w, p, m = host_world(golden("ic_333.bin"))
    pts = tr.probes(p, 200, seed=8)
    t = w.tidal_at(pts, SOFT).astype(np.float64)
    w.close()
    x, y = p[:m, 0].astype(np.float64), p[:m, 1].astype(np.float64)
    gm = (np.float32(nb.NB_G) * p[:m, 6]).astype(np.float64)
    dx, dy = x[None, :] - pts[:, 0].astype(np.float64)[:, None], y[None, :] - pts[:, 1].astype(np.float64)[:, None]
    d2 = dx * dx + dy * dy
    q = d2 + SOFT
    trace = (gm[None, :] * q ** -2.5 * (d2 - 2.0 * SOFT)).sum(axis=1)
    _, mag = tr.t_at_f64(p, m, pts, SOFT)
    # two float32 roundings (xx and yy) of parts no larger than mag
    assert np.all(np.abs(t[:, 0] + t[:, 2] - trace) <= 6e-8 * (mag[:, 0] + mag[:, 2]))
    assert np.all(np.abs(trace) > 0.0) and np.allclose(nb.tidal_invariants(t)[0], t[:, 0] + t[:, 2], rtol=0, atol=0)


def test_exchanging_x_and_y_exchanges_xx_and_yy(golden):
    a = golden("ic_333.bin")
    b = a.copy()
    b[:, 0], b[:, 1] = a[:, 1], a[:, 0]
    wa, pa, m = host_world(a)
    wb, pb, mb = host_world(b)
    assert m == mb and np.array_equal(pa[:, 0], pb[:, 1])
    pts = tr.probes(pa, 100, seed=9)
    ta, tb = wa.tidal_at(pts, SOFT), wb.tidal_at(pts[:, ::-1], SOFT)
    wa.close()
    wb.close()
    assert ta[:, 0].tobytes() == tb[:, 2].tobytes() and ta[:, 2].tobytes() == tb[:, 0].tobytes() and ta[:, 1].tobytes() == tb[:, 1].tobytes()


def test_tidal_invariants_are_the_trace_and_the_eigenvalues():
    t = np.array([[2.0, 0.0, -1.0], [1.0, 2.0, 1.0], [-15.0, 0.0, -15.0]])
    trace, hi, lo = nb.tidal_invariants(t)
    assert trace.tolist() == [1.0, 2.0, -30.0] and hi.tolist() == [2.0, 3.0, -15.0] and lo.tolist() == [-1.0, -1.0, -15.0]
    assert nb.tidal_invariants(np.zeros((4, 5, 3), np.float32))[1].shape == (4, 5)
    with pytest.raises(ValueError):
        nb.tidal_invariants(np.zeros((4, 2)))


# ---- the reference against central differences of g ---------------------------------------------------------------------------

def test_the_reference_is_the_derivative_of_g(golden):
    """T = dg/dp of tidal_ref against (g(p + h e_b) - g(p - h e_b)) / 2h in float64 at float64 points, h = 2^-10 sqrt(s).
    The allowance is the truncation term h^2 / 6 |d^3 g_a / dp_b^3|.  With u' = d u^3 (u = q^(-1/2)) the third derivative of
    one source's g_a = G m d_a u^3 along b is
        G m u^5 (9 delta_ab - 45 delta_ab x^2 - 45 x y + 105 x^3 y),   x = d_b u, y = d_a u (y = x where a = b),
    and u^5 = u^3 (1 - r^2) / s with r^2 = |d|^2 u^2 < 1, so it is G m u^3 / s times (1 - r^2) (9 - 90 x^2 + 105 x^4) for
    a = b, which is largest at d = 0 (9; it falls to -5.9 at x^2 = 3/7), or times (1 - x^2 - y^2) x y (105 x^2 - 45) for
    a != b, which stays below 3.6.  Hence h^2 / 6 |d^3 g| <= 1.5 (h^2 / s) G m u^3 at p; 2.5 also covers u^3 anywhere
    on [p - h, p + h] (a factor (1 + h / sqrt(s))^3 < 1.003) and the next term of the expansion.  1e-12 mag covers the float64
    roundoff of tidal_ref's own sums."""
    s = SOFT
    h = 2.0 ** -10 * np.sqrt(s)
    for name, a in world_cases(golden):
        w, p, m = host_world(a)
        w.close()
        pts = tr.probes(p, 150, seed=12)
        pts[0] = p[0, 0:2]
        t, mag = tr.t_at_f64(p, m, pts, s)
        p64 = pts.astype(np.float64)
        ex, ey = np.array([h, 0.0]), np.array([0.0, h])
        dgx = (tr.g_f64(p, m, p64 + ex, s) - tr.g_f64(p, m, p64 - ex, s)) / (2 * h)
        dgy = (tr.g_f64(p, m, p64 + ey, s) - tr.g_f64(p, m, p64 - ey, s)) / (2 * h)
        x, y = p[:m, 0].astype(np.float64), p[:m, 1].astype(np.float64)
        gm = (np.float32(nb.NB_G) * p[:m, 6]).astype(np.float64)
        q = (x[None, :] - p64[:, 0][:, None]) ** 2 + (y[None, :] - p64[:, 1][:, None]) ** 2 + s
        allow = 2.5 * (h * h / s) * (gm[None, :] * q ** -1.5).sum(axis=1)
        for c, fd in ((0, dgx[:, 0]), (1, dgy[:, 0]), (1, dgx[:, 1]), (2, dgy[:, 1])):
            err = np.abs(t[:, c] - fd)
            assert np.all(err <= allow + 1e-12 * mag[:, c]), (name, c, float(np.max(err / allow)))


# ---- invariances -----------------------------------------------------------------------------------------------------------

def test_a_world_of_massless_particles_only_has_no_tide():
    a = np.zeros((5, 8), dtype=np.float32)
    a[:, 0], a[:, 7] = np.arange(5), 0.5
    w, p, m = host_world(a)
    assert m == 0
    t = w.tidal_at(tr.probes(p, 40, seed=1), SOFT)
    img = w.tidal_map(w.fit_view(9, 4), SOFT)
    w.close()
    assert t.shape == (40, 3) and img.shape == (4, 9, 3)
    assert not t.view(np.uint32).any() and not img.view(np.uint32).any()          # three +0 everywhere


def test_a_non_finite_point_gives_nan_triples_and_no_points_give_an_empty_array(golden):
    w, p, m = host_world(golden("ic_333.bin"))
    pts = tr.probes(p, 6, seed=2)
    pts[1, 0], pts[3, 1], pts[4, 0] = np.nan, np.inf, -np.inf
    t = w.tidal_at(pts, SOFT)
    assert np.isnan(t).tolist() == [[b, b, b] for b in (False, True, False, True, True, False)]
    empty = w.tidal_at(np.zeros((0, 2), dtype=np.float32), SOFT)
    assert empty.shape == (0, 3) and empty.dtype == np.float32
    img = w.tidal_map(nb.RenderView.make((np.nan, 0.0), (0.0, 0.0), 1.0, 3, 2, 1.0), SOFT)
    w.close()
    assert img.shape == (2, 3, 3) and np.isnan(img).all()


def test_host_result_does_not_depend_on_the_thread_count():
    code = ("import sys, hashlib, numpy as np, nbody_amd as nb\n"
            "from gpu_common import synth\n"
            "from tidal_ref import probes\n"
            "w = nb.World(synth(3000, seed=11)[0]); p = w.particles(); h = hashlib.sha256()\n"
            "h.update(w.tidal_at(probes(p, 500, seed=4), 0.75).tobytes())\n"
            "h.update(w.tidal_map(w.fit_view(37, 7), 0.75).tobytes()); sys.stdout.write(h.hexdigest())\n")
    outs = []
    for threads in ("1", "7"):
        r = child(code, OMP_NUM_THREADS=threads)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1] and len(outs[0]) == 64


def test_cpu_only_worlds_and_batches_never_open_a_device():
    code = ("import os, numpy as np, nbody_amd as nb\n"
            "a = np.zeros((64, 8), dtype=np.float32); a[:, 0] = np.arange(64); a[:, 6] = 1; a[:, 7] = 1\n"
            "w = nb.World(a); w.update_cpu(0.01, 2)\n"
            "t = w.tidal_at([[-1.5, 2.0], [70.0, -3.0]], 0.5); img = w.tidal_map(w.fit_view(16, 4), 0.5)\n"
            "e = w.tidal_at(np.zeros((0, 2), np.float32), 0.5); w.close()\n"
            "wb = nb.WorldBatch(np.stack([a, a])); v = nb.RenderView.make((8.0, 0.0), (4.0, 2.0), 0.5, 8, 4, 1.0)\n"
            "bt = wb.tidal_at([[-1.5, 2.0]], 0.5); bi = wb.tidal_map(v, 0.5); be = wb.tidal_at(np.zeros((0, 2), np.float32), 0.5); wb.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', bool(np.isfinite(t).all()), bool(np.isfinite(img).all()), img.shape, e.shape, bt.shape, bi.shape, be.shape)\n")
    r = child(code)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "OK True True (4, 16, 3) (0, 3) (2, 1, 3) (2, 4, 8, 3) (2, 0, 3)"


# ---- ensembles on the host: member b is nb.World(member b) -----------------------------------------------------------------------

def member(n, massive, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * 40.0
    a[:, 7] = 0.5 + rng.random(n)
    a[rng.permutation(n)[:massive], 6] = (10.0 + 990.0 * rng.random(massive)).astype(np.float32)
    return a


def uniform_batch():
    members = [member(7, m, seed=10 + m) for m in (3, 7, 5)]
    return nb.WorldBatch(np.stack(members)), members


def ragged_batch():
    members = [member(n, m, seed=20 + n) for n, m in ((1, 1), (4, 0), (9, 6))]          # one member without a source
    return nb.WorldBatch.ragged(members), members


@pytest.mark.parametrize("make", [uniform_batch, ragged_batch], ids=["uniform", "ragged"])
def test_a_batch_that_never_stepped_answers_on_the_host_with_the_bits_of_each_member_alone(make):
    wb, members = make()
    count = len(members)
    pts = (np.random.default_rng(1).standard_normal((count, 5, 2)) * 60.0).astype(np.float32)
    pts[0, 2] = members[0][0, 0:2]
    vs = [nb.RenderView.make((12.0 * b, -4.0 - b), (-3.5 + b, -1.25 * b), 0.37 + 0.11 * b, 6, 3, 1.0) for b in range(count)]
    at, img = wb.tidal_at(pts, SOFT), wb.tidal_map(vs, SOFT)
    assert at.shape == (count, 5, 3) and img.shape == (count, 3, 6, 3) and at.dtype == img.dtype == np.float32
    for b in range(count):
        w = nb.World(members[b])
        assert at[b].tobytes() == w.tidal_at(pts[b], SOFT).tobytes() and img[b].tobytes() == w.tidal_map(vs[b], SOFT).tobytes(), b
        w.close()
    # one point set or view for all members is that set given to each
    assert wb.tidal_at(pts[0], SOFT).tobytes() == wb.tidal_at(np.stack([pts[0]] * count), SOFT).tobytes()
    assert wb.tidal_map(vs[0], SOFT).tobytes() == wb.tidal_map([vs[0]] * count, SOFT).tobytes()
    if make is ragged_batch:
        assert not at[1].view(np.uint32).any() and not img[1].view(np.uint32).any()     # M = 0: +0
        bad = pts.copy()
        bad[1, 3, 1], bad[2, 0, 0] = np.inf, np.nan                                   # NaN whatever M
        t = wb.tidal_at(bad, SOFT)
        hit = np.zeros((count, 5), dtype=bool)
        hit[1, 3] = hit[2, 0] = True
        assert np.array_equal(np.isnan(t), np.repeat(hit[:, :, None], 3, axis=2)) and t[~hit].tobytes() == at[~hit].tobytes()
    wb.close()


# ---- argument checks -------------------------------------------------------------------------------------------------------

SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
         "w = nb.World(a); wb = nb.WorldBatch(np.stack([a, a, a])); L = nb.nbody_lib(); H = nb.hip_lib()\n"
         "pts = np.zeros((3, 2), dtype=np.float32); bpts = np.zeros((3, 2, 2), dtype=np.float32); out = np.zeros(256, dtype=np.float32)\n"
         "v = nb.RenderView.make((0.0, 0.0), (0.0, 0.0), 1.0, 4, 4, 1.0)\n"
         "vs = (nb.RenderView * 3)(v, v, v)\n"
         "s = nb.SimPipeline(4, 4); sb = nb.SimBatch(4, [4, 4, 4])\n")
SOFTENING = "softening must be finite and > 0"
SHARDED = "fn = nb.ALLGATHER_FN(lambda *x: None); ws = L.CreateWorldShardedWith(a.ctypes.data, 4, 0, 2, fn, None); "
BAD_SOFT = (("0", "0.0"), ("negative", "-1.0"), ("inf", "float('inf')"), ("NaN", "float('nan')"))
ABORTS = [(f"{who} {what} softening {name}", f"{who}.tidal_{what}({arg}, {value})", SOFTENING)
          for who, at, mp in (("w", "pts", "v"), ("wb", "bpts", "v")) for what, arg in (("at", at), ("map", mp)) for name, value in BAD_SOFT] + [
    ("zoom 0", "v.zoom = 0.0; L.RenderWorldTidal(w._h, v, 0.5, out.ctypes.data)", "zoom must be finite and > 0"),
    ("too many pixels", "v.width, v.height = 4097, 4096; L.RenderWorldTidal(w._h, v, 0.5, out.ctypes.data)", "must not exceed 2^24"),
    ("too many points", "L.GetWorldTidalAt(w._h, pts.ctypes.data, (1 << 24) + 1, 0.5, out.ctypes.data)", "at most 2^24 points"),
    ("NULL t", "L.GetWorldTidalAt(w._h, pts.ctypes.data, 3, 0.5, None)", "NULL argument"),
    ("NULL points", "L.GetWorldTidalAt(w._h, None, 3, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL world", "L.GetWorldTidalAt(None, pts.ctypes.data, 3, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL map", "L.RenderWorldTidal(w._h, v, 0.5, None)", "NULL argument"),
    ("NULL view", "L.RenderWorldTidal(w._h, None, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL map world", "L.RenderWorldTidal(None, v, 0.5, out.ctypes.data)", "NULL argument"),
    ("map before set_data", "s.tidal_map(v, 0.5)", "nb_hip_tidal_map before SetSimulationData"),
    ("probes before set_data", "s.tidal_at(pts, 0.5)", "nb_hip_tidal_at before SetSimulationData"),
    ("sharded world map", SHARDED + "L.RenderWorldTidal(ws, v, 0.5, out.ctypes.data)", "RenderWorldTidal of a sharded pipeline needs a collective"),
    ("sharded world probes", SHARDED + "L.GetWorldTidalAt(ws, pts.ctypes.data, 3, 0.5, out.ctypes.data)",
     "GetWorldTidalAt of a sharded pipeline needs a collective"),
    # the ensemble
    ("batch zoom 0", "vs[1].zoom = 0.0; L.RenderWorldBatchTidal(wb._h, vs, 0.5, out.ctypes.data)", "invalid RenderView of member 1 of 3"),
    ("batch views of differing size", "vs[2].width = 5; L.RenderWorldBatchTidal(wb._h, vs, 0.5, out.ctypes.data)",
     "invalid RenderView of member 2 of 3 (5 x 4, zoom 1): width and height differ from member 0's"),
    ("batch too many pixels in all", "vs[0].width = vs[1].width = vs[2].width = 2048; vs[0].height = vs[1].height = vs[2].height = 4096; "
                                     "L.RenderWorldBatchTidal(wb._h, vs, 0.5, out.ctypes.data)", "count * width * height must not exceed 2^24"),
    ("batch count * n over the limit", "L.GetWorldBatchTidalAt(wb._h, bpts.ctypes.data, (1 << 24) // 3 + 1, 0.5, out.ctypes.data)",
     "at most 2^24 points per call"),
    ("batch NULL batch", "L.GetWorldBatchTidalAt(None, bpts.ctypes.data, 2, 0.5, out.ctypes.data)", "NULL argument"),
    ("batch NULL points", "L.GetWorldBatchTidalAt(wb._h, None, 2, 0.5, out.ctypes.data)", "NULL argument"),
    ("batch NULL t", "L.GetWorldBatchTidalAt(wb._h, bpts.ctypes.data, 2, 0.5, None)", "NULL argument"),
    ("batch NULL views", "L.RenderWorldBatchTidal(wb._h, None, 0.5, out.ctypes.data)", "NULL argument"),
    ("batch NULL map", "L.RenderWorldBatchTidal(wb._h, vs, 0.5, None)", "NULL argument"),
    ("batch NULL map batch", "L.RenderWorldBatchTidal(None, vs, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL ensemble map", "H.nb_hip_ensemble_tidal_map(None, vs, 0.5, out.ctypes.data)", "NULL ensemble"),
    ("NULL ensemble probes", "H.nb_hip_ensemble_tidal_at(None, bpts.ctypes.data, 2, 0.5, out.ctypes.data)", "NULL ensemble"),
    ("ensemble probes before set_data", "sb.tidal_at(bpts, 0.5)", "nb_hip_ensemble_tidal_at before nb_hip_batch_set_data"),
    ("ensemble map before set_data", "sb.tidal_map(v, 0.5)", "nb_hip_ensemble_tidal_map before nb_hip_batch_set_data"),
    ("ragged ensemble before set_data", "nb.SimBatch.ragged([4, 9], [1, 2]).tidal_map(v, 0.5)",
     "nb_hip_ensemble_tidal_map before nb_hip_batch_set_data"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


# ---- sources, headers, exports -----------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_tidal.h") == WORLD_FUNCS and declared_functions("nbody_batch_tidal.h") == BATCH_FUNCS
    assert set(WORLD_FUNCS + BATCH_FUNCS) <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        have = exported(os.path.join(nb.LIB_DIR, so))
        assert set(WORLD_FUNCS + BATCH_FUNCS) <= have, so
        assert not {"nb_cpu_tidal_at", "nb_cpu_tidal_map"} & have, so          # the host path is internal
    assert set(HIP_FUNCS) <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and set(HIP_FUNCS) <= exported(nb.HIP_SO)
    assert not set(HIP_FUNCS) & set(nb.TUNE_API)
    assert nb.hip_lib().nb_hip_version() == 400      # no version bump: the new surface is detected by its symbols
    seam = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert 'dlsym "nb_hip_tidal_map"' in seam and 'dlsym "nb_hip_ensemble_tidal_map"' in seam
    assert "typedef struct { float xx, xy, yy; } TidalTensor;" in open(os.path.join(ROOT, "include", "nbody_tidal.h")).read()
    assert "not zero" in open(os.path.join(ROOT, "include", "nbody_tidal.h")).read().lower()          # the in-plane trace
    assert "ragged" in open(os.path.join(ROOT, "include", "nbody_batch_tidal.h")).read().lower()
    for cls in (nb.SimPipeline, nb.World, nb.SimBatch, nb.WorldBatch):
        assert callable(getattr(cls, "tidal_at")) and callable(getattr(cls, "tidal_map")), cls
    assert callable(nb.tidal_invariants)
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\btidal\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*\bfield_cpu\.c", make, re.M)
    for header in ("nbody_tidal.h", "nbody_batch_tidal.h"):
        assert re.search(r"^WORLD_HDRS\s*:=(?:.*\\\n)*.*include/" + re.escape(header), make, re.M), header
    for header in ("field_kernels.h", "field_sampler.h", "ensemble_sampler.h", "batch_field.h"):
        assert re.search(r"^\$\(OUT\)/%\.o:.*\$\(HERE\)" + re.escape(header), make, re.M), header
    assert re.search(r"^\$\(OUT\)/%\.o:(?:.*\\\n)*.*include/nbody_tidal\.h", make, re.M)
    # one sampler: the third policy sits beside the other two, and tidal.hip only instantiates
    shared = open(os.path.join(csrc, "field_kernels.h")).read()
    assert "struct Tidal" in shared and "static constexpr int OUT = 3" in shared
    text = open(os.path.join(csrc, "tidal.hip")).read()
    for name in ("struct Tidal", "__global__", "void load_samples(", "void slice_sum("):
        assert name not in text, name
    assert '#include "field_sampler.h"' in text and '#include "ensemble_sampler.h"' in text
    for key, where in (("tidal_shape", "nbody_hip_tuning.h"), ("tidal_shape", "pipeline.hip"), ("tidal_shape", "pipeline_internal.h")):
        assert key in open(os.path.join(csrc, where)).read(), where
    for h in ("nbody.h", "galaxy.h", "nbody_diag.h", "nbody_render.h", "nbody_field.h", "nbody_gravity.h", "nbody_batch_field.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert not [f for f in WORLD_FUNCS + BATCH_FUNCS + HIP_FUNCS if f in text], h


def test_the_tidal_shape_hook_takes_its_three_values_and_rejects_others():
    s = nb.SimPipeline(4, 4)
    tune = nb.hip_lib().nb_hip_tune
    assert [tune(s._h, b"tidal_shape", v) for v in (1, 2, 0)] == [0, 1, 2]          # returns the previous value
    s.close()
    r = child("import nbody_amd as nb\ns = nb.SimPipeline(4, 4); s.configure(tidal_shape=3)\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout and "tidal_shape must be 0 (auto), 1 (source split) or 2" in r.stderr


# ---- static ISA of tidal.hip -------------------------------------------------------------------------------------------------------

KERNELS = ("sample_split_kernel", "sample_wave_kernel", "ensemble_sample_kernel")
VGPR_MAX = 64          # __launch_bounds__(..., 8): eight waves per SIMD, in all three shapes


@pytest.fixture(scope="module")
def tidal_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("tidal_isa"), "tidal.hip")


def test_tidal_hip_holds_six_kernels_at_eight_waves_per_simd_without_scratch(tidal_isa):
    meta = kernel_meta(tidal_isa)
    assert [sum(k in m[0] for m in meta) for k in KERNELS] == [2, 2, 2] and len(meta) == 6, [m[0] for m in meta]    # probes / map each
    for name, scratch, sgpr, vgpr in meta:
        print(f"[tidal isa] {name}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs")
        assert "Tidal" in name and "Potential" not in name and "Acceleration" not in name, name
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgpr <= VGPR_MAX, (name, vgpr)


def test_tidal_kernels_keep_the_wait_state_behind_every_rsq(tidal_isa):
    fns = functions(tidal_isa)
    names = [n for n in fns if any(k in n for k in KERNELS)]
    assert len(names) == 6, sorted(fns)
    for name in names:
        assert check_rsq_wait_states(name, fns[name]) >= 2, name


def test_the_loop_of_every_kernel_holds_sixteen_rsq_per_eight_sources(tidal_isa):
    names = [name for name, *_ in kernel_meta(tidal_isa)]
    for name in names:
        fetch8 = [(lab, ops) for lab, ops in loops(tidal_isa, name) if "s_load_dwordx16" in ops]
        assert len(fetch8) == 1, (name, [lab for lab, _ in fetch8])
        ops = fetch8[0][1]
        rsq = sum(o.startswith("v_rsq_f32") for o in ops)
        valu = sum(o.startswith("v_") for o in ops) - rsq
        print(f"[tidal isa] {name}: 8-source loop of {len(ops)} instructions: {valu} VALU + {rsq} v_rsq_f32 "
              f"({valu / 16:.2f} VALU per pair)")
        assert rsq == 16, (name, ops)          # 8 sources x 2 samples per lane
        assert valu >= 16 * 14                 # the statement's 14 plain VALU instructions per pair, none folded away


# ---- the numpy model of the device statement, and its teeth ------------------------------------------------------------------------

def model_worlds(golden):
    """what tests/test_gpu_tidal.py holds the device to: a map of the 1024 fixture and one of synth(4096), and probes of small
    worlds across the block and slice edges"""
    import oracle_binding as ob
    import render_ref as rr
    part, m = ob.partition(golden("ic_1024.bin"))
    yield "ic_1024 32 x 32", part, m, tr.pixel_points(rr.fit_view(part, 32, 32))
    part, m = synth(4096, seed=4096)
    yield "synth(4096) 64 x 32", part, m, tr.pixel_points(rr.fit_view(part, 64, 32))
    for m in (7, 257, 4500):
        rng = np.random.default_rng(1000 + m)
        a = np.zeros((m, 8), dtype=np.float32)
        a[:, 0:2] = rng.standard_normal((m, 2)) * 1.0e3
        a[:, 6], a[:, 7] = 10.0 + 990.0 * rng.random(m), 1.0
        yield f"M = {m}", a, m, tr.probes(a, 300, seed=m)


def test_the_model_of_the_statement_stays_inside_the_tolerance(golden):
    """1e-4 |T| + 1e-6 mag, the bound tests/test_gpu_tidal.py holds the device to, with rsq correctly rounded and one ulp off
    either way.  Measured here: 0.60 - 0.69 on the 1024 fixture (a pixel beside a heavy source: one term, whose u^5 carries
    five times the error of u), 0.30 - 0.41 on synth(4096)."""
    for name, part, m, pts in model_worlds(golden):
        t64, mag = tr.t_at_f64(part, m, pts, SOFT)
        ratios = [tr.ratio_to_bound(tr.device_model(part, m, pts, SOFT, ulps), t64, mag) for ulps in (0, 1, -1)]
        print(f"[tidal model] {name}: worst error / bound {ratios[0]:.3f} (rsq exact), {ratios[1]:.3f} (+1 ulp), {ratios[2]:.3f} (-1 ulp)")
        assert max(ratios) <= 1.0, (name, ratios)


# On tidal_ref.exact_world every instruction of the documented statement is exact and one source, or two equal ones, are
# summed exactly: "the factor 3 and the cancellation happen in float64, each component rounded once" then means the
# correctly rounded value of an exactly known number -- here that number is itself a float32 (G*m / 32 and G*m / 8), so 0 ulp.
EXACT_MASSES = ([1.2345678], [0.7654321, 0.7654321], [3.3333333], [917.0001])


def exact_world_errors(variant):
    out = []
    for masses in EXACT_MASSES:
        got = tr.device_model(tr.exact_world(masses), len(masses), tr.exact_probe(), tr.EXACT_SOFT, 0, variant)[0]
        out.append(max(ulps_off(g, e) for g, e in zip(got, tr.exact_tensor(masses))))
    return out


# The summation witness (tests/sum_witness.py's pattern for the sampler): 65 536 sources at one point, one of them 2^33 times
# as heavy as the others, seen from exact_probe(): every term of A and D is exact, a block of 256 small terms is summed
# exactly and totals 2^-25 of the big term.  Documented scheme: the 255 small terms that share the big one's block are lost
# in its fp32 sum (under 2^-25 of the result: at most half an ulp), every other block total reaches the float64 sums whole,
# and the final rounding costs half an ulp: E = 1 ulp.  With fp32 totals the blocks that share the big term's slice are
# lost too, a quarter ulp of the big term each.
WITNESS_M = 65536
WITNESS_E = 1.0


def witness_errors(variant):
    out = []
    for at in (0, WITNESS_M // 2 + 100):
        masses = tr.witness_masses(WITNESS_M, at)
        got = tr.device_model(tr.exact_world(masses), WITNESS_M, tr.exact_probe(), tr.EXACT_SOFT, 0, variant)[0]
        out.append(max(ulps_off(g, e) for g, e in zip(got, tr.exact_tensor(masses))))
    return out


def test_the_checkers_pass_the_documented_scheme_and_reject_the_two_defective_ones():
    documented = exact_world_errors(None), witness_errors(None)
    print(f"[tidal model] documented: exact worlds {documented[0]} ulp, witness {documented[1]} ulp (E = {WITNESS_E})")
    assert max(documented[0]) == 0.0 and max(documented[1]) <= WITNESS_E
    merged = exact_world_errors("merged diagonal")
    print(f"[tidal model] merged diagonal: exact worlds {merged} ulp")
    assert min(merged) >= 1.0          # 3 * tx is rounded for every pair: caught on every one of these worlds
    totals = witness_errors("f32 totals")
    print(f"[tidal model] f32 totals: witness {totals} ulp")
    assert min(totals) > 2.0 * WITNESS_E
