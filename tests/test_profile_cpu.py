"""Radial profiles (include/nbody_profile.h, include/nbody_batch_profile.h) without a GPU: the host path bit for bit the numpy
model of the statement and of its summation order (profile_ref.py), the row rule at its edges, non-finite state, the teeth of
the checker against five defective restatements, an analytic rotating and expanding disc, a seeded galaxy through the numpy
helpers, every abort with its message, the host dispatch of World / WorldBatch with every GPU hidden, and the static facts of
profile.hip's kernels."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
import profile_ref as pr
from isa_common import compile_isa, kernel_meta
from test_abi import declared_functions, exported

ROOT = nb.ROOT
HIDDEN = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")


def child(code, **env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **HIDDEN)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def host_profile(a, edges, centre, weights):
    """(rows, unplaced, partitioned particles, mass_len) of a CPU-only World."""
    w = nb.World(a)
    p = w.particles()
    out, lost = w.profile(edges, centre[0:2], centre[2:4], weights={pr.BY_MASS: "mass", pr.BY_NUMBER: "number"}[weights], return_unplaced=True)
    w.close()
    return out, lost, p, int(np.count_nonzero(p[:, 6] > 0))


# ---- the host path is the model, bit for bit ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", pr.SIZES)
def test_host_path_is_bitwise_the_model(n):
    for mass_len, bins, weights in pr.grid(n):
        a, edges = pr.world(n, mass_len, seed=n + mass_len), pr.log_edges(bins)
        got, lost, p, m = host_profile(a, edges, pr.CENTRE, weights)
        assert m == mass_len and got.shape == (bins + 2, 6) and got.dtype == np.float64
        want, want_lost = pr.model(p, m, edges, pr.CENTRE, weights)
        assert pr.same(got, want) and lost == want_lost == 0, (n, mass_len, bins, weights)
        read = m if weights == pr.BY_MASS else n
        assert got[:, 0].sum() == read - lost          # counts: every particle read is in exactly one row
        if weights == pr.BY_NUMBER:
            assert np.array_equal(got[:, 0], got[:, 1])          # S of weight 1 is the count


@pytest.mark.parametrize("name", list(pr.edge_case_worlds()))
def test_edge_placements_and_non_finite_state(name):
    a, mass_len, edges, centre, weights = pr.edge_case_worlds()[name]
    got, lost, p, m = host_profile(a, edges, centre, weights)
    want, want_lost = pr.model(p, m, edges, centre, weights)
    assert m == mass_len and pr.same(got, want) and lost == want_lost, name
    read = m if weights == pr.BY_MASS else a.shape[0]
    assert got[:, 0].sum() == read - lost
    bins = len(edges) - 1
    if name == "on an edge":
        q, _ = pr.terms(p[:m], centre, np.ones(m))
        hit = {float(v) for v in q} & {1.5 ** 2, 2.5 ** 2}
        assert hit == {2.25, 6.25}          # both particles sit exactly on e2[1] and e2[2] ...
        below, _ = pr.model(p, m, edges, centre, weights, variant="edge_swapped")
        assert got[3, 0] == below[3, 0] + 1 and got[2, 0] == below[2, 0] and got[1, 0] == below[1, 0] - 1          # ... and count in the bin ABOVE it
    if name == "centre on a particle, edges[0] = 0":
        assert got[0, 0] == 0 and got[1, 0] >= 1          # q = 0 is not < e2[0] = 0: row 1
    if name == "all in one row":
        assert got[1, 0] == a.shape[0] and not got[[0, 2], :].any()
    if name == "all beyond the last edge":
        assert got[bins + 1, 0] == m and not got[:bins + 1, :].any()
    if name == "NaN and inf positions":
        assert lost == 3 and got[bins + 1, 0] >= 2 and np.isinf(got[bins + 1, 2])          # I of the last row holds q = +inf
    if name == "inf velocity of a placed particle":
        assert lost == 0 and not np.all(np.isfinite(got[:, 3:6])) and np.all(np.isfinite(got[:, 0:3]))
    if name == "massless rows of NaN":
        clean = a.copy()
        clean[300:, 0:6] = 0.0
        other, other_lost, _, _ = host_profile(clean, edges, centre, weights)
        assert got.tobytes() == other.tobytes() and lost == other_lost == 0 and np.all(np.isfinite(got))
        _, lost_by_number, _, _ = host_profile(a, edges, centre, pr.BY_NUMBER)
        assert lost_by_number == 300          # ... and by number they are read, and lie in no row


def test_the_checker_rejects_every_defective_variant():
    """Each defective restatement differs from the host path on a world made to show it, and the checker says so."""
    e = pr.log_edges(12, 0.5, 30.0)
    on_edge = pr.world(64, 64, seed=21)
    on_edge[11, 0:2] = (float(e[4]), 0.0)
    witnesses = {
        "edge_swapped": (on_edge, 64, (0, 0, 0, 0)),
        "chunk_1000": (pr.world(2049, 2049, seed=22), 2049, pr.CENTRE),
        "pairwise": (pr.world(1024, 1024, seed=23), 1024, pr.CENTRE),
        "reads_massless": (pr.world(300, 150, seed=24), 150, pr.CENTRE),
        "fused": (pr.world(1024, 1024, seed=25), 1024, pr.CENTRE),
    }
    assert set(witnesses) == set(pr.VARIANTS)
    for variant, (a, mass_len, centre) in witnesses.items():
        got, lost, p, m = host_profile(a, e, centre, pr.BY_MASS)
        assert m == mass_len and pr.same(got, pr.model(p, m, e, centre)[0]), variant
        assert not pr.same(got, pr.model(p, m, e, centre, variant=variant)[0]), variant
    # and the checker itself: a zero's sign and one ulp count, a NaN's sign does not, a NaN against a number does
    z = np.zeros((3, 6))
    assert pr.same(z, z) and not pr.same(z, -z) and not pr.same(z + 1.0, np.nextafter(z + 1.0, 2.0))
    nan = np.full((3, 6), np.nan)
    assert pr.same(nan, -nan) and not pr.same(nan, z) and not pr.same(z + np.inf, z - np.inf)


# ---- what the moments mean -----------------------------------------------------------------------------------------------------

def test_rigid_rotation_plus_homologous_expansion_about_a_moving_centre():
    """v = u + Omega z x (r - c) + H (r - c): every populated row must give L / I = Omega and W / I = H, and no dispersion.  The
    velocities are stored in float32 (2^-24 relative per component), hence the 1e-6 of the stated scale."""
    omega, hubble = 0.37, -0.11
    c, u = np.array([12.5, -3.25]), np.array([4.0, 7.5])
    rng = np.random.default_rng(31)
    a = np.zeros((3000, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((3000, 2)) * 20.0 + c
    a[:, 6] = 0.5 + rng.random(3000)
    a[:, 7] = 1.0
    d = a[:, 0:2].astype(np.float64) - c          # from the STORED positions
    a[:, 2:4] = u + omega * np.stack([-d[:, 1], d[:, 0]], axis=1) + hubble * d
    edges = nb.profile_edges(0.5, 60.0, 24, log=True)
    w = nb.World(a)
    rows = w.profile(edges, centre=c, centre_velocity=u)
    w.close()
    used = rows[:, 0] > 0
    assert used.sum() >= 20
    S, I, L, W, K = (rows[used, i] for i in range(1, 6))
    scale = abs(omega) + abs(hubble) + np.linalg.norm(u) / float(edges[1])
    worst_rate = max(np.max(np.abs(L / I - omega)), np.max(np.abs(W / I - hubble)))
    worst_disp = np.max((K - L * L / I - W * W / I) / K)
    print(f"[profile analytic] worst |rate error| {worst_rate:.3e} of the bound {1e-6 * scale:.3e}; worst dispersion / K {worst_disp:.3e}")
    assert worst_rate <= 1e-6 * scale
    assert np.all(K - L * L / I - W * W / I <= 1e-6 * K)
    curves = nb.profile_curves(rows, edges)
    inner = curves["omega"][np.isfinite(curves["omega"])]
    assert np.allclose(inner, omega, rtol=0, atol=1e-6 * scale) and np.all(curves["sigma2"][np.isfinite(curves["sigma2"])] <= 1e-6 * np.max(K / S))


def test_a_seeded_galaxy_about_its_core():
    ic = nb.make_galaxies(4000, 1, seed=4242, own_rng=True)          # MakeGalaxiesSeeded: the libc-independent stream
    w = nb.World(ic)
    p = w.particles()
    core = int(np.argmax(p[:, 6]))
    c, u = p[core, 0:2], p[core, 2:4]
    r = np.hypot(*(p[:, 0:2] - c).T.astype(np.float64))
    edges = nb.profile_edges(float(np.percentile(r[r > 0], 2)), float(np.percentile(r, 98)), 32, log=True)
    rows, lost = w.profile(edges, centre=c, centre_velocity=u, weights="number", return_unplaced=True)
    w.close()
    assert lost == 0 and rows[:, 0].sum() == 4000 and rows[0, 0] >= 1          # the core itself lies inside edges[0]
    curves = nb.profile_curves(rows, edges)
    assert set(curves) == {"r_mid", "area", "surface_density", "enclosed", "r_rms", "omega", "v_rot", "expansion", "v_rad", "sigma2"}
    assert np.all(np.diff(curves["enclosed"]) >= 0) and curves["enclosed"][-1] == rows[:-1, 1].sum()
    used = rows[1:-1, 0] > 0
    assert used.sum() >= 16
    for key, v in curves.items():
        assert v.shape == (32,) and np.all(np.isfinite(v[used])), key
        if key not in ("r_mid", "area", "enclosed"):
            assert np.all(np.isnan(v[~used])), key
    assert np.all((curves["r_rms"][used] >= edges[:-1][used]) & (curves["r_rms"][used] <= edges[1:][used]))
    fractions = np.array([0.1, 0.25, 0.5, 0.75, 0.9])
    radii = nb.lagrangian_radii(rows, edges, fractions)
    assert np.all(np.isfinite(radii)) and np.all(np.diff(radii) > 0)
    inside = np.cumsum(rows[:-1, 1])          # S within edges[t]
    for f, rad in zip(fractions, radii):
        t = int(np.searchsorted(edges, rad, side="left"))          # edges[t - 1] < rad <= edges[t]
        assert 1 <= t <= 32 and inside[t - 1] <= f * 4000 <= inside[t], (f, rad)
    true = np.sort(r)[(fractions * 4000).astype(int)]          # the real radii lie in the same or a neighbouring bin
    assert np.all(np.abs(np.searchsorted(edges, true) - np.searchsorted(edges, radii)) <= 1)
    assert np.isnan(nb.lagrangian_radii(rows, edges, 1e-9)) and np.isnan(nb.lagrangian_radii(rows, edges, 1.0))


def test_profile_edges_and_the_helpers_reject_what_they_cannot_use():
    e = nb.profile_edges(0.0, 8.0, 4)
    assert e.dtype == np.float32 and np.array_equal(e, [0, 2, 4, 6, 8])
    g = nb.profile_edges(1.0, 16.0, 4, log=True)
    assert np.allclose(g, [1, 2, 4, 8, 16]) and g.dtype == np.float32
    for bad in (dict(r_min=0.0, r_max=1.0, bins=0), dict(r_min=0.0, r_max=1.0, bins=255), dict(r_min=2.0, r_max=1.0, bins=4),
                dict(r_min=0.0, r_max=1.0, bins=4, log=True), dict(r_min=1.0, r_max=1.0 + 1e-7, bins=64)):
        with pytest.raises(ValueError):
            nb.profile_edges(**bad)
    with pytest.raises(ValueError):
        nb.profile_curves(np.zeros((5, 6)), e)
    with pytest.raises(ValueError):
        nb.lagrangian_radii(np.zeros((6, 5)), e, 0.5)
    rows = np.zeros((6, 6))
    rows[2] = (4, 8.0, 8 * 9.0, 8 * 9.0 * 0.5, 0.0, 8 * 9.0 * 0.25 + 2.0)          # S = 8 at r_rms = 3, omega = 0.5, K = I omega^2 + 2
    rows[4] = (1, 8.0, 8 * 49.0, 0.0, 8 * 49.0 * 0.25, 8 * 49.0 * 0.0625)        # pure expansion, no dispersion
    c = nb.profile_curves(rows, e)
    assert c["surface_density"][1] == 8.0 / (np.pi * 12.0) and c["r_rms"][1] == 3.0 and c["omega"][1] == 0.5 and c["v_rot"][1] == 1.5
    assert c["sigma2"][1] == 0.25 and c["expansion"][3] == 0.25 and c["v_rad"][3] == 1.75 and c["sigma2"][3] == 0.0
    assert np.array_equal(c["enclosed"], [0, 8, 8, 16]) and np.isnan(c["omega"][0]) and np.isnan(c["sigma2"][2])
    assert nb.lagrangian_radii(rows, e, 0.25) == np.sqrt(4.0 + 0.5 * 12.0)          # half of the first bin's mass: linear in r^2
    assert np.array_equal(nb.lagrangian_radii(rows, e, [0.5, 1.0]), [4.0, 8.0])


# ---- ensembles on the host ---------------------------------------------------------------------------------------------------

def test_a_batch_that_never_stepped_answers_on_the_host_with_the_bits_of_each_member_alone():
    edges = pr.log_edges(9, 0.5, 30.0)
    members = [pr.world(n, m, seed=40 + n) for n, m in ((1, 1), (333, 0), (1025, 1025), (700, 350))]
    members[3][5, 0] = np.nan
    centres = np.array([[0.0, 0.0], [1.0, -1.0], [0.3, -0.2], [5.0, 5.0]], dtype=np.float32)
    wb = nb.WorldBatch.ragged(members)
    for weights in ("mass", "number"):
        got, lost = wb.profile(edges, centre=centres, centre_velocity=(0.5, 0.25), weights=weights, return_unplaced=True)
        assert got.shape == (4, 11, 6) and lost.dtype == np.uint32 and list(lost) == [0, 0, 0, 1]
        for b, a in enumerate(members):
            w = nb.World(a)
            alone, alone_lost = w.profile(edges, centre=centres[b], centre_velocity=(0.5, 0.25), weights=weights, return_unplaced=True)
            w.close()
            assert pr.same(got[b], alone) and lost[b] == alone_lost, (weights, b)
        shared = wb.profile(edges, centre=centres[2], weights=weights)
        assert pr.same(shared, wb.profile(edges, centre=np.stack([centres[2]] * 4), weights=weights))
    assert not wb.profile(edges)[1].any()          # M = 0 in mass mode: +0 everywhere
    wb.close()
    uniform = nb.WorldBatch(np.stack([pr.world(250, 100, seed=s) for s in range(3)]))
    assert uniform.profile(edges).shape == (3, 11, 6) and uniform.profile(edges)[:, :, 0].sum() == 300
    uniform.close()


def test_cpu_only_worlds_and_batches_never_open_a_device():
    code = ("import os, numpy as np, nbody_amd as nb, profile_ref as pr\n"
            "a = pr.world(1500, 700, seed=1); e = pr.log_edges(16)\n"
            "w = nb.World(a); w.update_cpu(0.01, 2); r = w.profile(e, centre=(0.3, -0.2)); p = w.particles(); w.close()\n"
            "ok = pr.same(r, pr.model(p, 700, e, (0.3, -0.2, 0, 0))[0])\n"
            "wb = nb.WorldBatch(np.stack([a, a])); rb = wb.profile(e, weights='number'); wb.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', ok, r.shape, rb.shape, float(rb[:, :, 0].sum()))\n")
    r = child(code)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "OK True (18, 6) (2, 18, 6) 3000.0"


# ---- argument checks -----------------------------------------------------------------------------------------------------------

SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
         "w = nb.World(a); wb = nb.WorldBatch(np.stack([a, a, a])); L = nb.nbody_lib(); H = nb.hip_lib()\n"
         "e = np.array([0, 1, 2, 3], dtype=np.float32); c = np.zeros(4, dtype=np.float32); c3 = np.zeros((3, 4), dtype=np.float32)\n"
         "out = np.zeros(4096, dtype=np.float64); big = np.arange(300, dtype=np.float32)\n"
         "s = nb.SimPipeline(4, 4); sb = nb.SimBatch(4, [4, 4, 4])\n"
         "def spec(edges=e, bins=3, centre=(0, 0), vel=(0, 0), weights=0, n=1):\n"
         "    sp = (nb.WorldProfileSpec * n)()\n"
         "    for x in sp:\n"
         "        x.edges, x.bins, x.weights = (edges.ctypes.data if edges is not None else None), bins, weights\n"
         "        x.centre[0], x.centre[1], x.centre_velocity[0], x.centre_velocity[1] = centre[0], centre[1], vel[0], vel[1]\n"
         "    return sp\n")
SHARDED = "fn = nb.ALLGATHER_FN(lambda *x: None); ws = L.CreateWorldShardedWith(a.ctypes.data, 4, 0, 2, fn, None); "
BINS_MSG, FINITE, NEGATIVE, RISING = "bins must be 1 .. 254", "edges must be finite", "edges must not be negative", "edges must be strictly increasing"
CENTRE_MSG, WEIGHTS_MSG = "centre and centre velocity must be finite", "weights must be NB_PROFILE_BY_MASS or NB_PROFILE_BY_NUMBER"
ABORTS = [
    # the World layer
    ("world NULL world", "L.GetWorldProfile(None, spec(), out.ctypes.data, None)", "NULL argument"),
    ("world NULL spec", "L.GetWorldProfile(w._h, None, out.ctypes.data, None)", "NULL argument"),
    ("world NULL edges", "L.GetWorldProfile(w._h, spec(edges=None), out.ctypes.data, None)", "NULL argument"),
    ("world NULL out", "L.GetWorldProfile(w._h, spec(), None, None)", "NULL argument"),
    ("world bins 0", "L.GetWorldProfile(w._h, spec(bins=0), out.ctypes.data, None)", BINS_MSG),
    ("world bins 255", "L.GetWorldProfile(w._h, spec(edges=big, bins=255), out.ctypes.data, None)", BINS_MSG),
    ("world edge inf", "e[3] = np.inf; w.profile(e)", FINITE),
    ("world edge NaN", "e[1] = np.nan; w.profile(e)", FINITE),
    ("world edge negative", "e[0] = -0.5; w.profile(e)", NEGATIVE),
    ("world edges equal", "e[2] = e[1]; w.profile(e)", RISING),
    ("world edges falling", "w.profile(e[::-1].copy())", RISING),
    ("world centre NaN", "w.profile(e, centre=(np.nan, 0))", CENTRE_MSG),
    ("world centre velocity inf", "w.profile(e, centre_velocity=(0, np.inf))", CENTRE_MSG),
    ("world weights 2", "w.profile(e, weights=2)", WEIGHTS_MSG),
    ("sharded world", SHARDED + "L.GetWorldProfile(ws, spec(), out.ctypes.data, None)", "GetWorldProfile of a sharded pipeline needs a collective"),
    # the batch layer
    ("batch NULL batch", "L.GetWorldBatchProfile(None, spec(), 1, out.ctypes.data, None)", "NULL argument"),
    ("batch NULL specs", "L.GetWorldBatchProfile(wb._h, None, 1, out.ctypes.data, None)", "NULL argument"),
    ("batch NULL out", "L.GetWorldBatchProfile(wb._h, spec(), 1, None, None)", "NULL argument"),
    ("batch two specs for three members", "L.GetWorldBatchProfile(wb._h, spec(n=2), 2, out.ctypes.data, None)", "2 specs for 3 members"),
    ("batch per-member edges", "sp = spec(n=3); e2 = e * 2; sp[1].edges = e2.ctypes.data; L.GetWorldBatchProfile(wb._h, sp, 3, out.ctypes.data, None)",
     "the spec of member 1 differs from member 0's"),
    ("batch per-member weights", "sp = spec(n=3); sp[2].weights = 1; L.GetWorldBatchProfile(wb._h, sp, 3, out.ctypes.data, None)",
     "the spec of member 2 differs from member 0's"),
    ("batch bins 0", "L.GetWorldBatchProfile(wb._h, spec(bins=0), 1, out.ctypes.data, None)", BINS_MSG),
    ("batch edges equal", "e[2] = e[1]; wb.profile(e)", RISING),
    ("batch centre of member 1 NaN", "wb.profile(e, centre=[[0, 0], [0, np.nan], [0, 0]])", CENTRE_MSG),
    ("batch weights 7", "wb.profile(e, weights=7)", WEIGHTS_MSG),
    # the seam: every check comes before any device touch (no device is visible to these children)
    ("seam NULL pipeline", "H.nb_hip_profile(None, e.ctypes.data, 3, c.ctypes.data, 0, out.ctypes.data, None)", "NULL pipeline"),
    ("seam NULL edges", "H.nb_hip_profile(s._h, None, 3, c.ctypes.data, 0, out.ctypes.data, None)", "nb_hip_profile: NULL argument"),
    ("seam NULL centre", "H.nb_hip_profile(s._h, e.ctypes.data, 3, None, 0, out.ctypes.data, None)", "nb_hip_profile: NULL argument"),
    ("seam NULL out", "H.nb_hip_profile(s._h, e.ctypes.data, 3, c.ctypes.data, 0, None, None)", "nb_hip_profile: NULL argument"),
    ("seam bins 0", "H.nb_hip_profile(s._h, e.ctypes.data, 0, c.ctypes.data, 0, out.ctypes.data, None)", BINS_MSG),
    ("seam bins 255", "H.nb_hip_profile(s._h, big.ctypes.data, 255, c.ctypes.data, 0, out.ctypes.data, None)", BINS_MSG),
    ("seam edge NaN", "e[2] = np.nan; s.profile(e)", FINITE),
    ("seam edge negative", "e[0] = -1; s.profile(e)", NEGATIVE),
    ("seam edges equal", "e[3] = e[2]; s.profile(e)", RISING),
    ("seam centre inf", "s.profile(e, centre=(np.inf, 0))", CENTRE_MSG),
    ("seam weights -1", "s.profile(e, weights=-1)", WEIGHTS_MSG),
    ("seam before set_data", "s.profile(e)", "nb_hip_profile before SetSimulationData"),
    ("ensemble NULL ensemble", "H.nb_hip_ensemble_profile(None, e.ctypes.data, 3, c3.ctypes.data, 0, out.ctypes.data, None)", "NULL ensemble"),
    ("ensemble NULL centres", "H.nb_hip_ensemble_profile(sb._h, e.ctypes.data, 3, None, 0, out.ctypes.data, None)",
     "nb_hip_ensemble_profile: NULL argument"),
    ("ensemble bins 255", "H.nb_hip_ensemble_profile(sb._h, big.ctypes.data, 255, c3.ctypes.data, 0, out.ctypes.data, None)", BINS_MSG),
    ("ensemble edges falling", "sb.profile(e[::-1].copy())", RISING),
    ("ensemble centre of member 2 NaN", "sb.profile(e, centre_velocity=[[0, 0], [0, 0], [np.nan, 0]])", CENTRE_MSG),
    ("ensemble weights 2", "sb.profile(e, weights=2)", WEIGHTS_MSG),
    ("ensemble before set_data", "sb.profile(e)", "nb_hip_ensemble_profile before nb_hip_batch_set_data"),
    ("ragged ensemble before set_data", "nb.SimBatch.ragged([4, 9], [1, 2]).profile(e)", "nb_hip_ensemble_profile before nb_hip_batch_set_data"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


def test_python_argument_shapes_raise_before_the_library_is_called():
    w = nb.World(pr.world(8, 8))
    e = pr.log_edges(4)
    for bad in (dict(edges=[1.0]), dict(edges=e.reshape(1, -1)), dict(edges=e, centre=(0, 0, 0)), dict(edges=e, centre_velocity=[0]),
                dict(edges=e, weights="volume"), dict(edges=e, weights=None)):
        with pytest.raises(ValueError):
            w.profile(**bad)
    w.close()
    wb = nb.WorldBatch(np.stack([pr.world(8, 8)] * 3))
    with pytest.raises(ValueError):
        wb.profile(e, centre=np.zeros((2, 2)))
    wb.close()


# ---- sources, headers, exports -----------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_profile.h") == ["GetWorldProfile"] and declared_functions("nbody_batch_profile.h") == ["GetWorldBatchProfile"]
    funcs, seam = {"GetWorldProfile", "GetWorldBatchProfile"}, {"nb_hip_profile", "nb_hip_ensemble_profile"}
    assert funcs <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        have = exported(os.path.join(nb.LIB_DIR, so))
        assert funcs <= have and "nb_cpu_profile" not in have, so          # the host path is internal
    assert seam <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and seam <= exported(nb.HIP_SO) and not seam & set(nb.TUNE_API)
    assert nb.hip_lib().nb_hip_version() == 400          # no version bump: the new surface is detected by its symbols
    text = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert 'dlsym "nb_hip_profile"' in text and 'dlsym "nb_hip_ensemble_profile"' in text
    header = open(os.path.join(ROOT, "include", "nbody_profile.h")).read()
    for name, value in (("NB_PROFILE_MAX_BINS", nb.NB_PROFILE_MAX_BINS), ("NB_PROFILE_QTY", nb.NB_PROFILE_QTY), ("NB_PROFILE_CHUNK", nb.NB_PROFILE_CHUNK)):
        assert re.search(rf"#define {name} {value}u\b", header), name
    assert nb.NB_PROFILE_CHUNK == pr.CHUNK and nb.NB_PROFILE_QTY == pr.QTY
    assert "NB_PROFILE_BY_MASS = 0, NB_PROFILE_BY_NUMBER = 1" in header and (nb.NB_PROFILE_BY_MASS, nb.NB_PROFILE_BY_NUMBER) == (pr.BY_MASS, pr.BY_NUMBER)
    for cls in (nb.SimPipeline, nb.World, nb.SimBatch, nb.WorldBatch):
        assert callable(getattr(cls, "profile")), cls
    assert callable(nb.profile_edges) and callable(nb.profile_curves) and callable(nb.lagrangian_radii)
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\bprofile\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*\bprofile_cpu\.c", make, re.M)
    assert re.search(r"^\$\(OUT\)/%\.o:.*\$\(HERE\)profile_common\.h", make, re.M) and "-ffp-contract=off" in make
    # the statement is written once: neither path restates the terms or the row rule
    for source in ("profile.hip", "profile_cpu.c"):
        body = open(os.path.join(csrc, source)).read()
        assert '#include "profile_common.h"' in body and "nb_profile_terms(" in body and "nb_profile_row(" in body, source
        assert "dx * dx" not in body and "e2[mid]" not in body, source
    for h in ("nbody.h", "galaxy.h", "nbody_diag.h", "nbody_field.h", "nbody_tidal.h"):
        assert "Profile" not in open(os.path.join(ROOT, "include", h)).read(), h


# ---- static ISA of profile.hip ---------------------------------------------------------------------------------------------------

KERNELS = ("profile_chunk_kernel", "profile_reduce_kernel", "ensemble_profile_kernel")


@pytest.fixture(scope="module")
def profile_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("profile_isa"), "profile.hip")


def test_profile_hip_holds_three_kernels_without_scratch_within_their_launch_bounds(profile_isa):
    meta = kernel_meta(profile_isa)
    assert [sum(k in m[0] for m in meta) for k in KERNELS] == [1, 1, 1] and len(meta) == 3, [m[0] for m in meta]
    for name, scratch, sgpr, vgpr in meta:
        print(f"[profile isa] {name}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgpr <= 128, (name, vgpr)          # __launch_bounds__(256): four waves, one per SIMD, each may hold 512; 128 keeps four per SIMD
    assert re.findall(r"\.max_flat_workgroup_size:\s+(\d+)", profile_isa) == ["256"] * 3
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s+(\d+)", profile_isa)]
    assert len(lds) == 3 and all(0 < x <= 160 * 1024 // 3 for x in lds), lds          # at least three workgroups per CU


def test_profile_kernels_use_no_float_atomic(profile_isa):
    body = [line.split(";")[0].strip() for line in profile_isa.splitlines()]
    atomics = [ins for ins in body if re.match(r"(global_atomic|flat_atomic|buffer_atomic|ds_(add|sub|min|max|cmpst|wrxchg|pk_add)\w*)", ins)]
    assert atomics, "the NaN counter is an integer LDS atomic"
    for ins in atomics:
        assert not re.search(r"_(f16|bf16|f32|f64)\b", ins.split()[0]), ins
        assert ins.startswith("ds_add_u32"), ins
