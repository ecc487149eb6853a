"""The potential at probe points and as a map (include/nbody_field.h) without a GPU: the host path of GetWorldPotentialAt /
RenderWorldPotential against the float64 numpy restatement (tests/field_ref.py), the map = probes identity, the argument
checks, the header / binding / export agreement, and static checks on the ISA of nbody_amd/csrc/field.hip.  Every child
process hides the devices."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
from field_ref import augmented, phi_at_f64, pixel_points, probes
from gpu_common import synth
from isa_common import check_rsq_wait_states, compile_isa, functions, kernel_meta
from test_abi import declared_functions, exported

ROOT = nb.ROOT
WORLD_FUNCS = ["GetWorldPotentialAt", "RenderWorldPotential"]
HIP_FUNCS = ["nb_hip_potential_at", "nb_hip_potential_map"]
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


def within(got, want):
    """The bound tests/test_energy_cpu.py holds the host Phi to: the float64 sum rounded once to float32."""
    return np.all(np.abs(got.astype(np.float64) - want) <= 6e-8 * np.abs(want) + 1e-300)


def fitted(w, width, height):
    return w.fit_view(width, height)


def offset_view(width, height):
    return nb.RenderView.make((120.0, -40.0), (-3.5, -11.25), 0.37, width, height, 1.0)


# ---- the host path against float64 ---------------------------------------------------------------------------------------

def world_cases(golden):
    yield "ic_333", golden("ic_333.bin")
    yield "synthetic 3000", synth(3000, seed=21)[0]


def test_host_probes_match_f64(golden):
    for name, a in world_cases(golden):
        w, p, m = host_world(a)
        pts = probes(p, 257, seed=3)
        pts[0] = p[0, 0:2]                          # a probe exactly on a source
        got = w.potential_at(pts, SOFT)
        before = w.particles().tobytes()
        w.close()
        want = phi_at_f64(p, m, pts, SOFT)
        assert got.dtype == np.float32 and got.shape == (257,) and before == p.tobytes(), name
        assert np.all(want < 0.0) and within(got, want), (name, np.max(np.abs(got - want) / np.abs(want)))


def test_a_world_of_massless_particles_only_has_potential_zero_everywhere():
    a = np.zeros((5, 8), dtype=np.float32)
    a[:, 0], a[:, 7] = np.arange(5), 0.5
    w, p, m = host_world(a)
    assert m == 0
    phi = w.potential_at(probes(p, 40, seed=1), SOFT)
    img = w.potential_map(fitted(w, 9, 4), SOFT)
    w.close()
    assert phi.shape == (40,) and img.shape == (4, 9) and np.all(phi == 0.0) and np.all(img == 0.0)


def test_a_probe_exactly_on_the_single_source_is_minus_gm_over_sqrt_s():
    a = np.zeros((1, 8), dtype=np.float32)
    a[0, 0:2], a[0, 6], a[0, 7] = (3.0, -2.0), 1234.5, 0.25
    w, p, m = host_world(a)
    phi = w.potential_at([[3.0, -2.0], [3.0, 2.0]], SOFT)
    w.close()
    gm = float(np.float32(nb.NB_G) * np.float32(1234.5))
    want = np.array([-gm / np.sqrt(SOFT), -gm / np.sqrt(16.0 + SOFT)])
    assert np.all(np.isfinite(phi)) and within(phi, want), (phi, want)


def test_a_map_is_the_probes_product_at_the_pixel_centres_bit_for_bit(golden):
    w, p, m = host_world(golden("ic_333.bin"))
    for view in (fitted(w, 37, 7), offset_view(37, 7)):
        pts = pixel_points(view)
        img = w.potential_map(view, SOFT)
        assert img.dtype == np.float32 and img.shape == (7, 37)
        assert img.tobytes() == w.potential_at(pts, SOFT).tobytes()
        assert within(img.reshape(-1), phi_at_f64(p, m, pts, SOFT))
    w.close()


def test_probes_equal_massless_particles_of_radius_s_in_the_diagnostics():
    """World.potential_at of a never-stepped World against World.potential()[N:] of the same particles with the probes
    appended as massless particles of radius s.  The masses are integers below 2^20, so NB_G * m_j is exact in float32
    and the two host paths' definitions of G*m_j (the float32 product here, the float64 product in diag_cpu.c) name the
    same number: both are then the same float64 sum in the same order, rounded once."""
    rng = np.random.default_rng(8)
    a = synth(700, seed=8)[0]
    m = int(np.count_nonzero(a[:, 6] > 0))
    a[:m, 6] = rng.integers(1, 1 << 20, m).astype(np.float32)
    w, p, m = host_world(a)
    pts = probes(p, 130, seed=9)
    pts[5] = p[2, 0:2]
    got = w.potential_at(pts, SOFT)
    w.close()
    both = augmented(p, pts, SOFT)
    w2 = nb.World(both)
    assert w2.particles().tobytes() == both.tobytes()      # already partitioned: the probes stay at [N, N + n)
    want = w2.potential()[p.shape[0]:]
    w2.close()
    assert within(got, want.astype(np.float64)), np.max(np.abs(got - want) / np.abs(want))


def test_a_non_finite_point_gives_nan_and_no_points_give_an_empty_array(golden):
    w, p, m = host_world(golden("ic_333.bin"))
    pts = probes(p, 6, seed=2)
    pts[1, 0], pts[3, 1], pts[4, 0] = np.nan, np.inf, -np.inf
    phi = w.potential_at(pts, SOFT)
    assert np.isnan(phi).tolist() == [False, True, False, True, True, False]
    empty = w.potential_at(np.zeros((0, 2), dtype=np.float32), SOFT)
    assert empty.shape == (0,) and empty.dtype == np.float32
    # a view whose target is not finite: every pixel centre is NaN
    img = w.potential_map(nb.RenderView.make((np.nan, 0.0), (0.0, 0.0), 1.0, 3, 2, 1.0), SOFT)
    w.close()
    assert np.isnan(img).all()


def test_host_result_does_not_depend_on_the_thread_count():
    code = ("import sys, hashlib, numpy as np, nbody_amd as nb\n"
            "from gpu_common import synth\n"
            "from field_ref import probes\n"
            "w = nb.World(synth(3000, seed=11)[0]); p = w.particles(); h = hashlib.sha256()\n"
            "h.update(w.potential_at(probes(p, 500, seed=4), 0.75).tobytes())\n"
            "h.update(w.potential_map(w.fit_view(37, 7), 0.75).tobytes()); sys.stdout.write(h.hexdigest())\n")
    outs = []
    for threads in ("1", "4"):
        r = child(code, OMP_NUM_THREADS=threads)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1] and len(outs[0]) == 64


def test_cpu_only_world_never_opens_a_device():
    code = ("import os, numpy as np, nbody_amd as nb\n"
            "a = np.zeros((64, 8), dtype=np.float32); a[:, 0] = np.arange(64); a[:, 6] = 1; a[:, 7] = 1\n"
            "w = nb.World(a); w.update_cpu(0.01, 2)\n"
            "phi = w.potential_at([[1.5, 2.0], [70.0, -3.0]], 0.5); img = w.potential_map(w.fit_view(16, 4), 0.5); w.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', bool(np.all(phi < 0)), bool(np.all(img < 0)), img.shape)\n")
    r = child(code)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "OK True True (4, 16)"


# ---- argument checks -------------------------------------------------------------------------------------------------------

SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
         "w = nb.World(a); L = nb.nbody_lib()\n"
         "pts = np.zeros((3, 2), dtype=np.float32); out = np.zeros(64, dtype=np.float32)\n"
         "v = nb.RenderView.make((0.0, 0.0), (0.0, 0.0), 1.0, 4, 4, 1.0)\n")
SOFTENING = "softening must be finite and > 0"
ABORTS = [
    ("softening 0", "w.potential_at(pts, 0.0)", SOFTENING),
    ("softening negative", "w.potential_at(pts, -1.0)", SOFTENING),
    ("softening inf", "w.potential_at(pts, float('inf'))", SOFTENING),
    ("softening NaN", "w.potential_at(pts, float('nan'))", SOFTENING),
    ("map softening 0", "w.potential_map(v, 0.0)", SOFTENING),
    ("map softening NaN", "w.potential_map(v, float('nan'))", SOFTENING),
    ("zoom 0", "v.zoom = 0.0; L.RenderWorldPotential(w._h, v, 0.5, out.ctypes.data)", "zoom must be finite and > 0"),
    ("too many pixels", "v.width, v.height = 4097, 4096; L.RenderWorldPotential(w._h, v, 0.5, out.ctypes.data)", "must not exceed 2^24"),
    ("too many points", "L.GetWorldPotentialAt(w._h, pts.ctypes.data, (1 << 24) + 1, 0.5, out.ctypes.data)", "at most 2^24 points"),
    ("NULL phi", "L.GetWorldPotentialAt(w._h, pts.ctypes.data, 3, 0.5, None)", "NULL argument"),
    ("NULL points", "L.GetWorldPotentialAt(w._h, None, 3, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL map", "L.RenderWorldPotential(w._h, v, 0.5, None)", "NULL argument"),
    ("NULL view", "L.RenderWorldPotential(w._h, None, 0.5, out.ctypes.data)", "NULL argument"),
    ("map before set_data", "s = nb.SimPipeline(4, 4); s.potential_map(v, 0.5)", "nb_hip_potential_map before SetSimulationData"),
    ("probes before set_data", "s = nb.SimPipeline(4, 4); s.potential_at(pts, 0.5)", "nb_hip_potential_at before SetSimulationData"),
    ("sharded world", "fn = nb.ALLGATHER_FN(lambda *x: None); ws = L.CreateWorldShardedWith(a.ctypes.data, 4, 0, 2, fn, None); "
                      "L.RenderWorldPotential(ws, v, 0.5, out.ctypes.data)", "RenderWorldPotential of a sharded pipeline needs a collective"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


# ---- sources, headers, exports -----------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_field.h") == WORLD_FUNCS and set(WORLD_FUNCS) <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        assert set(WORLD_FUNCS) <= exported(os.path.join(nb.LIB_DIR, so)), so
    assert set(HIP_FUNCS) <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and set(HIP_FUNCS) <= exported(nb.HIP_SO)
    assert not {"nb_cpu_potential_at", "nb_cpu_potential_map"} & exported(nb.NBODY_SO)     # the host path is internal
    assert nb.hip_lib().nb_hip_version() == 400      # no version bump: the new surface is detected by its symbols
    assert 'dlsym "nb_hip_potential_map"' in open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    for method in ("potential_at", "potential_map"):
        assert callable(getattr(nb.SimPipeline, method)) and callable(getattr(nb.World, method))
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\bfield\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*\bfield_cpu\.c", make, re.M)
    assert '#include "diag_common.h"' in open(os.path.join(csrc, "field.hip")).read()
    for h in ("nbody.h", "galaxy.h", "nbody_diag.h", "nbody_render.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert not [f for f in WORLD_FUNCS if f in text], h


def test_pixel_points_restates_the_hosts_pixel_centres():
    """The one host function (render_common.h nb_render_pixel_centres) against tests/field_ref.py through a world of one
    unit source, on views with negative offsets, a zoom that is no power of two and a large target."""
    a = np.zeros((1, 8), dtype=np.float32)
    a[0, 6], a[0, 7] = 1.0, 1.0
    w = nb.World(a)
    for view in (offset_view(33, 5), nb.RenderView.make((1.0e3, -7.0), (640.0, 360.0), 3.0, 64, 3, 1.0)):
        assert w.potential_map(view, SOFT).tobytes() == w.potential_at(pixel_points(view), SOFT).tobytes()
    w.close()


# ---- static ISA of field.hip: the kernels of the Potential policy ----------------------------------------------------------------

def is_phi(name):
    return "Potential" in name


@pytest.fixture(scope="module")
def field_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("field_isa"), "field.hip")


def test_field_kernels_keep_eight_waves_per_simd_without_scratch(field_isa):
    assert len(kernel_meta(field_isa)) == 8          # 2 shapes x probes / map x 2 quantities (the g half: test_gravity_cpu.py)
    meta = [m for m in kernel_meta(field_isa) if is_phi(m[0])]
    assert sum("sample_split_kernel" in m[0] for m in meta) == 2 and sum("sample_wave_kernel" in m[0] for m in meta) == 2 and len(meta) == 4
    for name, scratch, sgpr, vgpr in meta:
        print(f"[field isa] {name}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgpr <= 64, (name, vgpr)


def test_field_kernels_keep_the_wait_state_behind_every_rsq(field_isa):
    fns = functions(field_isa)
    names = [n for n in fns if is_phi(n) and ("sample_split_kernel" in n or "sample_wave_kernel" in n)]
    assert len(names) == 4, sorted(fns)
    for name in names:
        assert check_rsq_wait_states(name, fns[name]) >= 1, name
