"""The acceleration at probe points and as a map (include/nbody_gravity.h) without a GPU: the host path of
GetWorldAccelerationAt / RenderWorldAcceleration against the float64 numpy restatement (tests/gravity_ref.py), the map =
probes identity, the argument checks, the header / binding / export agreement, and static checks on the ISA of
nbody_amd/csrc/field.hip.  Every child process hides the devices."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
from gravity_ref import g_at_f64, pixel_points, probes
from gpu_common import synth
from isa_common import check_rsq_wait_states, compile_isa, functions, kernel_meta
from test_abi import declared_functions, exported

ROOT = nb.ROOT
WORLD_FUNCS = ["GetWorldAccelerationAt", "RenderWorldAcceleration"]
HIP_FUNCS = ["nb_hip_acceleration_at", "nb_hip_acceleration_map"]
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
    """Each component is the float64 sum rounded once to float32 (the bound tests/test_field_cpu.py holds the host Phi to,
    with 1e-30 for the exact zeros a vector component can be)."""
    return np.all(np.abs(got.astype(np.float64) - want) <= 6e-8 * np.abs(want) + 1e-30)


def worst(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)))


def offset_view(width, height):
    return nb.RenderView.make((120.0, -40.0), (-3.5, -11.25), 0.37, width, height, 1.0)


# ---- the host path against float64 ---------------------------------------------------------------------------------------

def world_cases(golden):
    yield "ic_333", golden("ic_333.bin")
    yield "synthetic 3000", synth(3000, seed=21)[0]


def test_host_probes_and_map_match_f64(golden):
    for name, a in world_cases(golden):
        w, p, m = host_world(a)
        pts = probes(p, 257, seed=3)
        pts[0] = p[0, 0:2]                          # a probe exactly on a source
        got = w.acceleration_at(pts, SOFT)
        view = w.fit_view(19, 11)
        img = w.acceleration_map(view, SOFT)
        before = w.particles().tobytes()
        w.close()
        assert got.dtype == np.float32 and got.shape == (257, 2) and before == p.tobytes(), name
        assert img.dtype == np.float32 and img.shape == (11, 19, 2), name
        want, _ = g_at_f64(p, m, pts, SOFT)
        assert np.all(np.isfinite(got)) and within(got, want), (name, worst(got, want))
        want_img, _ = g_at_f64(p, m, pixel_points(view), SOFT)
        assert within(img.reshape(-1, 2), want_img), (name, worst(img.reshape(-1, 2), want_img))


def test_a_map_is_the_probes_product_at_the_pixel_centres_bit_for_bit(golden):
    w, p, m = host_world(golden("ic_333.bin"))
    for view in (w.fit_view(37, 7), offset_view(37, 7)):
        pts = pixel_points(view)
        img = w.acceleration_map(view, SOFT)
        assert img.dtype == np.float32 and img.shape == (7, 37, 2)
        assert img.tobytes() == w.acceleration_at(pts, SOFT).tobytes()
    w.close()


def test_a_probe_on_the_single_source_feels_nothing_and_one_beside_it_the_softened_pull():
    a = np.zeros((1, 8), dtype=np.float32)
    a[0, 0:2], a[0, 6], a[0, 7] = (3.0, -2.0), 1.0, 0.25
    w, p, m = host_world(a)
    d = 4.0
    g = w.acceleration_at([[3.0, -2.0], [3.0 + d, -2.0]], SOFT)
    w.close()
    gm = float(np.float32(nb.NB_G) * np.float32(1.0))
    assert g[0].tolist() == [0.0, 0.0]
    want = np.array([-gm * d / (d * d + SOFT) ** 1.5, 0.0])
    assert within(g[1], want), (g[1], want)


# ---- invariances -----------------------------------------------------------------------------------------------------------

def test_a_world_of_massless_particles_only_has_no_field():
    a = np.zeros((5, 8), dtype=np.float32)
    a[:, 0], a[:, 7] = np.arange(5), 0.5
    w, p, m = host_world(a)
    assert m == 0
    g = w.acceleration_at(probes(p, 40, seed=1), SOFT)
    img = w.acceleration_map(w.fit_view(9, 4), SOFT)
    w.close()
    assert g.shape == (40, 2) and img.shape == (4, 9, 2)
    assert not g.view(np.uint32).any() and not img.view(np.uint32).any()          # (+0, +0) everywhere


def test_a_non_finite_point_gives_nan_pairs_and_no_points_give_an_empty_array(golden):
    w, p, m = host_world(golden("ic_333.bin"))
    pts = probes(p, 6, seed=2)
    pts[1, 0], pts[3, 1], pts[4, 0] = np.nan, np.inf, -np.inf
    g = w.acceleration_at(pts, SOFT)
    assert np.isnan(g).tolist() == [[b, b] for b in (False, True, False, True, True, False)]
    empty = w.acceleration_at(np.zeros((0, 2), dtype=np.float32), SOFT)
    assert empty.shape == (0, 2) and empty.dtype == np.float32
    # a view whose target is not finite in x: every pixel centre is non-finite
    img = w.acceleration_map(nb.RenderView.make((np.nan, 0.0), (0.0, 0.0), 1.0, 3, 2, 1.0), SOFT)
    w.close()
    assert img.shape == (2, 3, 2) and np.isnan(img).all()


def test_host_result_does_not_depend_on_the_thread_count():
    code = ("import sys, hashlib, numpy as np, nbody_amd as nb\n"
            "from gpu_common import synth\n"
            "from gravity_ref import probes\n"
            "w = nb.World(synth(3000, seed=11)[0]); p = w.particles(); h = hashlib.sha256()\n"
            "h.update(w.acceleration_at(probes(p, 500, seed=4), 0.75).tobytes())\n"
            "h.update(w.acceleration_map(w.fit_view(37, 7), 0.75).tobytes()); sys.stdout.write(h.hexdigest())\n")
    outs = []
    for threads in ("1", "7"):
        r = child(code, OMP_NUM_THREADS=threads)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1] and len(outs[0]) == 64


def test_cpu_only_world_never_opens_a_device():
    code = ("import os, numpy as np, nbody_amd as nb\n"
            "a = np.zeros((64, 8), dtype=np.float32); a[:, 0] = np.arange(64); a[:, 6] = 1; a[:, 7] = 1\n"
            "w = nb.World(a); w.update_cpu(0.01, 2)\n"
            "g = w.acceleration_at([[-1.5, 2.0], [70.0, -3.0]], 0.5); img = w.acceleration_map(w.fit_view(16, 4), 0.5); w.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', bool(g[0, 0] > 0 and g[1, 0] < 0), bool(np.isfinite(img).all()), img.shape)\n")
    r = child(code)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "OK True True (4, 16, 2)"


# ---- argument checks -------------------------------------------------------------------------------------------------------

SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
         "w = nb.World(a); L = nb.nbody_lib()\n"
         "pts = np.zeros((3, 2), dtype=np.float32); out = np.zeros(64, dtype=np.float32)\n"
         "v = nb.RenderView.make((0.0, 0.0), (0.0, 0.0), 1.0, 4, 4, 1.0)\n")
SOFTENING = "softening must be finite and > 0"
SHARDED = "fn = nb.ALLGATHER_FN(lambda *x: None); ws = L.CreateWorldShardedWith(a.ctypes.data, 4, 0, 2, fn, None); "
ABORTS = [
    ("softening 0", "w.acceleration_at(pts, 0.0)", SOFTENING),
    ("softening negative", "w.acceleration_at(pts, -1.0)", SOFTENING),
    ("softening inf", "w.acceleration_at(pts, float('inf'))", SOFTENING),
    ("softening NaN", "w.acceleration_at(pts, float('nan'))", SOFTENING),
    ("map softening 0", "w.acceleration_map(v, 0.0)", SOFTENING),
    ("map softening negative", "w.acceleration_map(v, -1.0)", SOFTENING),
    ("map softening inf", "w.acceleration_map(v, float('inf'))", SOFTENING),
    ("map softening NaN", "w.acceleration_map(v, float('nan'))", SOFTENING),
    ("zoom 0", "v.zoom = 0.0; L.RenderWorldAcceleration(w._h, v, 0.5, out.ctypes.data)", "zoom must be finite and > 0"),
    ("too many pixels", "v.width, v.height = 4097, 4096; L.RenderWorldAcceleration(w._h, v, 0.5, out.ctypes.data)", "must not exceed 2^24"),
    ("too many points", "L.GetWorldAccelerationAt(w._h, pts.ctypes.data, (1 << 24) + 1, 0.5, out.ctypes.data)", "at most 2^24 points"),
    ("NULL acc", "L.GetWorldAccelerationAt(w._h, pts.ctypes.data, 3, 0.5, None)", "NULL argument"),
    ("NULL points", "L.GetWorldAccelerationAt(w._h, None, 3, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL world", "L.GetWorldAccelerationAt(None, pts.ctypes.data, 3, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL map", "L.RenderWorldAcceleration(w._h, v, 0.5, None)", "NULL argument"),
    ("NULL view", "L.RenderWorldAcceleration(w._h, None, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL map world", "L.RenderWorldAcceleration(None, v, 0.5, out.ctypes.data)", "NULL argument"),
    ("map before set_data", "s = nb.SimPipeline(4, 4); s.acceleration_map(v, 0.5)", "nb_hip_acceleration_map before SetSimulationData"),
    ("probes before set_data", "s = nb.SimPipeline(4, 4); s.acceleration_at(pts, 0.5)", "nb_hip_acceleration_at before SetSimulationData"),
    ("sharded world map", SHARDED + "L.RenderWorldAcceleration(ws, v, 0.5, out.ctypes.data)",
     "RenderWorldAcceleration of a sharded pipeline needs a collective"),
    ("sharded world probes", SHARDED + "L.GetWorldAccelerationAt(ws, pts.ctypes.data, 3, 0.5, out.ctypes.data)",
     "GetWorldAccelerationAt of a sharded pipeline needs a collective"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


# ---- sources, headers, exports -----------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_gravity.h") == WORLD_FUNCS and set(WORLD_FUNCS) <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        assert set(WORLD_FUNCS) <= exported(os.path.join(nb.LIB_DIR, so)), so
    assert set(HIP_FUNCS) <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and set(HIP_FUNCS) <= exported(nb.HIP_SO)
    for so in WORLD_LIBS:          # the host path is internal
        assert not {"nb_cpu_acceleration_at", "nb_cpu_acceleration_map"} & exported(os.path.join(nb.LIB_DIR, so)), so
    assert nb.hip_lib().nb_hip_version() == 400      # no version bump: the new surface is detected by its symbols
    assert 'dlsym "nb_hip_acceleration_map"' in open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    for method in ("acceleration_at", "acceleration_map"):
        assert callable(getattr(nb.SimPipeline, method)) and callable(getattr(nb.World, method))
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    # the acceleration lives in the field sampler's files: field.hip, field_cpu.c, field_common.h
    assert re.search(r"^HIP_TUS\s*:=.*\bfield\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*\bfield_cpu\.c", make, re.M)
    assert re.search(r"^WORLD_HDRS\s*:=(.*\\\n)*.*field_common\.h", make, re.M) and make.count("field_common.h") >= 2
    assert make.count("include/nbody_gravity.h") >= 2          # libnbody*.so (WORLD_HDRS) and the HIP objects
    text = open(os.path.join(csrc, "field.hip")).read()
    assert '#include "diag_common.h"' in text and '#include "interaction_asm.h"' in text and "NB_INTERACTION2_ASM" in text
    assert '"gravity_shape"' in open(os.path.join(csrc, "nbody_hip_tuning.h")).read()
    for h in ("nbody.h", "galaxy.h", "nbody_diag.h", "nbody_render.h", "nbody_field.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert not [f for f in WORLD_FUNCS + HIP_FUNCS if f in text], h


# ---- static ISA of field.hip: the kernels of the Acceleration policy -------------------------------------------------------------

KERNELS = ("sample_split_kernel", "sample_wave_kernel")


def is_g(name):
    return "Acceleration" in name


@pytest.fixture(scope="module")
def gravity_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("gravity_isa"), "field.hip")


def test_gravity_kernels_keep_eight_waves_per_simd_without_scratch(gravity_isa):
    meta = [m for m in kernel_meta(gravity_isa) if is_g(m[0])]
    assert [sum(k in m[0] for m in meta) for k in KERNELS] == [2, 2] and len(meta) == 4, [m[0] for m in meta]
    for name, scratch, sgpr, vgpr in meta:
        print(f"[gravity isa] {name}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgpr <= 64, (name, vgpr)          # __launch_bounds__(..., 8): eight waves per SIMD


def test_gravity_kernels_keep_the_wait_state_behind_every_rsq(gravity_isa):
    fns = functions(gravity_isa)
    names = [n for n in fns if is_g(n) and any(k in n for k in KERNELS)]
    assert len(names) == 4, sorted(fns)
    for name in names:
        assert check_rsq_wait_states(name, fns[name]) >= 2, name


def loops(text, symbol):
    """(label, opcodes) of every basic block of `symbol` that branches back to its own label."""
    body = text[text.index(symbol + ":"):]
    body = body[:body.index(".Lfunc_end")]
    parts = re.split(r"^(\.LBB\d+_\d+):", body, flags=re.M)
    for k in range(1, len(parts), 2):
        lines = [ln.split(";")[0].strip() for ln in parts[k + 1].splitlines()]
        ins = [ln for ln in lines if ln and not ln.startswith(".")]
        if any(ins_.split()[-1] == parts[k] for ins_ in ins if ins_.startswith(("s_cbranch", "s_branch"))):
            yield parts[k], [i.split()[0] for i in ins]


def test_the_unmasked_loop_of_every_kernel_holds_sixteen_rsq_per_eight_sources(gravity_isa):
    names = [name for name, *_ in kernel_meta(gravity_isa) if is_g(name)]
    assert len(names) == 4, names
    for name in names:
        fetch8 = [(lab, ops) for lab, ops in loops(gravity_isa, name) if "s_load_dwordx16" in ops]
        assert len(fetch8) == 1, (name, [lab for lab, _ in fetch8])
        ops = fetch8[0][1]
        assert sum(o.startswith("v_rsq_f32") for o in ops) == 16, (name, ops)          # 8 sources x 2 samples per lane
