"""The potential and the acceleration field of world ensembles (include/nbody_batch_field.h, nb_hip_ensemble_potential_at and
its three siblings) without a GPU: the host path of a WorldBatch that never stepped against nb.World(member) bit for bit,
uniform and ragged; broadcasting of one point set or view; the edge values; the argument checks; the header / binding /
export / Makefile agreement; and static checks on the ISA of nbody_amd/csrc/batch_field.hip.  Every child process hides the
devices."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
from isa_common import check_rsq_wait_states, compile_isa, functions, kernel_meta
from test_abi import declared_functions, exported

ROOT = nb.ROOT
WORLD_FUNCS = ["GetWorldBatchPotentialAt", "RenderWorldBatchPotential", "GetWorldBatchAccelerationAt", "RenderWorldBatchAcceleration"]
HIP_FUNCS = ["nb_hip_ensemble_potential_at", "nb_hip_ensemble_potential_map", "nb_hip_ensemble_acceleration_at",
             "nb_hip_ensemble_acceleration_map"]
METHODS = ("potential_at", "potential_map", "acceleration_at", "acceleration_map")
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")
HIDDEN = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
SOFT = 0.75


def child(code):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **HIDDEN)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def member(n, massive, seed):
    """n particles in caller order, `massive` of them with mass, scattered among the massless ones"""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * 40.0
    a[:, 2:4] = rng.standard_normal((n, 2))
    a[:, 7] = 0.5 + rng.random(n)
    a[rng.permutation(n)[:massive], 6] = (10.0 + 990.0 * rng.random(massive)).astype(np.float32)
    return a


def points(count, n, seed):
    return (np.random.default_rng(seed).standard_normal((count, n, 2)) * 60.0).astype(np.float32)


def views(count, width, height):
    """one view per member, each different: negative offsets, zooms that are no powers of two"""
    return [nb.RenderView.make((12.0 * b, -4.0 - b), (-3.5 + b, -1.25 * b), 0.37 + 0.11 * b, width, height, 1.0) for b in range(count)]


def uniform_batch():
    members = [member(7, m, seed=10 + m) for m in (3, 7, 5)]
    return nb.WorldBatch(np.stack(members)), members


def ragged_batch():
    members = [member(n, m, seed=20 + n) for n, m in ((1, 1), (4, 0), (9, 6))]          # one member without a source
    return nb.WorldBatch.ragged(members), members


# ---- the host path: member b is nb.World(member b) ---------------------------------------------------------------------------

@pytest.mark.parametrize("make", [uniform_batch, ragged_batch], ids=["uniform", "ragged"])
def test_a_batch_that_never_stepped_answers_on_the_host_with_the_bits_of_each_member_alone(make):
    wb, members = make()
    count = len(members)
    pts, vs = points(count, 5, seed=1), views(count, 6, 3)
    pts[0, 2] = members[0][0, 0:2]                    # a probe exactly on a particle
    got = (wb.potential_at(pts, SOFT), wb.potential_map(vs, SOFT), wb.acceleration_at(pts, SOFT), wb.acceleration_map(vs, SOFT))
    assert [g.shape for g in got] == [(count, 5), (count, 3, 6), (count, 5, 2), (count, 3, 6, 2)]
    assert all(g.dtype == np.float32 for g in got)
    before = [wb.member(b).tobytes() for b in range(count)]
    for b in range(count):
        w = nb.World(members[b])
        assert w.particles().tobytes() == before[b]
        want = (w.potential_at(pts[b], SOFT), w.potential_map(vs[b], SOFT), w.acceleration_at(pts[b], SOFT), w.acceleration_map(vs[b], SOFT))
        w.close()
        for name, g, x in zip(METHODS, got, want):
            assert g[b].tobytes() == x.tobytes(), (b, name)
    if make is ragged_batch:
        assert np.all(got[0][1] == 0.0) and np.all(got[1][1] == 0.0) and np.all(got[2][1] == 0.0) and np.all(got[3][1] == 0.0)   # M = 0
        assert np.all(got[0][2] < 0.0)
    wb.close()


def test_one_point_set_or_view_for_all_members_is_that_set_given_to_each():
    wb, members = uniform_batch()
    pts, view = points(1, 9, seed=2)[0], views(1, 5, 4)[0]
    assert wb.potential_at(pts, SOFT).tobytes() == wb.potential_at(np.stack([pts] * 3), SOFT).tobytes()
    assert wb.acceleration_at(pts, SOFT).tobytes() == wb.acceleration_at(np.stack([pts] * 3), SOFT).tobytes()
    assert wb.potential_map(view, SOFT).tobytes() == wb.potential_map([view] * 3, SOFT).tobytes()
    assert wb.acceleration_map(view, SOFT).tobytes() == wb.acceleration_map([view] * 3, SOFT).tobytes()
    with pytest.raises(ValueError):
        wb.potential_at(np.zeros((2, 4, 2), np.float32), SOFT)         # neither (n, 2) nor (3, n, 2)
    with pytest.raises(ValueError):
        wb.potential_map([view] * 2, SOFT)
    wb.close()


def test_a_nan_coordinate_gives_nan_for_that_sample_only_and_no_points_give_empty_arrays():
    wb, members = ragged_batch()
    pts = points(3, 4, seed=3)
    clean_phi, clean_g = wb.potential_at(pts, SOFT), wb.acceleration_at(pts, SOFT)
    bad = pts.copy()
    bad[0, 1, 0], bad[1, 3, 1], bad[2, 0, 0] = np.nan, np.inf, -np.inf      # member 1 has no source: NaN whatever M
    phi, g = wb.potential_at(bad, SOFT), wb.acceleration_at(bad, SOFT)
    hit = np.zeros((3, 4), dtype=bool)
    hit[0, 1] = hit[1, 3] = hit[2, 0] = True
    assert np.array_equal(np.isnan(phi), hit) and np.array_equal(np.isnan(g), np.stack([hit, hit], axis=-1))
    assert phi[~hit].tobytes() == clean_phi[~hit].tobytes() and g[~hit].tobytes() == clean_g[~hit].tobytes()
    empty = np.zeros((0, 2), dtype=np.float32)
    assert wb.potential_at(empty, SOFT).shape == (3, 0) and wb.acceleration_at(empty, SOFT).shape == (3, 0, 2)
    assert wb.potential_at(np.zeros((3, 0, 2), np.float32), SOFT).dtype == np.float32
    wb.close()


def test_a_batch_that_never_stepped_never_opens_a_device():
    code = ("import os, numpy as np, nbody_amd as nb\n"
            "a = np.zeros((2, 16, 8), dtype=np.float32); a[:, :, 0] = np.arange(16); a[:, :, 6] = 1; a[:, :, 7] = 1\n"
            "wb = nb.WorldBatch(a); v = nb.RenderView.make((8.0, 0.0), (4.0, 2.0), 0.5, 8, 4, 1.0)\n"
            "pts = np.array([[1.5, 2.0], [70.0, -3.0]], dtype=np.float32)\n"
            "out = [wb.potential_at(pts, 0.5), wb.potential_map(v, 0.5), wb.acceleration_at(pts, 0.5), wb.acceleration_map(v, 0.5)]\n"
            "wb.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', bool(np.all(out[0] < 0)), [o.shape for o in out])\n")
    r = child(code)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == "OK True [(2, 2), (2, 4, 8), (2, 2, 2), (2, 4, 8, 2)]"


# ---- argument checks -------------------------------------------------------------------------------------------------------

SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((3, 4, 8), dtype=np.float32); a[:, :, 0] = np.arange(4); a[:, :, 6] = 1; a[:, :, 7] = 0.25\n"
         "w = nb.WorldBatch(a); L = nb.nbody_lib(); H = nb.hip_lib()\n"
         "pts = np.zeros((3, 2, 2), dtype=np.float32); out = np.zeros(256, dtype=np.float32)\n"
         "v = nb.RenderView.make((0.0, 0.0), (0.0, 0.0), 1.0, 4, 4, 1.0)\n"
         "vs = (nb.RenderView * 3)(v, v, v)\n"
         "s = nb.SimBatch(4, [4, 4, 4])\n")
SOFTENING = "softening must be finite and > 0"
ABORTS = [
    ("softening 0", "w.potential_at(pts, 0.0)", SOFTENING),
    ("softening negative", "w.acceleration_at(pts, -1.0)", SOFTENING),
    ("softening NaN", "w.potential_at(pts, float('nan'))", SOFTENING),
    ("map softening 0", "w.potential_map(v, 0.0)", SOFTENING),
    ("map softening negative", "w.acceleration_map(v, -0.5)", SOFTENING),
    ("map softening NaN", "w.acceleration_map(v, float('nan'))", SOFTENING),
    ("views of differing size", "vs[2].width = 5; L.RenderWorldBatchPotential(w._h, vs, 0.5, out.ctypes.data)",
     "invalid RenderView of member 2 of 3 (5 x 4, zoom 1): width and height differ from member 0's"),
    ("an invalid view", "vs[1].zoom = 0.0; L.RenderWorldBatchAcceleration(w._h, vs, 0.5, out.ctypes.data)",
     "invalid RenderView of member 1 of 3"),
    ("too many pixels in all", "vs[0].width = vs[1].width = vs[2].width = 2048; vs[0].height = vs[1].height = vs[2].height = 4096; "
                               "L.RenderWorldBatchPotential(w._h, vs, 0.5, out.ctypes.data)", "count * width * height must not exceed 2^24"),
    ("too many points in all", "L.GetWorldBatchPotentialAt(w._h, pts.ctypes.data, (1 << 24) // 3 + 1, 0.5, out.ctypes.data)",
     "at most 2^24 points per call"),
    ("too many points in all, g", "L.GetWorldBatchAccelerationAt(w._h, pts.ctypes.data, (1 << 24) // 3 + 1, 0.5, out.ctypes.data)",
     "at most 2^24 points per call"),
    ("NULL batch", "L.GetWorldBatchPotentialAt(None, pts.ctypes.data, 2, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL points", "L.GetWorldBatchPotentialAt(w._h, None, 2, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL phi", "L.GetWorldBatchPotentialAt(w._h, pts.ctypes.data, 2, 0.5, None)", "NULL argument"),
    ("NULL acc", "L.GetWorldBatchAccelerationAt(w._h, pts.ctypes.data, 2, 0.5, None)", "NULL argument"),
    ("NULL views", "L.RenderWorldBatchPotential(w._h, None, 0.5, out.ctypes.data)", "NULL argument"),
    ("NULL map", "L.RenderWorldBatchAcceleration(w._h, vs, 0.5, None)", "NULL argument"),
    ("NULL ensemble", "H.nb_hip_ensemble_potential_map(None, vs, 0.5, out.ctypes.data)", "NULL ensemble"),
    ("probes before set_data", "s.potential_at(pts, 0.5)", "nb_hip_ensemble_potential_at before nb_hip_batch_set_data"),
    ("map before set_data", "s.potential_map(v, 0.5)", "nb_hip_ensemble_potential_map before nb_hip_batch_set_data"),
    ("g probes before set_data", "s.acceleration_at(pts, 0.5)", "nb_hip_ensemble_acceleration_at before nb_hip_batch_set_data"),
    ("g map before set_data", "s.acceleration_map(v, 0.5)", "nb_hip_ensemble_acceleration_map before nb_hip_batch_set_data"),
    ("ragged before set_data", "nb.SimBatch.ragged([4, 9], [1, 2]).potential_map(v, 0.5)",
     "nb_hip_ensemble_potential_map before nb_hip_batch_set_data"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


# ---- sources, headers, exports -----------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_batch_field.h") == WORLD_FUNCS and set(WORLD_FUNCS) <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        assert set(WORLD_FUNCS) <= exported(os.path.join(nb.LIB_DIR, so)), so
    assert set(HIP_FUNCS) <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and set(HIP_FUNCS) <= exported(nb.HIP_SO)
    assert not set(HIP_FUNCS) & set(nb.TUNE_API)
    assert nb.hip_lib().nb_hip_version() == 400      # no version bump: the new surface is detected by its symbols
    assert 'dlsym "nb_hip_ensemble_potential_map"' in open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    for method in METHODS:
        assert callable(getattr(nb.SimBatch, method)) and callable(getattr(nb.WorldBatch, method))
    assert "ragged" in open(os.path.join(ROOT, "include", "nbody_batch_field.h")).read().lower()     # said where it is supported
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\bbatch_field\b", make, re.M) and re.search(r"^HIP_TUS\s*:=.*\bfield\b", make, re.M)
    assert re.search(r"^WORLD_HDRS\s*:=(?:.*\\\n)*.*nbody_batch_field\.h", make, re.M)
    for header in ("field_kernels.h", "batch_field.h"):
        assert re.search(r"^\$\(OUT\)/%\.o:.*\$\(HERE\)" + re.escape(header), make, re.M), header
    # one set of statements: both files take the policies, the loads, the store and the slice sum from the shared header
    shared = open(os.path.join(csrc, "field_kernels.h")).read()
    for name in ("struct Potential", "struct Acceleration", "struct Params", "void load_samples(", "void store_sample(", "void slice_sum("):
        assert name in shared, name
        for f in ("field.hip", "batch_field.hip"):
            text = open(os.path.join(csrc, f)).read()
            assert name not in text and '#include "field_kernels.h"' in text, (name, f)
    assert '#include "diag_common.h"' in open(os.path.join(csrc, "field.hip")).read()


# ---- static ISA of batch_field.hip -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch_field_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("batch_field_isa"), "batch_field.hip")


def test_the_four_ensemble_kernels_keep_eight_waves_per_simd_without_scratch(batch_field_isa):
    meta = kernel_meta(batch_field_isa)
    assert len(meta) == 4 and all("ensemble_sample_kernel" in m[0] for m in meta), [m[0] for m in meta]
    assert sum("Potential" in m[0] for m in meta) == 2 and sum("Acceleration" in m[0] for m in meta) == 2
    for name, scratch, sgpr, vgpr in meta:
        print(f"[batch field isa] {name}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs")
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert vgpr <= 64, (name, vgpr)


def test_the_ensemble_kernels_keep_the_wait_state_behind_every_rsq(batch_field_isa):
    fns = functions(batch_field_isa)
    names = [n for n in fns if "ensemble_sample_kernel" in n]
    assert len(names) == 4, sorted(fns)
    for name in names:
        assert check_rsq_wait_states(name, fns[name]) >= 1, name


def test_field_hip_still_compiles_to_its_eight_kernels(tmp_path_factory):
    meta = kernel_meta(compile_isa(tmp_path_factory.mktemp("field_isa_again"), "field.hip"))
    assert len(meta) == 8
    assert sum("sample_split_kernel" in m[0] for m in meta) == 4 and sum("sample_wave_kernel" in m[0] for m in meta) == 4
