"""Ragged world ensembles without a GPU: the declared surface (include/nbody_hip.h nb_hip_ragged_*,
include/nbody_batch_ragged.h), creation and its launch groups, the argument checks, the World layer's partition and host
diagnostics, and the static ISA of the kernels that find their members through the ragged tables: the instantiations for
nb::RaggedParams of kernels.hip batch_chain_kernel / batch_trace_chain_kernel / batch_lane_split_kernel, for
nbd::RaggedDiagParams of batch_diag.hip ensemble_phi_kernel, for RaggedRecords of convert.hip batch_split_kernel /
batch_merge_kernel, and convert.hip ragged_copy_rows_kernel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nbody_amd as nb
from isa_common import check_rsq_wait_states, compile_isa, functions, kernel_meta
from test_abi import declared_functions, exported
from test_batch_cpu import BATCH_HIP, BATCH_WORLD, _batch

ROOT = nb.ROOT
RAGGED_HIP = ["nb_hip_ragged_create", "nb_hip_ragged_layout", "nb_hip_ragged_launch_shape", "nb_hip_ragged_member_shape"]
RAGGED_WORLD = ["CreateWorldBatchRagged"]
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")


# ---- surface ---------------------------------------------------------------------------------------------------------

def test_header_exports_and_binding_agree_for_both_libraries():
    names = declared_functions("nbody_hip.h")
    assert [n for n in names if n.startswith("nb_hip_ragged_")] == RAGGED_HIP
    have = exported(nb.HIP_SO)
    assert sorted(n for n in have if n.startswith("nb_hip_ragged_")) == sorted(RAGGED_HIP)
    assert set(RAGGED_HIP) <= set(nb.HIP_API) and not set(RAGGED_HIP) & set(nb.TUNE_API)
    assert declared_functions("nbody_batch_ragged.h") == RAGGED_WORLD and set(RAGGED_WORLD) <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        assert set(RAGGED_WORLD) <= exported(os.path.join(nb.LIB_DIR, so)), so
    assert callable(nb.SimBatch.ragged) and callable(nb.WorldBatch.ragged)
    nb.hip_lib()
    nb.nbody_lib()          # binds every entry or raises


def test_the_pinned_headers_gained_nothing_and_the_version_stays():
    assert declared_functions("nbody_batch.h") == BATCH_WORLD
    assert [n for n in declared_functions("nbody_hip.h") if n.startswith("nb_hip_batch_")] == BATCH_HIP
    assert declared_functions("nbody_batch_diag.h") == ["GetWorldBatchEnergy", "GetWorldBatchPotential"]
    assert declared_functions("nbody_batch_trace.h") == ["UpdateWorldBatch_GPU_Traced", "UpdateWorldBatch_GPU_Traced_dts"]
    for header in ("nbody.h", "galaxy.h", "nbody_diag.h", "nbody_batch.h", "nbody_batch_diag.h", "nbody_batch_trace.h",
                   "nbody_batch_render.h", "nbody_render.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "ragged" not in text.lower(), header
    assert nb.hip_lib().nb_hip_version() == 400
    assert 'dlsym "nb_hip_ragged_create"' in open(os.path.join(ROOT, "include", "nbody_hip.h")).read()


# ---- creation --------------------------------------------------------------------------------------------------------

SIZES = [1, 128, 129, 512, 513, 1581, 1582, 3000]
ORDER = [5, 2, 7, 0, 4, 3, 6, 1]            # member b holds SIZES[ORDER[b]]


def test_create_and_destroy_touch_no_gpu_and_report_the_groups():
    sizes = [SIZES[i] for i in ORDER]
    r = nb.SimBatch.ragged(sizes, [n // 3 for n in sizes])
    shape = r.launch_shape()
    # chain: 1, 128, 129, 512 (w of the largest: 4); lane-split (8, 8): 513, 1581; lane-split (16, 4): 1582, 3000
    assert shape["groups"] == [
        {"path": "chain", "k": 2, "w": 4, "lanes": 1, "members": 4, "workgroups": 4},
        {"path": "lanes", "k": 1, "w": 8, "lanes": 8, "members": 2, "workgroups": 2 * 198},
        {"path": "lanes", "k": 1, "w": 16, "lanes": 4, "members": 2, "workgroups": 2 * 188}]
    want = {1: (0, 2, 16, 1), 128: (0, 2, 16, 1), 129: (0, 2, 8, 1), 512: (0, 2, 4, 1), 513: (1, 1, 8, 8), 1581: (1, 1, 8, 8),
            1582: (2, 1, 16, 4), 3000: (2, 1, 16, 4)}
    assert shape["members"] == [want[n] for n in sizes]
    assert r.sizes() == sizes
    assert r.last_ms() == 0.0 and r.dt_uploads() == 0
    r.sync()                 # nothing on the device yet: a no-op
    r.close()
    # a member's shape is a function of its own size alone: the same as that of a uniform ensemble of its size
    for n in SIZES:
        u = nb.SimBatch(n, [0])
        s = u.launch_shape()
        assert (s["k"], s["w"], s["lanes"]) == want[n][1:], n
        u.close()
    # absent groups are not reported
    r = nb.SimBatch.ragged([2000, 1600], [5, 0])
    assert [(g["path"], g["w"], g["lanes"], g["members"]) for g in r.launch_shape()["groups"]] == [("lanes", 16, 4, 2)]
    r.close()


def test_layout_offsets_are_the_running_sum_also_for_a_uniform_ensemble():
    sizes = [SIZES[i] for i in ORDER]
    r = nb.SimBatch.ragged(sizes, [0] * len(sizes))
    got_sizes, offsets = r.layout()
    assert list(got_sizes) == sizes and list(offsets) == [0] + list(np.cumsum(sizes))
    r.close()
    u = nb.SimBatch(250, [0, 250, 17])
    got_sizes, offsets = u.layout()
    assert list(got_sizes) == [250] * 3 and list(offsets) == [0, 250, 500, 750]
    u.close()


def _group(batch, i):
    """nb_hip_ragged_launch_shape of group i, called on the handle whatever made it: (groups, path, k, w, lanes, members, workgroups)."""
    path, k, w, lanes, members, wgs = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_uint32(), C.c_uint32()
    total = nb.hip_lib().nb_hip_ragged_launch_shape(batch._h, i, C.byref(path), C.byref(k), C.byref(w), C.byref(lanes), C.byref(members),
                                                    C.byref(wgs))
    return (int(total), path.value, k.value, w.value, lanes.value, members.value, wgs.value)


def _member(batch, b):
    grp, k, w, lanes = C.c_uint32(), C.c_int(), C.c_int(), C.c_int()
    nb.hip_lib().nb_hip_ragged_member_shape(batch._h, b, C.byref(grp), C.byref(k), C.byref(w), C.byref(lanes))
    return (grp.value, k.value, w.value, lanes.value)


@pytest.mark.parametrize("n", [1, 128, 129, 256, 257, 512, 513, 1581, 1582, 3000])
def test_a_uniform_ensemble_is_the_one_group_case_of_a_ragged_one(n):
    """SimBatch(N, [N, 0]) and SimBatch.ragged([N, N], [N, 0]) come out of one constructor: one group of 2 members with the
    shape nb_hip_batch_launch_shape reports, the same member shapes, the same layout.  Creation touches no device."""
    u, r = nb.SimBatch(n, [n, 0]), nb.SimBatch.ragged([n, n], [n, 0])
    s = u.launch_shape()
    total, path, k, w, lanes, members, wgs = _group(u, 0)
    assert (total, members) == (1, 2)
    assert ("lanes" if path else "chain", k, w, lanes, wgs) == (s["path"], s["k"], s["w"], s["lanes"], s["workgroups"])
    assert _group(r, 0) == _group(u, 0)
    assert r.launch_shape()["groups"] == [dict(s, members=2)]
    assert [_member(u, b) for b in range(2)] == [_member(r, b) for b in range(2)] == [(0, k, w, lanes)] * 2
    (us, uo), (rs, ro) = u.layout(), r.layout()
    assert list(us) == list(rs) == [n, n] and list(uo) == list(ro) == [0, n, 2 * n]
    u.close()
    r.close()


# ---- argument checks ---------------------------------------------------------------------------------------------------

RENDER_SETUP = "import numpy as np; r = nb.SimBatch.ragged([4, 5], [1, 1]); v = nb.RenderView.make((0, 0), (0, 0), 1.0, 8, 8, 1.0); "
WORLD_SETUP = ("import numpy as np; w = nb.WorldBatch.ragged([np.ones((4, 8), np.float32), np.ones((5, 8), np.float32)]); "
               "v = nb.RenderView.make((0, 0), (0, 0), 1.0, 8, 8, 1.0); ")
ABORTS = [
    ("count = 0", "nb.SimBatch.ragged([], [])", "count = 0"),
    ("a size of 0", "nb.SimBatch.ragged([5, 0, 7], [1, 0, 1])", "member 1: total_len = 0"),
    ("a size of 3001", "nb.SimBatch.ragged([5, 7, 3001], [1, 1, 1])", "member 2: total_len 3001 > 3000"),
    ("mass_len > size", "nb.SimBatch.ragged([5, 7, 9], [1, 8, 1])", "member 1: mass_len 8 > total_len 7"),
    ("update before set_data", "nb.SimBatch.ragged([5, 700], [1, 2]).update(1, 0.01)", "before nb_hip_batch_set_data"),
    ("bounds", RENDER_SETUP + "r.bounds()", "nb_hip_ensemble_bounds: rendering of ragged ensembles"),
    ("render_counts", RENDER_SETUP + "r.render_counts(v)", "nb_hip_ensemble_render_counts: rendering of ragged ensembles"),
    ("render_rgba", RENDER_SETUP + "r.render(v)", "nb_hip_ensemble_render_rgba: rendering of ragged ensembles"),
    ("world size of 0", "import numpy as np; nb.WorldBatch.ragged([np.ones((4, 8), np.float32), np.ones((0, 8), np.float32)])",
     "member 1: world_size 0 outside"),
    ("world of 0 members", "nb.WorldBatch.ragged([])", "count 0 outside"),
    ("world bounds", WORLD_SETUP + "w.bounds()", "GetWorldBatchBounds: rendering of ragged ensembles"),
    ("world fit_views", WORLD_SETUP + "w.fit_views(8, 8)", "FitWorldBatchViews: rendering of ragged ensembles"),
    ("world render_counts", WORLD_SETUP + "w.render_counts(v)", "RenderWorldBatchCounts: rendering of ragged ensembles"),
    ("world render", WORLD_SETUP + "w.render(v)", "RenderWorldBatch: rendering of ragged ensembles"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    """Every case runs with every GPU hidden: the checks come before any device touch."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run(["python", "-c", "import nbody_amd as nb\n" + code + "\nprint('SURVIVED')"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


# ---- World layer: partition and host diagnostics, no GPU ----------------------------------------------------------------

def test_world_batch_ragged_partitions_and_diagnoses_each_member_as_a_world_does():
    """Before any update: member(b) == World(member).particles() bytewise, and energy() / potential() -- the host path,
    member by member -- equal World(member).energy() / .potential() bit for bit.  In a child process that hides every GPU."""
    code = """
import numpy as np, nbody_amd as nb
from gpu_common import synth
sizes, fracs = [333, 1, 700, 7, 1582], [0.5, 1.1, 0.0, 0.9, 0.1]
members = [synth(n, frac_massive=f, seed=40 + i)[0][::-1].copy() for i, (n, f) in enumerate(zip(sizes, fracs))]   # massless first
wb = nb.WorldBatch.ragged(members)
assert wb.sizes() == sizes
e, phi, parts = wb.energy(), wb.potential(), wb.particles()
assert len(e) == len(phi) == len(parts) == len(sizes)
for b, a in enumerate(members):
    w = nb.World(a)
    want = w.particles()
    assert wb.member(b).tobytes() == want.tobytes() == parts[b].tobytes(), b
    m = int((want[:, 6] > 0).sum())
    assert (want[:m, 6] > 0).all() and not (want[m:, 6] > 0).any()
    assert e[b] == w.energy(), (b, e[b], w.energy())
    assert phi[b].shape == (sizes[b],) and phi[b].tobytes() == w.potential().tobytes(), b
    w.close()
wb.update_gpu(0.01, 0)          # n = 0: a no-op that touches no device
wb.close()
print("OK")
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run(["python", "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout, r.stderr)


# ---- static ISA of the new kernels -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp("ragged_isa")
    return {src: compile_isa(d, src) for src in ("kernels.hip", "batch_diag.hip", "convert.hip")}


def _ragged(name):
    """by the parameter type in the mangled name (RaggedParams, RaggedDiagParams, RaggedRecords), or ragged_copy_rows_kernel"""
    return "ragged" in name.lower()


def _meta(text):
    return {n: (scratch, sgpr, vgpr) for n, scratch, sgpr, vgpr in kernel_meta(text) if _ragged(n)}


def _phi_body(text):
    """the instruction lines of ensemble_phi_kernel<RaggedDiagParams>"""
    (name,) = _meta(text)
    lines = text[text.index(name + ":"):].split(".Lfunc_end")[0].splitlines()[1:]
    body = [ln.split(";")[0].strip() for ln in lines if ln.startswith("\t")]
    return [ln for ln in body if ln and not ln.startswith(".")]


def test_the_new_kernels_exist_and_are_not_mistaken_for_the_uniform_ones(isa):
    step = sorted(_meta(isa["kernels.hip"]))
    assert len(step) == 4 and sum("batch_lane_split_kernel" in n for n in step) == 2, step
    assert any("batch_chain_kernel" in n for n in step) and any("batch_trace_chain_kernel" in n for n in step)
    # tests/test_batch_cpu.py selects the uniform instantiations by their parameter type, tests/test_isa.py step kernels by name
    assert not _batch(step) and not [n for n in step if "step_kernel" in n]
    assert len(_meta(isa["batch_diag.hip"])) == 1 and "ensemble_phi_kernel" in next(iter(_meta(isa["batch_diag.hip"])))
    assert len(kernel_meta(isa["batch_diag.hip"])) == 3          # beside the two of the uniform ensemble
    convert = sorted(_meta(isa["convert.hip"]))
    assert len(convert) == 3, convert
    assert [sum(k in n for n in convert) for k in ("batch_split_kernel", "batch_merge_kernel", "ragged_copy_rows_kernel")] == [1, 1, 1]


def test_the_new_kernels_fit_their_launch_bounds_without_scratch(isa):
    for name, (scratch, sgpr, vgpr) in _meta(isa["kernels.hip"]).items():
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert sgpr <= 102, (name, sgpr)
        # 512 VGPRs per SIMD lane, waves of a workgroup spread over 4 SIMDs: a W-wave workgroup must fit once
        waves = 16 if "chain_kernel" in name else int(re.search(r"kernelILi(\d+)ELi\d+E", name).group(1))
        assert vgpr <= 512 // ((waves + 3) // 4), (name, vgpr)
    for src in ("batch_diag.hip", "convert.hip"):
        for name, (scratch, sgpr, vgpr) in _meta(isa[src]).items():
            assert scratch == 0 and sgpr <= 102, (name, scratch, sgpr)
            assert vgpr <= 64, (name, vgpr)      # 256-thread workgroups at full occupancy
    assert not re.search(r"^\s+scratch_", isa["batch_diag.hip"], re.M)


def test_the_new_step_kernels_keep_the_wait_state_behind_every_rsq(isa):
    fns = functions(isa["kernels.hip"])
    names = [n for n in fns if _ragged(n)]
    assert len(names) == 4, names
    for name in names:
        total = check_rsq_wait_states(name, fns[name])
        assert total >= 5, (name, total)


def test_the_ragged_potential_kernel_keeps_the_scalar_route_and_the_wait_state(isa):
    """ensemble_phi_kernel<RaggedDiagParams> is the potential half of the uniform one: sources through the scalar cache, one
    wait state behind every v_rsq_f32, no LDS."""
    body = _phi_body(isa["batch_diag.hip"])
    ops = [ln.split()[0] for ln in body]
    assert "s_load_dwordx16" in ops and "s_load_dwordx8" in ops
    assert not [o for o in ops if o.startswith("ds_")]
    rsq = [i for i, o in enumerate(ops) if o.startswith("v_rsq_f32")]
    assert len(rsq) >= 16
    for i in rsq:
        dest = re.match(r"v_rsq_f32(?:_e\d+)?\s+(v\d+)", body[i]).group(1)
        assert not (ops[i + 1].startswith("v_") and not ops[i + 1].startswith("v_rsq_f32")
                    and re.search(r"\b%s\b" % dest, body[i + 1])), body[i:i + 2]
