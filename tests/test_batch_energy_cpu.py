"""Energy / potential diagnostics of world ensembles without a GPU: the declared surface (include/nbody_batch_diag.h,
nb_hip_ensemble_* of include/nbody_hip.h), the host path of GetWorldBatchEnergy / GetWorldBatchPotential against the single
World and against float64 numpy, the argument checks, and the static ISA of nbody_amd/csrc/batch_diag.hip."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
from energy_ref import assert_energy_close, energy_f64, phi_f64
from gpu_common import synth
from isa_common import compile_isa
from test_abi import declared_functions, exported
from test_batch_cpu import BATCH_HIP, BATCH_WORLD

ROOT = nb.ROOT
WORLD_FUNCS = ["GetWorldBatchEnergy", "GetWorldBatchPotential"]
HIP_FUNCS = ["nb_hip_ensemble_energy", "nb_hip_ensemble_potential"]
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")


# ---- surface ---------------------------------------------------------------------------------------------------------

def test_the_new_header_declares_exactly_the_two_functions():
    assert declared_functions("nbody_batch_diag.h") == WORLD_FUNCS


def test_header_binding_and_exports_agree():
    assert set(WORLD_FUNCS) <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        have = exported(os.path.join(nb.LIB_DIR, so))
        assert not [n for n in WORLD_FUNCS if n not in have], so
        assert not {"nb_cpu_energy", "nb_cpu_potential"} & have, so      # the host path stays internal
    names = declared_functions("nbody_hip.h")
    assert set(HIP_FUNCS) <= set(names) & set(nb.HIP_API)
    assert set(HIP_FUNCS) <= exported(nb.HIP_SO)
    tuning = open(os.path.join(ROOT, "nbody_amd", "csrc", "nbody_hip_tuning.h")).read()
    assert "nb_hip_ensemble_last_diag_ms" in tuning and "nb_hip_ensemble_last_diag_ms" in nb.TUNE_API
    assert "nb_hip_ensemble_last_diag_ms" in exported(nb.HIP_SO) and "nb_hip_ensemble_last_diag_ms" not in names
    for cls in (nb.SimBatch, nb.WorldBatch):
        assert callable(cls.energy) and callable(cls.potential)
    assert callable(nb.SimBatch.last_diag_ms)
    nb.hip_lib()
    nb.nbody_lib()          # binds every entry or raises


def test_the_pinned_surfaces_are_unchanged():
    assert declared_functions("nbody_batch.h") == BATCH_WORLD
    assert declared_functions("nbody_diag.h") == ["GetWorldEnergy", "GetWorldPotential"]
    assert [n for n in declared_functions("nbody_hip.h") if n.startswith("nb_hip_batch_")] == BATCH_HIP
    assert sorted(n for n in exported(nb.HIP_SO) if n.startswith("nb_hip_batch_")) == sorted(BATCH_HIP)
    for header in ("nbody.h", "galaxy.h", "nbody_diag.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "Batch" not in text and "batch" not in text and "ensemble" not in text, header
    assert nb.hip_lib().nb_hip_version() == 400
    text = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert 'dlsym "nb_hip_ensemble_energy"' in text


def test_the_arithmetic_is_written_once():
    """The pair statement, the eight terms and the row sum live in diag_common.h; both translation units include it."""
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    for needle in ("define NB_PHI_HEAD_ASM", "void block_sum(", "void energy_terms(", "void reduce_rows("):
        assert [f for f in sorted(os.listdir(csrc)) if needle in open(os.path.join(csrc, f), errors="replace").read()] == \
            ["diag_common.h"], needle
    for f in ("diagnostics.hip", "batch_diag.hip"):
        assert '#include "diag_common.h"' in open(os.path.join(csrc, f)).read()
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\bbatch_diag\b", make, re.M)


# ---- host path -------------------------------------------------------------------------------------------------------

def host_ensemble(n, count, seed, fixture=None):
    """(count, n, 8) caller-order particles: M_b = 0, M_b = 1 (where n > 1) and M_b = n among them, the rest mixed; with a
    fixture, every other mixed member is the fixture with its velocities scaled."""
    out = []
    for b in range(count):
        if b == 0:
            a = synth(n, frac_massive=0.0, seed=seed)[0]
        elif b == 1:
            a = synth(n, frac_massive=0.0, seed=seed + 1)[0]
            a[n // 2, 6] = 5.0e3
        elif b == 2:
            a = synth(n, frac_massive=1.0, seed=seed + 2)[0]
        elif fixture is not None and b % 2:
            a = fixture.copy()
            a[:, 2:4] *= np.float32(1.0 + 0.25 * b)
        else:
            a = synth(n, frac_massive=0.15 * b, seed=seed + b)[0][::-1].copy()
        out.append(a)
    return np.stack(out)


def check_host_ensemble(a):
    count, n = a.shape[:2]
    wb = nb.WorldBatch(a)
    energies, phis = wb.energy(), wb.potential()
    parts = wb.particles()
    wb.close()
    assert len(energies) == count and phis.shape == (count, n) and phis.dtype == np.float32
    ms = []
    for b in range(count):
        w = nb.World(a[b])
        e, phi, p = w.energy(), w.potential(), w.particles()
        w.close()
        assert p.tobytes() == parts[b].tobytes()
        assert energies[b] == e, b                              # exactly the single World's host result
        assert phis[b].tobytes() == phi.tobytes(), b
        m = int(np.count_nonzero(p[:, 6] > 0))
        ms.append(m)
        want_phi = phi_f64(p, m)
        assert np.all(np.abs(phis[b].astype(np.float64) - want_phi) <= 6e-8 * np.abs(want_phi) + 1e-300), b
        want, scale = energy_f64(p, m)
        assert_energy_close(energies[b], want, scale)
        if m == 0:
            assert np.all(phis[b] == 0.0) and e["kinetic"] == 0.0 and e["potential"] == 0.0 and e["mass"] == 0.0
        if m == 1:
            assert phis[b][0] == 0.0 and e["potential"] == 0.0
    assert ms[0] == 0 and ms[1] == 1 and ms[2] == n, ms


@pytest.mark.parametrize("n,count", [(1, 3), (65, 4), (333, 5), (1024, 6), (3000, 7)])
def test_host_path_equals_the_single_world_member_by_member(golden, n, count):
    fixture = golden(f"ic_{n}.bin") if n in (333, 1024) else None
    check_host_ensemble(host_ensemble(n, count, seed=10 * n, fixture=fixture))


def test_host_result_does_not_depend_on_the_thread_count():
    code = ("import sys, hashlib, numpy as np, nbody_amd as nb\n"
            "sys.path.insert(0, 'tests')\n"
            "from test_batch_energy_cpu import host_ensemble\n"
            "wb = nb.WorldBatch(host_ensemble(1024, 5, seed=3)); e = wb.energy(); phi = wb.potential()\n"
            "sys.stdout.write(repr([[x['kinetic'], x['potential'], x['angular_momentum'], list(x['momentum'])] for x in e]) + ' ' + "
            "hashlib.sha256(phi.tobytes()).hexdigest())\n")
    outs = []
    for threads in ("1", "4"):
        env = dict(os.environ, OMP_NUM_THREADS=threads,
                   PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout)
    assert outs[0] == outs[1] and len(outs[0]) > 64


def test_a_world_batch_that_never_stepped_opens_no_device():
    code = ("import os, numpy as np, nbody_amd as nb\n"
            "a = np.zeros((3, 64, 8), dtype=np.float32); a[:, :, 0] = np.arange(64); a[:, :, 6] = 1; a[:, :, 7] = 1\n"
            "wb = nb.WorldBatch(a); e = wb.energy(); phi = wb.potential(); wb.update_gpu(0.01, 0); e2 = wb.energy(); wb.close()\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK', all(x['potential'] < 0 for x in e), bool(np.all(phi < 0)), e == e2)\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")     # any device contact would abort
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["OK", "True", "True", "True"]


# ---- argument checks -------------------------------------------------------------------------------------------------

ABORTS = [
    ("energy: NULL out", "nb.hip_lib().nb_hip_ensemble_energy(nb.SimBatch(10, [3])._h, None)", "nb_hip_ensemble_energy: NULL result array"),
    ("potential: NULL phi", "nb.hip_lib().nb_hip_ensemble_potential(nb.SimBatch(10, [3])._h, None)",
     "nb_hip_ensemble_potential: NULL result array"),
    ("energy: NULL ensemble", "import ctypes as C; nb.hip_lib().nb_hip_ensemble_energy(None, C.byref(nb.WorldEnergy()))", "NULL ensemble"),
    ("energy before set_data", "nb.SimBatch(10, [3, 4]).energy()", "nb_hip_ensemble_energy before nb_hip_batch_set_data"),
    ("potential before set_data", "nb.SimBatch(10, [3]).potential()", "nb_hip_ensemble_potential before nb_hip_batch_set_data"),
    ("last_diag_ms: NULL ensemble", "nb.hip_lib().nb_hip_ensemble_last_diag_ms(None)", "NULL ensemble"),
    ("world batch energy: NULL out", "import numpy as np; nb.nbody_lib().GetWorldBatchEnergy(nb.WorldBatch(np.ones((2, 4, 8), np.float32))._h, None)",
     "NULL argument"),
    ("world batch potential: NULL batch", "import numpy as np; nb.nbody_lib().GetWorldBatchPotential(None, np.ones(8, np.float32).ctypes.data)",
     "NULL argument"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_calls_print_file_line_func_and_abort(name, code, needle):
    r = subprocess.run([sys.executable, "-c", "import nbody_amd as nb\n" + code + "\nprint('SURVIVED')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


def test_last_diag_ms_is_zero_before_any_call():
    b = nb.SimBatch(10, [3])
    assert b.last_diag_ms() == 0.0
    b.close()


# ---- static ISA of batch_diag.hip ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("batch_diag_isa"), "batch_diag.hip")


def kernel_metadata(text):
    out = {}
    for block in re.split(r"\n\s+- \.", text.split("amdhsa.kernels:")[1]):
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return out


def basic_blocks(text, symbol):
    body = text[text.index(symbol + ":"):]
    body = body[:body.index(".Lfunc_end")]
    parts = re.split(r"^(\.LBB\d+_\d+):", body, flags=re.M)
    for k in range(1, len(parts), 2):
        lines = [ln.split(";")[0].strip() for ln in parts[k + 1].splitlines()]
        yield parts[k], [ln for ln in lines if ln and not ln.startswith(".")]


def test_ensemble_diagnostics_kernels_have_no_scratch_and_no_spills(isa):
    meta = kernel_metadata(isa)
    uniform = [n for n in meta if "RaggedDiagParams" not in n]    # the third is tests/test_ragged_cpu.py's
    assert len(uniform) == 2 and len(meta) == 3, meta
    assert any("ensemble_phi_kernel" in n for n in uniform) and any("ensemble_reduce_kernel" in n for n in uniform), meta
    assert not any("potential_kernel" in n or "step_kernel" in n for n in meta)     # other ISA tests match those names
    for name, m in meta.items():
        print(f"[batch_diag isa] {name}: {m['vgpr_count']} VGPRs, {m['sgpr_count']} SGPRs, "
              f"{m['group_segment_fixed_size']} bytes of LDS, workgroups of up to {m['max_flat_workgroup_size']}")
        assert m["private_segment_fixed_size"] == 0, name
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0, name
        assert not re.search(r"^\s+scratch_", isa, re.M)
        # four waves per workgroup, one per SIMD: 512 VGPRs each would do; 8 waves per SIMD need <= 64
        if "ensemble_phi_kernel" in name:
            assert m["vgpr_count"] <= 64 and m["sgpr_count"] <= 102, m
            assert m["max_flat_workgroup_size"] == 256 and m["group_segment_fixed_size"] == 0


def test_ensemble_diagnostics_write_memory_with_vector_stores_only(isa):
    ops = {ln.split()[0] for ln in isa.splitlines() if ln.startswith("\t") and ln.strip() and not ln.strip().startswith((".", ";"))}
    writes = {op for op in ops if "store" in op or "atomic" in op}
    assert writes and all(op.startswith(("global_", "ds_", "buffer_", "flat_")) for op in writes), writes
    assert not [op for op in ops if "atomic" in op], ops        # and no atomics at all: every sum has a fixed order


def test_ensemble_potential_loop_is_five_valu_and_one_rsq_per_pair(isa):
    sym = next(n for n in kernel_metadata(isa) if "ensemble_phi_kernel" in n and "RaggedDiagParams" not in n)
    loops = []
    for label, ins in basic_blocks(isa, sym):
        ops = [i.split()[0] for i in ins]
        if any(label in i for i in ins if i.startswith("s_cbranch") or i.startswith("s_branch")) and "v_rsq_f32" in " ".join(ops):
            loops.append((label, ops))
    plain = [(lab, ops) for lab, ops in loops if not any(o.startswith("v_cndmask") for o in ops)]
    masked = [(lab, ops) for lab, ops in loops if any(o.startswith("v_cndmask") for o in ops)]
    assert plain and masked, loops   # the unmasked loop and the loop over the wave's own 128 indices are separate
    ops = max(plain, key=lambda x: x[1].count("v_rsq_f32"))[1]
    rsq = sum(o.startswith("v_rsq_f32") for o in ops)
    other = [o for o in ops if o.startswith("v_") and not o.startswith("v_rsq_f32")]
    assert rsq == 16, ops              # 8 sources x 2 receivers per lane
    assert len(other) <= 5 * rsq, (len(other), sorted(set(other)))
    assert not [o for o in other if o.startswith("v_pk_")], other
    # sources arrive through the scalar cache, never as vector loads inside the loop
    assert "s_load_dwordx16" in ops and "s_load_dwordx8" in ops
    for lab, body in loops:
        assert not [o for o in body if o.startswith(("global_load", "buffer_load", "flat_load", "ds_"))], lab
    # gfx950: one wait state between v_rsq_f32 and the instruction that reads its result, in every loop
    for lab, body in loops:
        for i, o in enumerate(body):
            if o.startswith("v_rsq_f32"):
                assert body[i + 1].startswith("s_"), (lab, body[i:i + 3])
