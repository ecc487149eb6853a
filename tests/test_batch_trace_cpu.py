"""Traced ensemble updates without a GPU (nb_hip_ensemble_trace* of include/nbody_hip.h, UpdateWorldBatch_GPU_Traced* of
include/nbody_batch_trace.h): the declared surface and its binding, the record count, the argument checks, and that there
is no CPU fallback."""
import os
import re
import subprocess

import numpy as np
import pytest

import nbody_amd as nb
from test_abi import declared_functions, exported

ROOT = nb.ROOT
HIP_FUNCS = ["nb_hip_ensemble_trace_rows", "nb_hip_ensemble_trace", "nb_hip_ensemble_trace_dts"]
HOOKS = ["nb_hip_ensemble_trace_mode", "nb_hip_ensemble_last_trace_info"]
WORLD_FUNCS = ["UpdateWorldBatch_GPU_Traced", "UpdateWorldBatch_GPU_Traced_dts"]
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")


def test_header_exports_and_binding_agree():
    names = declared_functions("nbody_hip.h")
    assert [n for n in names if "trace" in n] == HIP_FUNCS
    have = exported(nb.HIP_SO)
    assert set(HIP_FUNCS) <= have and set(HIP_FUNCS) <= set(nb.HIP_API)
    # the two tooling hooks: exported, declared in the tuning header, bound, and not in the public header
    tuning = open(os.path.join(ROOT, "nbody_amd", "csrc", "nbody_hip_tuning.h")).read()
    for hook in HOOKS:
        assert hook in have and hook in nb.TUNE_API and re.search(r"\b%s\s*\(" % hook, tuning), hook
        assert hook not in names, hook
    assert declared_functions("nbody_batch_trace.h") == WORLD_FUNCS and set(WORLD_FUNCS) <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        assert set(WORLD_FUNCS) <= exported(os.path.join(nb.LIB_DIR, so)), so
    nb.hip_lib()
    nb.nbody_lib()          # binds every entry or raises
    for f in (nb.SimBatch.trace, nb.SimBatch.trace_mode, nb.SimBatch.last_trace_info, nb.WorldBatch.update_gpu_traced,
              nb.energy_row, nb.trace_rows):
        assert callable(f)
    # no version bump: detected by symbol, and the header says so
    assert nb.hip_lib().nb_hip_version() == 400
    assert 'dlsym "nb_hip_ensemble_trace"' in open(os.path.join(ROOT, "include", "nbody_hip.h")).read()


@pytest.mark.parametrize("n,every,rows", [(0, 1, 1), (7, 1, 8), (10, 3, 4), (3, 10, 1)])
def test_the_record_count_is_one_plus_n_over_every(n, every, rows):
    assert nb.hip_lib().nb_hip_ensemble_trace_rows(n, every) == rows
    assert nb.trace_rows(n, every) == rows


def test_a_row_becomes_the_dict_energy_returns():
    e = nb.WorldEnergy(1.5, -2.5, 3.0, (nb.C.c_double * 2)(4.0, 5.0), 6.0, (nb.C.c_double * 2)(7.0, 8.0))
    row = np.array([1.5, -2.5, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0])
    assert nb.energy_row(row) == e.as_dict()
    assert nb.energy_row(row)["total"] == -1.0 and nb.energy_row(row)["center_of_mass"] == (7.0, 8.0)


# Rows are written through a raw pointer: the buffers below are large enough for a call that would go through.
OUT = "import ctypes as C; out = (nb.WorldEnergy * 64)(); L = nb.hip_lib(); dt = (C.c_float * 2)(0.01, 0.02)\n"
ABORTS = [
    ("every = 0", "nb.SimBatch(10, [3]).trace(4, 0.01, 0)", "every = 0"),
    ("every = 0, per-member dt", "b = nb.SimBatch(10, [3, 4]); L.nb_hip_ensemble_trace_dts(b._h, 4, dt, 0, out)", "every = 0"),
    ("every = 0, record count", "L.nb_hip_ensemble_trace_rows(4, 0)", "every = 0"),
    ("NULL ensemble", "L.nb_hip_ensemble_trace(None, 1, 0.01, 1, out)", "NULL argument"),
    ("NULL rows", "b = nb.SimBatch(10, [3]); L.nb_hip_ensemble_trace(b._h, 1, 0.01, 1, None)", "NULL argument"),
    ("NULL step sizes", "b = nb.SimBatch(10, [3, 4]); L.nb_hip_ensemble_trace_dts(b._h, 1, None, 1, out)", "NULL argument"),
    ("before set_data", "nb.SimBatch(10, [3]).trace(4, 0.01, 2)", "before nb_hip_batch_set_data"),
    ("before set_data, per-member dt", "nb.SimBatch(10, [3, 4]).trace(4, [0.01, 0.02], 2)", "before nb_hip_batch_set_data"),
    # 2^24 + 1 rows of one member; 2^23 + 1 records of two (the check precedes every allocation, host or device)
    ("too many rows", "b = nb.SimBatch(10, [3]); L.nb_hip_ensemble_trace(b._h, 1 << 24, 0.01, 1, out)", "16777217 records x 1 members"),
    ("too many rows, two members", "b = nb.SimBatch(10, [3, 4]); L.nb_hip_ensemble_trace_dts(b._h, 1 << 24, dt, 2, out)",
     "8388609 records x 2 members"),
    ("world batch: every = 0", "import numpy as np; nb.WorldBatch(np.ones((2, 4, 8), np.float32)).update_gpu_traced(0.01, 4, 0)",
     "every = 0"),
    ("world batch: NULL rows", "import numpy as np; w = nb.WorldBatch(np.ones((2, 4, 8), np.float32)); "
     "nb.nbody_lib().UpdateWorldBatch_GPU_Traced(w._h, 0.01, 1, 1, None)", "NULL argument"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = subprocess.run(["python", "-c", "import nbody_amd as nb\n" + OUT + code + "\nprint('SURVIVED')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


def test_the_largest_legal_row_count_passes_the_limit():
    """2^24 rows exactly are legal: the call gets past the limit and stops at the next check (no data yet)."""
    code = ("import nbody_amd as nb\n" + OUT +
            "b = nb.SimBatch(10, [3]); L.nb_hip_ensemble_trace(b._h, (1 << 24) - 1, 0.01, 1, out)\nprint('SURVIVED')")
    r = subprocess.run(["python", "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "before nb_hip_batch_set_data" in r.stderr and "records x" not in r.stderr, r.stderr


def test_a_traced_call_without_a_gpu_aborts_loudly():
    """No CPU fallback: a traced update of a WorldBatch on a box without a GPU must abort, not compute -- also for
    n = 0, whose one row is the device's value."""
    for n in (3, 0):
        code = ("import numpy as np, nbody_amd as nb\n"
                "a = np.zeros((2, 8, 8), dtype=np.float32); a[:, :, 6] = 1; a[:, :, 7] = 1\n"
                f"w = nb.WorldBatch(a); w.update_gpu_traced(0.1, {n}, 1); print('SURVIVED')\n")
        env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
        r = subprocess.run(["python", "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
        assert "no HIP device" in r.stderr or "hipError" in r.stderr, r.stderr
