"""World ensembles without a GPU: the declared surface (include/nbody_hip.h nb_hip_batch_*, include/nbody_batch.h), its
argument checks, the per-member partition of CreateWorldBatch, and the static ISA of the ensemble kernels
(nbody_amd/csrc/kernels.hip batch_chain_kernel, batch_lane_split_kernel: their instantiations for nb::BatchParams, the members
addressed by block index; tests/test_ragged_cpu.py holds the ones for nb::RaggedParams)."""
import os
import re
import subprocess

import numpy as np
import pytest

import nbody_amd as nb
from test_abi import declared_functions, exported
from isa_common import check_rsq_wait_states, compile_isa, functions, kernel_meta

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

BATCH_HIP = ["nb_hip_batch_create", "nb_hip_batch_destroy", "nb_hip_batch_set_data", "nb_hip_batch_get_data",
             "nb_hip_batch_get_member", "nb_hip_batch_update", "nb_hip_batch_update_dts", "nb_hip_batch_step_async",
             "nb_hip_batch_sync", "nb_hip_batch_last_ms", "nb_hip_batch_dt_uploads", "nb_hip_batch_launch_shape"]
BATCH_WORLD = ["CreateWorldBatch", "DestroyWorldBatch", "GetWorldBatchParticles", "UpdateWorldBatch_GPU",
               "UpdateWorldBatch_GPU_dts"]


# ---- surface ---------------------------------------------------------------------------------------------------------

def test_header_exports_and_binding_agree_for_the_hip_library():
    names = declared_functions("nbody_hip.h")
    assert set(BATCH_HIP) <= set(names)
    assert [n for n in names if n.startswith("nb_hip_batch_")] == BATCH_HIP     # nothing undeclared, nothing extra
    have = exported(nb.HIP_SO)
    assert not [n for n in BATCH_HIP if n not in have]
    assert set(BATCH_HIP) <= set(nb.HIP_API)
    assert sorted(n for n in have if n.startswith("nb_hip_batch_")) == sorted(BATCH_HIP)
    nb.hip_lib()          # binds every entry of HIP_API or raises


def test_header_exports_and_binding_agree_for_the_world_library():
    assert declared_functions("nbody_batch.h") == BATCH_WORLD
    assert set(BATCH_WORLD) <= set(nb.NBODY_API)
    for so in ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so"):
        have = exported(os.path.join(nb.LIB_DIR, so))
        assert not [n for n in BATCH_WORLD if n not in have], so
    nb.nbody_lib()


def test_the_pinned_headers_gained_nothing():
    for header in ("nbody.h", "galaxy.h", "nbody_diag.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "Batch" not in text and "batch" not in text, header
        assert not set(declared_functions(header)) & set(BATCH_HIP + BATCH_WORLD), header


def test_no_version_bump_and_the_header_says_so():
    assert nb.hip_lib().nb_hip_version() == 400
    text = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert "WITHOUT a version bump" in text and "by symbol" in text


def test_partition_routine_exists_once():
    """CreateWorld and CreateWorldBatch share one copy of the partition (world_partition.h)."""
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if re.search(r"uint32_t partition_by_mass\(", open(os.path.join(csrc, f)).read())]
    assert defs == ["world_partition.h"]
    for f in ("world.c", "world_batch.c"):
        assert '#include "world_partition.h"' in open(os.path.join(csrc, f)).read()


# ---- no GPU needed -----------------------------------------------------------------------------------------------------

def test_create_and_destroy_touch_no_gpu():
    """create allocates nothing on the device: it works (and reports its shape) on a box without one."""
    for n, m, want in ((1, [0], ("chain", 2, 16, 1, 1)), (250, [0, 250, 17], ("chain", 2, 8, 1, 3)),
                       (512, [5] * 7, ("chain", 2, 4, 1, 7)), (513, [1, 2], ("lanes", 1, 8, 8, 2 * 65)),
                       (1581, [9], ("lanes", 1, 8, 8, 198)), (1582, [9], ("lanes", 1, 16, 4, 99)),
                       (3000, [3000, 0], ("lanes", 1, 16, 4, 2 * 188))):
        b = nb.SimBatch(n, m)
        s = b.launch_shape()
        assert (s["path"], s["k"], s["w"], s["lanes"], s["workgroups"]) == want, (n, s)
        assert b.last_ms() == 0.0 and b.dt_uploads() == 0
        b.sync()             # nothing on the device yet: a no-op
        b.close()
    nb.hip_lib().nb_hip_batch_destroy(None)
    nb.nbody_lib().DestroyWorldBatch(None)


def test_the_lane_split_shape_is_the_auto_rule_at_full_mass():
    """(W, H) of an ensemble is lane_split_rule(N, N): a function of N alone, reachable on a single pipeline through the
    `lanes` / `w` hooks, and defined for every N the ensemble accepts above the chain's 512."""
    for n in (513, 800, 1000, 1581, 1582, 2000, 3000):
        b = nb.SimBatch(n, [n // 3])
        s = b.launch_shape()
        plan = nb.plan_launch(n, n)
        assert (s["lanes"], s["w"]) == (plan["lanes"], plan["lanes_w"]) and s["lanes"] > 1, (n, s, plan)
        assert b.pinned_knobs() == dict(lanes=s["lanes"], w=s["w"], fused_chain=0)
        b.close()
    assert nb.plan_launch(3001, 3001)["lanes"] == 1     # the rule's own cut-off is the ensemble's limit


ABORTS = [
    ("count = 0", "nb.SimBatch(10, [])", "count = 0"),
    ("count > 65535", "nb.SimBatch(4, [1] * 65536)", "count 65536 > 65535"),
    ("total_len = 0", "nb.SimBatch(0, [0])", "total_len = 0"),
    ("total_len > 3000", "nb.SimBatch(3001, [5])", "total_len 3001 > 3000"),
    ("mass_len > total_len", "nb.SimBatch(10, [3, 11, 2])", "member 1: mass_len 11 > total_len 10"),
    ("update before set_data", "nb.SimBatch(10, [3]).update(1, 0.01)", "before nb_hip_batch_set_data"),
    ("update_dts before set_data", "nb.SimBatch(10, [3, 4]).update(1, [0.01, 0.02])", "before nb_hip_batch_set_data"),
    ("get before set_data", "nb.SimBatch(10, [3]).get_data()", "before nb_hip_batch_set_data"),
    ("get_member out of range", "nb.SimBatch(10, [3]).get_member(1)", "member 1 of 1"),
    ("world batch of 0 worlds", "import numpy as np; nb.WorldBatch(np.zeros((0, 4, 8), np.float32))", "count 0 outside"),
    ("world batch too large a world", "import numpy as np; nb.WorldBatch(np.zeros((1, 3001, 8), np.float32))", "world_size 3001 outside"),
    ("world batch member out of range", "import numpy as np; nb.WorldBatch(np.ones((2, 4, 8), np.float32)).member(2)", "member 2 of 2"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = subprocess.run(["python", "-c", "import nbody_amd as nb\n" + code + "\nprint('SURVIVED')"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


def test_members_without_sources_and_zero_steps_are_legal():
    b = nb.SimBatch(5, [0, 0])
    b.close()
    wb = nb.WorldBatch(np.zeros((2, 5, 8), np.float32))     # all massless
    wb.update_gpu(0.01, 0)                                   # n = 0 returns before anything is uploaded
    wb.update_gpu([0.01, 0.02], 0)
    assert wb.particles().shape == (2, 5, 8)
    wb.close()


def _worlds(n, fracs, seed):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((len(fracs), n, 8)).astype(np.float32)
    for b, f in enumerate(fracs):
        massive = rng.random(n) < f
        a[b, :, 6] = np.where(massive, 1.0 + rng.random(n), np.where(rng.random(n) < 0.5, 0.0, -1.0)).astype(np.float32)
    return a


@pytest.mark.parametrize("n", [1, 7, 333, 1000])
def test_create_world_batch_partitions_each_member_as_create_world_does(n):
    """GetWorldBatchParticles before any update == World(member).particles(), bytewise: M_b = 0, M_b = N and in between.
    Runs in a child process that hides every GPU: neither constructor nor read may need one."""
    code = f"""
import numpy as np, nbody_amd as nb
from test_batch_cpu import _worlds
a = _worlds({n}, [0.0, 1.0, 0.5, 0.1, 0.9], {n})
assert (a[0, :, 6] > 0).sum() == 0 and (a[1, :, 6] > 0).sum() == {n}
wb = nb.WorldBatch(a)
for b in range(a.shape[0]):
    w = nb.World(a[b])
    want = w.particles(); w.close()
    got = wb.member(b)
    assert got.tobytes() == want.tobytes(), b
    m = int((want[:, 6] > 0).sum())
    assert (got[:m, 6] > 0).all() and not (got[m:, 6] > 0).any()
assert wb.particles().shape == a.shape
wb.update_gpu(0.01, 0)          # n = 0: a no-op that touches no device
wb.close()
print("OK")
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run(["python", "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "OK" in r.stdout, (r.stdout, r.stderr)


# ---- static ISA of the ensemble kernels ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("batch_isa"), "kernels.hip")


def _batch(names):
    """the untraced step kernels whose (mangled) parameter type is nb::BatchParams"""
    return [n for n in names if ("batch_chain_kernel" in n or "batch_lane_split_kernel" in n) and "BatchParams" in n]


def test_ensemble_kernels_keep_the_wait_state_behind_every_rsq(isa):
    fns = functions(isa)
    names = _batch(fns)
    assert len(names) == 3, names          # the chain and the two lane-split shapes the rule reaches
    assert not [n for n in fns if "batch" in n and "step_kernel" in n]   # test_isa.py matches step kernels by name
    for name in names:
        total = check_rsq_wait_states(name, fns[name])
        assert total >= 5, (name, total)


def test_ensemble_kernels_fit_their_launch_bounds_without_scratch(isa):
    rows = {n: (scratch, sgpr, vgpr) for n, scratch, sgpr, vgpr in kernel_meta(isa)}
    names = _batch(rows)
    assert len(names) == 3, names
    for name in names:
        scratch, sgpr, vgpr = rows[name]
        assert scratch == 0, f"{name}: {scratch} bytes of scratch"
        assert sgpr <= 102, (name, sgpr)
        # 512 VGPRs per SIMD lane, waves of a workgroup spread over 4 SIMDs: a W-wave workgroup must fit once
        waves = 16 if "batch_chain_kernel" in name else int(re.search(r"kernelILi(\d+)ELi\d+E", name).group(1))
        assert vgpr <= 512 // ((waves + 3) // 4), (name, vgpr)
