"""Leapfrog (kick-drift-kick) steps (include/nbody_leapfrog.h) without a GPU: UpdateWorld_CPU_Leapfrog against the composition
from public calls bit for bit (tests/leapfrog_ref.py), the mutants a checker must reject, the acc-current flag, the order
of the scheme on a two-body orbit, the argument checks, the header / binding / export agreement and static checks on the
ISA of nbody_amd/csrc/leapfrog.hip.  Every child process hides the devices."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import leapfrog_ref as lr
import nbody_amd as nb
from isa_common import compile_isa, functions, kernel_meta
from test_abi import declared_functions, exported

ROOT = nb.ROOT
HIDDEN = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
WORLD_FUNCS = ["UpdateWorld_GPU_Leapfrog", "UpdateWorld_CPU_Leapfrog", "UpdateWorldBatch_GPU_Leapfrog", "UpdateWorldBatch_GPU_Leapfrog_dts"]
HIP_FUNCS = ["nb_hip_leapfrog_steps", "nb_hip_leapfrog_steps_async", "nb_hip_ensemble_leapfrog", "nb_hip_ensemble_leapfrog_dts"]
HOOKS = ["nb_hip_last_leapfrog_info", "nb_hip_ensemble_last_leapfrog_info"]
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")
DT = 0.01


def cpu_force(p):
    """update_cpu(0, 1) of a World holding exactly these particles (massive first, so the partition keeps the order)."""
    w = nb.World(p)
    assert w.particles()[:, 6:8].tobytes() == np.ascontiguousarray(p[:, 6:8]).tobytes()
    w.update_cpu(0.0, 1)
    out = w.particles()
    w.close()
    return out


def massless_tail():
    """40 massive particles on a jittered ring and 9 massless ones among them, with velocities."""
    rng = np.random.default_rng(11)
    a = np.zeros((49, 8), dtype=np.float32)
    phi = rng.random(49) * 2.0 * math.pi
    a[:, 0], a[:, 1] = np.cos(phi) * (1.0 + rng.random(49)), np.sin(phi) * (1.0 + rng.random(49))
    a[:, 2:4] = rng.standard_normal((49, 2)) * 0.1
    a[:40, 6] = 0.01 * (0.5 + rng.random(40))
    a[:, 7] = 1.0e-3
    return a


def partitioned(ic):
    """The World's own order of these particles (massive first): a World made from it keeps it."""
    w = nb.World(ic)
    p = w.particles()
    w.close()
    return p


@pytest.fixture(scope="module")
def worlds(golden):
    return {"ic_333": partitioned(golden("ic_333.bin")), "ic_4096": partitioned(golden("ic_4096.bin")), "massless tail": massless_tail()}


@pytest.fixture(scope="module")
def composed(worlds):
    """The composition of 1, 2, 3 and 5 steps of every world, computed once."""
    return {(name, n): lr.compose(cpu_force, ic, [DT] * n) for name, ic in worlds.items() for n in (1, 2, 3, 5)}


def cpu_leapfrog(ic, calls, dt=DT):
    w = nb.World(ic)
    for n in calls:
        w.update_cpu_leapfrog(dt, n)
    p = w.particles()
    w.close()
    return p


# ---- 1. the host path equals the composition bit for bit -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ic_333", "ic_4096", "massless tail"])
def test_cpu_leapfrog_equals_the_composition_bitwise(worlds, composed, name):
    ic = worlds[name]
    for n in (1, 3):
        got = cpu_leapfrog(ic, [n])
        assert lr.same_bits(got, composed[name, n]), (name, n, lr.differing(got, composed[name, n]))
    got = cpu_leapfrog(ic, [2, 3])
    assert lr.same_bits(got, composed[name, 5]), (name, "2 + 3", lr.differing(got, composed[name, 5]))
    assert lr.same_bits(cpu_leapfrog(ic, [5]), composed[name, 5])
    if name != "ic_333":
        assert np.any(ic[:, 6] == 0) and np.any(got[ic[:, 6] == 0, 0:2] != ic[ic[:, 6] == 0, 0:2])   # massless ones move too


@pytest.mark.parametrize("name", ["ic_333", "ic_4096", "massless tail"])
def test_the_checker_rejects_every_mutant(worlds, composed, name):
    ic = worlds[name]
    got = cpu_leapfrog(ic, [3])
    told = {}
    for m in lr.MUTANTS:
        wrong = lr.compose(cpu_force, ic, [DT] * 3, mutant=m)
        told[m] = lr.differing(got, wrong)
    print(f"[leapfrog mutants] {name}: particles whose bits a mutant changes: " + "  ".join(f"{m} {c}" for m, c in told.items()))
    assert all(c > 0 for c in told.values()), told
    # an unprimed composition (the caller's acc taken for the state's own) is told apart as well
    assert not lr.same_bits(got, lr.compose(cpu_force, ic, [DT] * 3, prime=False))


def test_an_euler_update_clears_the_flag_so_the_next_call_primes_again(worlds):
    ic = worlds["ic_333"]
    w = nb.World(ic)
    w.update_cpu_leapfrog(DT, 2)
    w.update_cpu(DT, 1)
    mid = w.particles()
    w.update_cpu_leapfrog(DT, 2)
    got = w.particles()
    w.close()
    assert lr.same_bits(got, lr.compose(cpu_force, mid, [DT] * 2, prime=True))
    assert not lr.same_bits(got, lr.compose(cpu_force, mid, [DT] * 2, prime=False))
    # a dt = 0 Euler update clears it too; two leapfrog calls in a row do not prime in between
    w = nb.World(ic)
    w.update_cpu_leapfrog(DT, 1)
    w.update_cpu_leapfrog(DT, 1)
    assert lr.same_bits(w.particles(), lr.compose(cpu_force, ic, [DT] * 2))
    w.close()


def test_cpu_adaptive_leapfrog_logs_the_criterion_of_each_state_and_replays(worlds):
    import timestep_ref as tr
    ic = worlds["ic_333"]
    w = nb.World(ic)
    log, res = w.update_cpu_adaptive(2, 0.1, 0.5, leapfrog=True)
    w.close()
    span = float(log[0]) + 0.5 * float(log[1])
    w = nb.World(ic)
    log, res = w.update_cpu_adaptive(4, 0.1, 0.5, span=span, leapfrog=True)
    got = w.particles()
    w.close()
    assert res["elapsed"] == span and res["steps"] == 2 and res["idle_steps"] == 2 and not log[2:].any()
    r, clock = nb.World(ic), tr.Clock(span)
    r.update_cpu(0.0, 1)                      # the implied prime, once
    for i in range(4):
        want = clock.step(tr.timestep(r.particles(), 0.1, 0.5))
        assert np.float32(want).tobytes() == log[i].tobytes(), (i, want, log[i])
        r.update_cpu_leapfrog(float(log[i]), 1)
    assert lr.same_bits(got, r.particles()) and res == clock.result()
    r.close()
    assert log[0] < np.float32(0.5)           # the criterion saw the state's own acc, not the fresh world's zeros


# ---- 2. the order of the scheme on a two-body orbit --------------------------------------------------------------------------

def two_body(e):
    """Equal masses, G (m1 + m2) = a = 1 with G = NB_G, at apocentre; one period is 2 pi (as in tests/test_adaptive_cpu.py)."""
    r, m = 1.0 + e, 0.5 / nb.NB_G
    v = math.sqrt(2.0 / r - 1.0)
    a = np.zeros((2, 8), dtype=np.float32)
    a[0, 0], a[1, 0] = -r / 2, r / 2
    a[0, 3], a[1, 3] = -v / 2, v / 2
    a[:, 6], a[:, 7] = m, 1.0e-6
    return a


def worst_drift(ic, dts, leapfrog):
    """max |dE/E| after every step (float32 state, float64 energies)."""
    w = nb.World(ic)
    w.update_cpu(0.0, 1)
    e0, worst = w.energy()["total"], 0.0
    for dt in dts:
        if leapfrog:
            w.update_cpu_leapfrog(float(dt), 1)
        else:
            w.update_cpu(float(dt), 1)
        worst = max(worst, abs(w.energy()["total"] - e0) / abs(e0))
    w.close()
    return worst


PERIOD = 2.0 * math.pi


def test_two_body_e05_leapfrog_is_second_order_and_euler_first():
    """e = 0.5, one period in 359, 718 and 1 436 steps.  Measured here: leapfrog max |dE/E| 8.12e-4, 2.00e-4, 5.21e-5 (ratios
    4.07, 3.83); Euler 2.48e-2, 1.23e-2, 6.12e-3 (ratios 2.01, 2.02)."""
    ic = two_body(0.5)
    kdk = [worst_drift(ic, [np.float32(PERIOD / n)] * n, True) for n in (359, 718, 1436)]
    euler = [worst_drift(ic, [np.float32(PERIOD / n)] * n, False) for n in (359, 718, 1436)]
    print("[two-body e=0.5] leapfrog " + " ".join(f"{x:.3e}" for x in kdk) + f"  ratios {kdk[0] / kdk[1]:.2f} {kdk[1] / kdk[2]:.2f}")
    print("[two-body e=0.5] euler    " + " ".join(f"{x:.3e}" for x in euler) + f"  ratios {euler[0] / euler[1]:.2f} {euler[1] / euler[2]:.2f}")
    for a, b in ((kdk[0], kdk[1]), (kdk[1], kdk[2])):
        assert 3.0 <= a / b <= 5.0, kdk
    for a, b in ((euler[0], euler[1]), (euler[1], euler[2])):
        assert 1.7 <= a / b <= 2.3, euler


def test_two_body_e09_fixed_leapfrog_beats_euler():
    """e = 0.9, 1 436 fixed steps over one period.  Measured here: leapfrog 0.0443, Euler 0.4902, ratio 0.090."""
    ic, n = two_body(0.9), 1436
    dts = [np.float32(PERIOD / n)] * n
    kdk, euler = worst_drift(ic, dts, True), worst_drift(ic, dts, False)
    print(f"[two-body e=0.9] {n} fixed steps: leapfrog {kdk:.4f}  euler {euler:.4f}  ratio {kdk / euler:.3f}")
    assert kdk < 0.2 * euler, (kdk, euler)


def test_two_body_e09_adaptive_leapfrog():
    """e = 0.9, eta = 0.1, dt_max = 1, span one period, leapfrog=True.  Measured here: 1 405 steps, max |dE/E| 3.5e-4."""
    ic = two_body(0.9)
    w = nb.World(ic)
    log, res = w.update_cpu_adaptive(4000, 0.1, 1.0, span=PERIOD, leapfrog=True)
    w.close()
    steps = res["steps"]
    assert res["elapsed"] == PERIOD and res["steps"] + res["idle_steps"] == 4000
    assert log[:steps].all() and not log[steps:].any()
    drift = worst_drift(ic, log[:steps], True)
    print(f"[two-body e=0.9] adaptive leapfrog: {steps} steps, max |dE/E| {drift:.3e}")
    assert 1000 < steps < 2000, steps
    assert drift < 0.01, drift


# ---- 3. argument checks ------------------------------------------------------------------------------------------------------

def child(code, **env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **HIDDEN)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
         "w = nb.World(a); L = nb.nbody_lib(); inf = float('inf'); nan = float('nan')\n"
         "s = nb.SimPipeline(4, 4); b = nb.SimBatch(4, [4, 4]); wb = nb.WorldBatch(np.stack([a, a]))\n")
SHARDED = "fn = nb.ALLGATHER_FN(lambda *x: None); ws = nb.World.__new__(nb.World); ws._h = L.CreateWorldShardedWith(a.ctypes.data, 4, 0, 2, fn, None); "
SHARDED_PIPE = "fn = lambda *x: None; sp = nb.SimPipeline(4, 4, rank=0, nranks=2, allgather=fn); "
ABORTS = [
    ("sharded pipeline", SHARDED_PIPE + "sp.update_leapfrog(1, 0.1)", "nb_hip_leapfrog_steps of a sharded pipeline needs a collective"),
    ("sharded pipeline async", SHARDED_PIPE + "sp.update_leapfrog_async(1, 0.1)", "nb_hip_leapfrog_steps_async of a sharded pipeline needs a collective"),
    ("sharded pipeline adaptive", SHARDED_PIPE + "sp.update_adaptive(1, 0.1, 1.0, leapfrog=True)", "nb_hip_adaptive_steps of a sharded pipeline needs a collective"),
    ("sharded world", SHARDED + "ws.update_gpu_leapfrog(0.1, 1)", "UpdateWorld_GPU_Leapfrog of a sharded pipeline needs a collective"),
    ("sharded world advance", SHARDED + "ws.advance_gpu(1.0, 0.1, 1.0, leapfrog=True)", "AdvanceWorld_GPU of a sharded pipeline needs a collective"),
    ("ragged ensemble", "r = nb.SimBatch.ragged([4, 3], [4, 3]); r.update_leapfrog(1, 0.1)", "nb_hip_ensemble_leapfrog: leapfrog steps of ragged ensembles"),
    ("ragged ensemble dts", "r = nb.SimBatch.ragged([4, 3], [4, 3]); r.update_leapfrog(1, [0.1, 0.2])",
     "nb_hip_ensemble_leapfrog_dts: leapfrog steps of ragged ensembles"),
    ("ragged ensemble adaptive", "r = nb.SimBatch.ragged([4, 3], [4, 3]); r.update_adaptive(1, 0.1, 1.0, leapfrog=True)",
     "nb_hip_ensemble_adaptive_steps: adaptive steps of ragged ensembles"),
    ("ragged batch", "r = nb.WorldBatch.ragged([a, a[:3]]); r.update_gpu_leapfrog(0.1, 1)", "UpdateWorldBatch_GPU_Leapfrog: leapfrog steps of ragged ensembles"),
    ("ragged batch dts", "r = nb.WorldBatch.ragged([a, a[:3]]); r.update_gpu_leapfrog([0.1, 0.2], 1)",
     "UpdateWorldBatch_GPU_Leapfrog_dts: leapfrog steps of ragged ensembles"),
    ("before set_data", "s.update_leapfrog(1, 0.1)", "nb_hip_leapfrog_steps before SetSimulationData"),
    ("batch before set_data", "b.update_leapfrog(1, 0.1)", "nb_hip_ensemble_leapfrog before nb_hip_batch_set_data"),
    ("NULL pipeline", "nb.hip_lib().nb_hip_leapfrog_steps(None, 1, 0.1)", "nb_hip_leapfrog_steps: NULL argument"),
    ("NULL batch dts", "nb.hip_lib().nb_hip_ensemble_leapfrog_dts(b._h, 1, None)", "nb_hip_ensemble_leapfrog_dts: NULL argument"),
    ("NULL world", "L.UpdateWorld_CPU_Leapfrog(None, 0.1, 1)", "UpdateWorld_CPU_Leapfrog: NULL argument"),
    ("NULL world gpu", "L.UpdateWorld_GPU_Leapfrog(None, 0.1, 1)", "UpdateWorld_GPU_Leapfrog: NULL argument"),
    ("eta 0 with the flag", "w.update_cpu_adaptive(1, 0.0, 1.0, leapfrog=True)", "UpdateWorld_CPU_Adaptive: eta must be finite and > 0"),
    ("dt_max inf with the flag", "s.update_adaptive(1, 0.1, inf, leapfrog=True)", "nb_hip_adaptive_steps: dt_max must be finite and > 0"),
    ("span 0 with the flag", "b.update_adaptive(1, 0.1, 1.0, span=0.0, leapfrog=True)", "nb_hip_ensemble_adaptive_steps: span must be > 0"),
    ("dt_min above dt_max with the flag", "wb.advance_gpu(1.0, 0.1, 1.0, dt_min=2.0, leapfrog=True)", "AdvanceWorldBatch_GPU: dt_min must be within [0, dt_max]"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_calls_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


def test_no_steps_do_nothing_and_open_no_device():
    code = (SETUP +
            "import os\n"
            "before = w.particles().tobytes()\n"
            "w.update_cpu_leapfrog(0.1, 0); w.update_gpu_leapfrog(0.1, 0); s.update_leapfrog(0, 0.1); s.update_leapfrog_async(0, 0.1)\n"
            "b.update_leapfrog(0, 0.1); b.update_leapfrog(0, [0.1, 0.2]); wb.update_gpu_leapfrog(0.1, 0); wb.update_gpu_leapfrog([0.1, 0.2], 0)\n"
            "zero = {'elapsed': 0.0, 'steps': 0, 'idle_steps': 0, 'dt_last': 0.0, 'dt_smallest': 0.0}\n"
            "out = [w.update_cpu_adaptive(0, 0.1, 1.0, leapfrog=True), w.update_gpu_adaptive(0, 0.1, 1.0, leapfrog=True),\n"
            "       s.update_adaptive(0, 0.1, 1.0, leapfrog=True)]\n"
            "assert all(log.shape == (0,) and res == zero for log, res in out), out\n"
            "assert s.last_leapfrog_info() == (0, False) and b.last_leapfrog_info() == (0, False)\n"
            "assert w.particles().tobytes() == before\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK')\n")
    r = child(code)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.stdout, r.stderr)


# ---- 4. sources, headers, exports ------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_leapfrog.h") == WORLD_FUNCS and set(WORLD_FUNCS) <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        have = exported(os.path.join(nb.LIB_DIR, so))
        assert set(WORLD_FUNCS) <= have and not {"nb_cpu_leapfrog_open", "nb_cpu_leapfrog_close"} & have, so
    assert set(HIP_FUNCS) <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and set(HIP_FUNCS) <= exported(nb.HIP_SO)
    public = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert 'dlsym\n * "nb_hip_leapfrog_steps"' in public or 'dlsym "nb_hip_leapfrog_steps"' in public
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    tuning = open(os.path.join(csrc, "nbody_hip_tuning.h")).read()
    for hook in HOOKS:
        assert hook in nb.TUNE_API and hook in exported(nb.HIP_SO) and re.search(r"\b%s\s*\(" % hook, tuning), hook
        assert not re.search(r"\b%s\s*\(" % hook, public), hook
    assert nb.NB_ADAPT_LEAPFROG == 4 and re.search(r"#define NB_ADAPT_LEAPFROG 4u", open(os.path.join(ROOT, "include", "nbody_adaptive.h")).read())
    assert nb.adaptive_cfg(0.1, 1.0, leapfrog=True).flags == 4 and nb.adaptive_cfg(0.1, 1.0, prime=True, resume=True, leapfrog=True).flags == 7
    import inspect
    for cls, methods in ((nb.SimPipeline, ("update_leapfrog", "update_leapfrog_async")), (nb.SimBatch, ("update_leapfrog",)),
                         (nb.World, ("update_gpu_leapfrog", "update_cpu_leapfrog")), (nb.WorldBatch, ("update_gpu_leapfrog",))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)
    for cls, methods in ((nb.SimPipeline, ("update_adaptive", "update_adaptive_async")), (nb.SimBatch, ("update_adaptive",)),
                         (nb.World, ("update_gpu_adaptive", "update_cpu_adaptive", "advance_gpu")),
                         (nb.WorldBatch, ("update_gpu_adaptive", "advance_gpu"))):
        for m in methods:
            assert inspect.signature(getattr(cls, m)).parameters["leapfrog"].default is False, (cls, m)
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\bleapfrog\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*\bleapfrog_cpu\.c", make, re.M)
    assert re.search(r"^WORLD_HDRS\s*:=.*leapfrog_common\.h", make, re.M) and "include/nbody_leapfrog.h" in make
    for src in ("leapfrog.hip", "leapfrog_cpu.c", "world.c"):
        assert '#include "leapfrog_common.h"' in open(os.path.join(csrc, src)).read(), src
    # the statement is written once: the passes call it, nobody restates a half kick
    for src in ("leapfrog.hip", "leapfrog_cpu.c"):
        text = open(os.path.join(csrc, src)).read()
        assert "nb_leapfrog_kick(" in text and "nb_leapfrog_half(" in text and "0.5f" not in text, src


# ---- 5. static ISA of leapfrog.hip -----------------------------------------------------------------------------------------

KERNELS = ("leapfrog_kernel", "ensemble_leapfrog_kernel")
FORMS = ("ILb1ELb1EE", "ILb1ELb0EE", "ILb0ELb1EE")     # <CLOSE, OPEN>: both, close alone, open alone


@pytest.fixture(scope="module")
def leapfrog_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("leapfrog_isa"), "leapfrog.hip")


def test_leapfrog_kernels_use_no_scratch_no_lds_no_atomics_and_no_fma(leapfrog_isa):
    meta = {n: (scratch, sgpr, vgpr) for n, scratch, sgpr, vgpr in kernel_meta(leapfrog_isa)}
    lds = {name: int(size) for size, name in re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)", leapfrog_isa)}
    bodies = functions(leapfrog_isa)
    for k in KERNELS:
        for form in FORMS:
            names = [n for n in meta if re.search(r"\d%s%s" % (k, form), n)]
            assert len(names) == 1, (k, form, sorted(meta))
            scratch, sgpr, vgpr = meta[names[0]]
            print(f"[leapfrog isa] {names[0]}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs, {lds[names[0]]} bytes of LDS")
            assert scratch == 0, f"{names[0]}: {scratch} bytes of scratch"
            assert lds[names[0]] == 0, (names[0], lds[names[0]])
            assert vgpr <= 64 and sgpr <= 102, (names[0], sgpr, vgpr)       # 256 threads per workgroup: far inside __launch_bounds__(256)
            body = bodies[names[0]]
            bad = [i for i in body if re.match(r"(v_fma|v_fmac|v_pk_fma|v_mad|ds_|scratch_|buffer_atomic|global_atomic|flat_atomic)", i)]
            assert not bad, (names[0], bad[:4])
            muls = sum(i.startswith(("v_mul_f32", "v_pk_mul_f32")) for i in body)
            adds = sum(i.startswith(("v_add_f32", "v_pk_add_f32")) for i in body)
            assert muls >= 1 and adds >= 1, (names[0], muls, adds)
            # float2 rows: every particle access is a 64-bit global load or store
            assert any(i.startswith("global_load_dwordx2") for i in body) and any(i.startswith("global_store_dwordx2") for i in body), names[0]
