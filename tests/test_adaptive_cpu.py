"""Adaptive time steps (include/nbody_adaptive.h) without a GPU: the host criterion against its exact numpy restatement
(tests/timestep_ref.py) bit for bit, UpdateWorld_CPU_Adaptive against the loop it stands for, the span clip, an eccentric
two-body orbit, the argument checks, the header / binding / export agreement and static checks on the ISA of
nbody_amd/csrc/timestep.hip.  Every child process hides the devices."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nbody_amd as nb
import timestep_cases as tc
import timestep_ref as tr
from isa_common import compile_isa, kernel_meta
from test_abi import declared_functions, exported

ROOT = nb.ROOT
HIDDEN = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
WORLD_FUNCS = ["UpdateWorld_GPU_Adaptive", "UpdateWorld_CPU_Adaptive", "GetWorldTimestep", "AdvanceWorld_GPU",
               "UpdateWorldBatch_GPU_Adaptive", "AdvanceWorldBatch_GPU"]
HIP_FUNCS = ["nb_hip_adaptive_steps", "nb_hip_adaptive_steps_async", "nb_hip_adaptive_collect", "nb_hip_timestep",
             "nb_hip_ensemble_adaptive_steps"]
WORLD_LIBS = ("libnbody.so", "libnbody_sse.so", "libnbody_scalar.so", "libnbody_f64.so")
ETA = 0.1


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


def host_dt(particles, eta, dt_max, dt_min=0.0):
    """GetWorldTimestep of a CPU-only World holding exactly these particles (massive first, so the partition keeps the order)."""
    w = nb.World(particles)
    assert w.particles().tobytes() == np.ascontiguousarray(particles, dtype=np.float32).tobytes()
    dt = w.timestep(eta, dt_max, dt_min)
    w.close()
    return np.float32(dt)


def state_333(golden):
    w = nb.World(golden("ic_333.bin"))
    w.update_cpu(0.01, 3)
    p = w.particles()
    w.close()
    return p


def small(n, seed):
    """n massive particles with accelerations as a step would leave them (any values do: the criterion only reads them)."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((n, 2))
    a[:, 4:6] = rng.standard_normal((n, 2)) * 3.0
    a[:, 6] = 1.0
    a[:, 7] = 0.5 + rng.random(n)
    return a


# ---- 1. the host criterion equals the restatement bit for bit -------------------------------------------------------------

def criterion_cases(golden):
    p333 = state_333(golden)
    for name, base in (("n1", small(1, 1)), ("n7", small(7, 2)), ("n333", p333)):
        n = base.shape[0]
        yield name + " as it is", base, ETA, 1.0e3, 0.0
        first, last = base.copy(), base.copy()
        first[0, 4:6], first[0, 7] = (4.0e4, -3.0e4), 1.0e-6
        last[n - 1, 4:6], last[n - 1, 7] = (4.0e4, -3.0e4), 1.0e-6
        yield name + " minimum in the first particle", first, ETA, 1.0e3, 0.0
        yield name + " minimum in the last particle", last, ETA, 1.0e3, 0.0
        zero = base.copy()
        zero[n // 2, 4:6] = 0.0
        yield name + " a particle with acc = 0", zero, ETA, 1.0e3, 0.0
        nan = base.copy()
        nan[n // 2, 4] = np.nan
        yield name + " a NaN acc", nan, ETA, 1.0e3, 0.0
        r0 = base.copy()
        r0[n - 1, 7] = 0.0
        if not np.any(r0[n - 1, 4:6]):
            r0[n - 1, 4:6] = (1.0, 2.0)
        yield name + " radius = 0 gives dt_min", r0, ETA, 1.0e3, 3.0e-5
        skipped = base.copy()
        skipped[:, 4:6] = 0.0
        skipped[0, 4] = np.inf
        yield name + " every particle skipped gives dt_max", skipped, ETA, 0.125, 0.0
        yield name + " clamped from above", base, ETA, 1.0e-9, 0.0
        yield name + " clamped from below", base, ETA, 2.0e3, 1.0e3


def test_host_criterion_equals_the_restatement_bit_for_bit(golden):
    seen = 0
    for name, p, eta, dt_max, dt_min in criterion_cases(golden):
        got, want = host_dt(p, eta, dt_max, dt_min), tr.timestep(p, eta, dt_max, dt_min)
        assert bits(got) == bits(want), (name, got, want)
        if "gives dt_min" in name or "from below" in name:
            assert got == np.float32(dt_min), name
        if "gives dt_max" in name or "from above" in name:
            assert got == np.float32(dt_max), name
        if "minimum in" in name:
            j = 0 if "first" in name else p.shape[0] - 1
            assert int(np.argmin(tr.q_all(p))) == j and np.float32(dt_min) < got < np.float32(dt_max), name
        seen += 1
    assert seen == 27


def test_case_tables_tell_the_statement_from_its_mutants():
    """tests/timestep_cases.py: over sweep(4096) + directed() every wrong statement (a)-(d) changes the dt bits of at least 50
    cases, and the -0.0 and negative-radius cases tell (e) apart in a two-particle world.  This is what keeps the device sweep
    of tests/test_gpu_adaptive_edges.py from passing vacuously; a seed that misses it is a reason to change the generator."""
    cases = np.concatenate([tc.sweep(4096), tc.directed()])
    cfg = dict(eta=1.0, dt_max=3.0e38, dt_min=0.0)
    want = tc.expected(cases, **cfg)
    assert bits(tc.mutant_dt(cases, None, **cfg)) == bits(want)          # the vectorised real statement is the restatement
    counts = {m: int(np.sum(tc.mutant_dt(cases, m, **cfg).view(np.uint32) != want.view(np.uint32))) for m in "abcd"}
    told = 0
    for name in ("radius -0", "radius -1", "radius -inf", "radius -smallest subnormal"):
        pair = np.stack([tc.named(name), tc.named("q = 1")])
        real, wrong = tc.expected_world(pair, **cfg), tc.mutant_e_world(pair, **cfg)
        assert bits(real) == bits(0.0) and bits(wrong) == bits(tc.expected(pair[1:], **cfg)[0]) and wrong > 0, (name, real, wrong)
        told += 1
    counts["e"] = told
    print("[timestep cases] cases whose dt bits a mutant changes: " + "  ".join(f"({m}) {c}" for m, c in counts.items()))
    assert all(counts[m] >= 50 for m in "abcd") and counts["e"] >= 2, counts
    # what the sweep is stated to contain
    s = tc.sweep(4096)
    assert s.dtype == np.float32 and s.tobytes() == tc.sweep(4096).tobytes()
    ratio = np.abs(s[:, 0].astype(np.float64)) / np.where(s[:, 1] == 0, np.inf, np.abs(s[:, 1].astype(np.float64)))
    assert 0.10 < np.mean(s[:, 1] == 0) < 0.15 and np.mean((ratio > 0.25) & (ratio < 4)) > 0.125
    a2 = tr.a2_f32(s[:, 0], s[:, 1])
    tiny = np.float32(2.0 ** -126)
    assert np.sum((a2 > 0) & (a2 < tiny)) > 50 and np.sum(np.isinf(a2)) > 10
    q = tr.q_all(tc.particles(s))
    assert np.sum((q > 0) & (q < tiny)) > 50 and np.sum(q == 0) > 100 and np.sum(np.isinf(q)) > 100
    assert np.sum(np.abs(s[:, 2]) < tiny) > 100 and np.sum(s[:, 2] < 0) > 100
    names = tc.directed_names()
    assert len(set(names)) == len(names) == tc.directed().shape[0]


def test_host_criterion_equals_the_restatement_over_the_case_tables():
    """GetWorldTimestep of a one-particle CPU World for every directed case and the first 512 sweep cases, under both
    configurations the device sweep uses, and the two-particle worlds of the device's pair test."""
    cases = np.concatenate([tc.directed(), tc.sweep(512)])
    names = tc.directed_names() + [f"sweep {i}" for i in range(512)]
    for cfg in (dict(eta=1.0, dt_max=3.0e38, dt_min=0.0), dict(eta=0.1, dt_max=10.0, dt_min=1.0e-3)):
        want = tc.expected(cases, **cfg)
        for name, c, w in zip(names, cases, want):
            got = host_dt(tc.particles(c), **cfg)
            assert bits(got) == bits(w), (name, [hex(b) for b in bits(c)], got, w)
    for a, b in tc.PAIRS:
        pair = tc.particles(np.stack([tc.named(a), tc.named(b)]))
        for p in (pair, pair[::-1]):
            got, want = host_dt(p, 1.0, 3.0e38), tr.timestep(p, 1.0, 3.0e38)
            assert bits(got) == bits(want), (a, b, got, want)


def test_the_restated_fma_is_the_correctly_rounded_one():
    """tests/timestep_ref.py a2_f32 against exact rational arithmetic, over magnitudes that reach the subnormals and overflow."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    ax = (rng.standard_normal(400) * 10.0 ** rng.integers(-24, 20, 400)).astype(np.float32)
    ay = (rng.standard_normal(400) * 10.0 ** rng.integers(-24, 20, 400)).astype(np.float32)
    got = tr.a2_f32(ax, ay)
    for x, y, g in zip(ax, ay, got):
        exact = Fraction(float(x)) ** 2 + Fraction(float(np.float32(np.float64(y) * np.float64(y))))
        if not np.isfinite(g):
            assert exact > Fraction(float(np.finfo(np.float32).max)), (x, y)
            continue
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        err = abs(exact - Fraction(float(g)))
        assert err <= abs(exact - Fraction(float(lo))) and (not np.isfinite(hi) or err <= abs(exact - Fraction(float(hi)))), (x, y, g)


# ---- 2. UpdateWorld_CPU_Adaptive is the loop of timestep() + update_cpu(dt, 1) ---------------------------------------------

def loop(ic, n, eta, dt_max, dt_min=0.0, span=math.inf, prime=False):
    w, clock, log = nb.World(ic), tr.Clock(span), []
    if prime:
        w.update_cpu(0.0, 1)
    for _ in range(n):
        dt = clock.step(np.float32(w.timestep(eta, dt_max, dt_min)))
        w.update_cpu(float(dt), 1)
        log.append(dt)
    p = w.particles()
    w.close()
    return p, np.array(log, dtype=np.float32), clock.result()


@pytest.mark.parametrize("prime", [False, True])
def test_cpu_adaptive_equals_the_loop_bitwise(golden, prime):
    ic = golden("ic_333.bin")
    w = nb.World(ic)
    log, res = w.update_cpu_adaptive(6, ETA, 0.5, prime=prime)
    p = w.particles()
    w.close()
    want_p, want_log, want_res = loop(ic, 6, ETA, 0.5, prime=prime)
    assert bits(log) == bits(want_log) and p.tobytes() == want_p.tobytes() and res == want_res
    if prime:
        assert log[0] < np.float32(0.5)
    else:
        assert log[0] == np.float32(0.5)          # a fresh world holds acc = 0: the first step is dt_max
    assert bits(log) == bits([tr.timestep(s, ETA, 0.5) for s in replay_states(ic, want_log, prime)])


def replay_states(ic, log, prime):
    """The states before every step of `log`, by fixed-step CPU updates."""
    w, out = nb.World(ic), []
    if prime:
        w.update_cpu(0.0, 1)
    for dt in log:
        out.append(w.particles())
        w.update_cpu(float(dt), 1)
    w.close()
    return out


def test_cpu_adaptive_span_that_ends_inside_the_call(golden):
    ic = golden("ic_333.bin")
    _, free, _ = loop(ic, 3, ETA, 0.5, prime=True)
    span = float(free[0]) + float(free[1]) + 0.5 * float(free[2])
    w = nb.World(ic)
    log, res = w.update_cpu_adaptive(6, ETA, 0.5, span=span, prime=True)
    p = w.particles()
    w.close()
    want_p, want_log, want_res = loop(ic, 6, ETA, 0.5, span=span, prime=True)
    assert bits(log) == bits(want_log) and p.tobytes() == want_p.tobytes() and res == want_res
    assert res["elapsed"] == span and res["steps"] == 3 and res["idle_steps"] == 3 and res["steps"] + res["idle_steps"] == 6
    assert bits(log[:2]) == bits(free[:2])
    assert bits(log[2]) == bits(np.float32(span - (float(free[0]) + float(free[1]))))          # the clipped step is (float)rem
    assert not log[3:].any() and res["dt_last"] == float(log[2])


# ---- 3. an eccentric two-body orbit ------------------------------------------------------------------------------------------

def two_body(e=0.9):
    """Equal masses, G (m1 + m2) = a = 1 with G = NB_G, at apocentre; one period is 2 pi."""
    r, m = 1.0 + e, 0.5 / nb.NB_G
    v = math.sqrt(2.0 / r - 1.0)
    a = np.zeros((2, 8), dtype=np.float32)
    a[0, 0], a[1, 0] = -r / 2, r / 2
    a[0, 3], a[1, 3] = -v / 2, v / 2
    a[:, 6], a[:, 7] = m, 1.0e-6
    return a


def worst_drift(ic, dts, prime):
    w = nb.World(ic)
    if prime:
        w.update_cpu(0.0, 1)
    e0, worst = w.energy()["total"], 0.0
    for dt in dts:
        w.update_cpu(float(dt), 1)
        worst = max(worst, abs(w.energy()["total"] - e0) / abs(e0))
    w.close()
    return worst


def test_two_body_orbit_adaptive_beats_fixed_steps():
    """e = 0.9, eta = 0.1, one period on the CPU path (float32 state, float64 energies): max |dE/E| of the primed adaptive run
    against the same number of fixed steps.  Measured here: 1 436 steps, adaptive 0.1358, fixed 0.4902, ratio 0.277 (the
    float64 sketch of the criterion gave 1 436 steps and 0.28).  The bound is the issue's 0.5."""
    ic, period = two_body(), 2.0 * math.pi
    w = nb.World(ic)
    log, res = w.update_cpu_adaptive(4000, ETA, 1.0, span=period, prime=True)
    w.close()
    assert res["elapsed"] == period and res["steps"] + res["idle_steps"] == 4000
    steps = res["steps"]
    assert 1000 < steps < 2000 and not log[steps:].any() and log[:steps].all()
    adaptive = worst_drift(ic, log[:steps], True)
    fixed = worst_drift(ic, [np.float32(period / steps)] * steps, True)
    print(f"[two-body e=0.9] {steps} steps: adaptive {adaptive:.4f}  fixed {fixed:.4f}  ratio {adaptive / fixed:.3f}")
    assert adaptive < 0.5 * fixed, (steps, adaptive, fixed)


# ---- 4. argument checks ------------------------------------------------------------------------------------------------------

def child(code, **env):
    e = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), **HIDDEN)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


SETUP = ("import numpy as np, ctypes as C, nbody_amd as nb\n"
         "a = np.zeros((4, 8), dtype=np.float32); a[:, 0] = np.arange(4); a[:, 6] = 1; a[:, 7] = 0.25\n"
         "w = nb.World(a); L = nb.nbody_lib(); inf = float('inf'); nan = float('nan')\n"
         "s = nb.SimPipeline(4, 4); b = nb.SimBatch(4, [4, 4]); wb = nb.WorldBatch(np.stack([a, a]))\n")
SHARDED = "fn = nb.ALLGATHER_FN(lambda *x: None); ws = nb.World.__new__(nb.World); ws._h = L.CreateWorldShardedWith(a.ctypes.data, 4, 0, 2, fn, None); "
ETA_MSG, MAX_MSG, MIN_MSG, SPAN_MSG = ("eta must be finite and > 0", "dt_max must be finite and > 0", "dt_min must be within [0, dt_max]",
                                       "span must be > 0")
ABORTS = [
    ("eta 0", "w.update_cpu_adaptive(1, 0.0, 1.0)", "UpdateWorld_CPU_Adaptive: " + ETA_MSG),
    ("eta negative", "w.update_gpu_adaptive(1, -0.1, 1.0)", "UpdateWorld_GPU_Adaptive: " + ETA_MSG),
    ("eta NaN", "w.timestep(nan, 1.0)", "GetWorldTimestep: " + ETA_MSG),
    ("eta inf", "s.update_adaptive(1, inf, 1.0)", "nb_hip_adaptive_steps: " + ETA_MSG),
    ("dt_max 0", "s.update_adaptive_async(1, 0.1, 0.0)", "nb_hip_adaptive_steps_async: " + MAX_MSG),
    ("dt_max inf", "b.update_adaptive(1, 0.1, inf)", "nb_hip_ensemble_adaptive_steps: " + MAX_MSG),
    ("dt_max NaN", "wb.update_gpu_adaptive(1, 0.1, nan)", "UpdateWorldBatch_GPU_Adaptive: " + MAX_MSG),
    ("dt_min negative", "w.advance_gpu(1.0, 0.1, 1.0, dt_min=-1e-3)", "AdvanceWorld_GPU: " + MIN_MSG),
    ("dt_min above dt_max", "wb.advance_gpu(1.0, 0.1, 1.0, dt_min=2.0)", "AdvanceWorldBatch_GPU: " + MIN_MSG),
    ("dt_min NaN", "s.timestep(0.1, 1.0, dt_min=nan)", "nb_hip_timestep: " + MIN_MSG),
    ("span 0", "w.update_cpu_adaptive(1, 0.1, 1.0, span=0.0)", "UpdateWorld_CPU_Adaptive: " + SPAN_MSG),
    ("span negative", "s.update_adaptive(1, 0.1, 1.0, span=-1.0)", "nb_hip_adaptive_steps: " + SPAN_MSG),
    ("span NaN", "b.update_adaptive(1, 0.1, 1.0, span=nan)", "nb_hip_ensemble_adaptive_steps: " + SPAN_MSG),
    ("advance span 0", "w.advance_gpu(0.0, 0.1, 1.0)", "AdvanceWorld_GPU: " + SPAN_MSG),
    ("too many steps", "s.update_adaptive((1 << 20) + 1, 0.1, 1.0)", "nb_hip_adaptive_steps: 1048577 steps > 2^20"),
    ("too many steps world", "w.update_cpu_adaptive((1 << 20) + 1, 0.1, 1.0)", "UpdateWorld_CPU_Adaptive: 1048577 steps > 2^20"),
    ("too many steps batch", "b.update_adaptive((1 << 20) + 1, 0.1, 1.0)", "nb_hip_ensemble_adaptive_steps: 1048577 steps > 2^20"),
    ("NULL cfg", "L.GetWorldTimestep(w._h, None, C.byref(C.c_float()))", "GetWorldTimestep: NULL argument"),
    ("NULL world", "cfg = nb.adaptive_cfg(0.1, 1.0); L.UpdateWorld_GPU_Adaptive(None, 1, C.byref(cfg), None, None)",
     "UpdateWorld_GPU_Adaptive: NULL argument"),
    ("before set_data", "s.update_adaptive(1, 0.1, 1.0)", "nb_hip_adaptive_steps before SetSimulationData"),
    ("timestep before set_data", "s.timestep(0.1, 1.0)", "nb_hip_timestep before SetSimulationData"),
    ("batch before set_data", "b.update_adaptive(1, 0.1, 1.0)", "nb_hip_ensemble_adaptive_steps before nb_hip_batch_set_data"),
    ("sharded pipeline", "fn = lambda *x: None; sp = nb.SimPipeline(4, 4, rank=0, nranks=2, allgather=fn); sp.update_adaptive(1, 0.1, 1.0)",
     "nb_hip_adaptive_steps of a sharded pipeline needs a collective"),
    ("sharded world", SHARDED + "ws.update_gpu_adaptive(1, 0.1, 1.0)", "UpdateWorld_GPU_Adaptive of a sharded pipeline needs a collective"),
    ("sharded world advance", SHARDED + "ws.advance_gpu(1.0, 0.1, 1.0)", "AdvanceWorld_GPU of a sharded pipeline needs a collective"),
    ("ragged ensemble", "r = nb.SimBatch.ragged([4, 3], [4, 3]); r.update_adaptive(1, 0.1, 1.0)",
     "nb_hip_ensemble_adaptive_steps: adaptive steps of ragged ensembles"),
    ("ragged batch", "r = nb.WorldBatch.ragged([a, a[:3]]); r.update_gpu_adaptive(1, 0.1, 1.0)",
     "UpdateWorldBatch_GPU_Adaptive: adaptive steps of ragged ensembles"),
    ("ragged batch advance", "r = nb.WorldBatch.ragged([a, a[:3]]); r.advance_gpu(1.0, 0.1, 1.0)",
     "AdvanceWorldBatch_GPU: adaptive steps of ragged ensembles"),
]


@pytest.mark.parametrize("name,code,needle", ABORTS, ids=[c[0] for c in ABORTS])
def test_bad_arguments_print_file_line_func_and_abort(name, code, needle):
    r = child(SETUP + code + "\nprint('SURVIVED')")
    assert r.returncode != 0 and "SURVIVED" not in r.stdout, (r.stdout, r.stderr)
    assert re.search(r"\.(hip|c|h):\d+ \[\w+\]", r.stderr), r.stderr
    assert needle in r.stderr, r.stderr


def test_no_steps_do_nothing_and_open_no_device():
    code = (SETUP +
            "import os\n"
            "before = w.particles().tobytes()\n"
            "out = [w.update_cpu_adaptive(0, 0.1, 1.0), w.update_gpu_adaptive(0, 0.1, 1.0), s.update_adaptive(0, 0.1, 1.0)]\n"
            "s.update_adaptive_async(0, 0.1, 1.0); out.append(s.adaptive_collect(0))\n"
            "zero = {'elapsed': 0.0, 'steps': 0, 'idle_steps': 0, 'dt_last': 0.0, 'dt_smallest': 0.0}\n"
            "assert all(log.shape == (0,) and res == zero for log, res in out), out\n"
            "for log, res in (b.update_adaptive(0, 0.1, 1.0), wb.update_gpu_adaptive(0, 0.1, 1.0)):\n"
            "    assert log.shape == (0, 2) and res == [zero, zero], (log, res)\n"
            "assert w.particles().tobytes() == before\n"
            "fds = []\n"
            "for f in os.listdir('/proc/self/fd'):\n"
            "    try: fds.append(os.readlink('/proc/self/fd/' + f))\n"
            "    except OSError: pass\n"
            "assert not [f for f in fds if f == '/dev/kfd' or f.startswith('/dev/dri/')], fds\n"
            "print('OK')\n")
    r = child(code)
    assert r.returncode == 0 and r.stdout.strip() == "OK", (r.stdout, r.stderr)


# ---- sources, headers, exports -----------------------------------------------------------------------------------------------

def test_header_binding_exports_and_sources_agree():
    assert declared_functions("nbody_adaptive.h") == WORLD_FUNCS and set(WORLD_FUNCS) <= set(nb.NBODY_API)
    for so in WORLD_LIBS:
        have = exported(os.path.join(nb.LIB_DIR, so))
        assert set(WORLD_FUNCS) <= have and not {"nb_cpu_timestep", "nb_cpu_timestep_q"} & have, so
    assert set(HIP_FUNCS) <= set(declared_functions("nbody_hip.h")) & set(nb.HIP_API) and set(HIP_FUNCS) <= exported(nb.HIP_SO)
    assert 'dlsym "nb_hip_adaptive_steps"' in open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    assert C_sizes() == (32, 24)
    for cls, methods in ((nb.SimPipeline, ("update_adaptive", "timestep")), (nb.SimBatch, ("update_adaptive",)),
                         (nb.World, ("update_gpu_adaptive", "update_cpu_adaptive", "timestep", "advance_gpu")),
                         (nb.WorldBatch, ("update_gpu_adaptive", "advance_gpu"))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)
    import inspect
    sig = inspect.signature(nb.SimPipeline.update_adaptive).parameters
    assert sig["eta"].default is inspect.Parameter.empty and sig["dt_max"].default is inspect.Parameter.empty
    csrc = os.path.join(ROOT, "nbody_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    assert re.search(r"^HIP_TUS\s*:=.*\btimestep\b", make, re.M) and re.search(r"^WORLD_SRCS\s*:=.*\btimestep_cpu\.c", make, re.M)
    assert make.count("timestep_common.h") >= 2 and make.count("include/nbody_adaptive.h") >= 2
    for src in ("timestep.hip", "timestep_cpu.c", "step_schedule.hip", "world.c", "world_batch.c"):
        assert '#include "timestep_common.h"' in open(os.path.join(csrc, src)).read(), src
    # the statement is written once: nobody else divides a radius by a squared acceleration
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".c", ".h")) and name != "timestep_common.h":
            text = open(os.path.join(csrc, name), errors="replace").read()
            assert "__builtin_fmaxf(radius" not in text and "radius > 0.0f ? radius" not in text, name
    assert "(radius > 0.0f ? radius : 0.0f) / a2" in open(os.path.join(csrc, "timestep_common.h")).read()


def C_sizes():
    import ctypes as C
    return C.sizeof(nb.NbAdaptive), C.sizeof(nb.NbAdaptiveResult)


# ---- 5. static ISA of timestep.hip ---------------------------------------------------------------------------------------------

KERNELS = ("timestep_kernel", "ensemble_timestep_kernel")


@pytest.fixture(scope="module")
def timestep_isa(tmp_path_factory):
    return compile_isa(tmp_path_factory.mktemp("timestep_isa"), "timestep.hip")


def test_timestep_kernels_fit_their_launch_bounds_without_scratch(timestep_isa):
    meta = {n: (scratch, sgpr, vgpr) for n, scratch, sgpr, vgpr in kernel_meta(timestep_isa)}
    lds = {name: int(size) for size, name in re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)", timestep_isa)}
    for k in KERNELS:
        names = [n for n in meta if re.search(r"\d%sE" % k, n)]
        assert len(names) == 1, (k, sorted(meta))
        scratch, sgpr, vgpr = meta[names[0]]
        print(f"[timestep isa] {names[0]}: scratch {scratch}, {sgpr} SGPRs, {vgpr} VGPRs, {lds[names[0]]} bytes of LDS")
        assert scratch == 0, f"{k}: {scratch} bytes of scratch"
        assert vgpr <= 64 and sgpr <= 102, (k, sgpr, vgpr)          # 256 threads per workgroup: far inside __launch_bounds__(256)
        assert lds[names[0]] == 16, (k, lds[names[0]])              # one value per wave, nothing dynamic
