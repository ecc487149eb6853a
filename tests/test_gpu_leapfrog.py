"""Leapfrog (kick-drift-kick) steps on the MI355X (include/nbody_leapfrog.h): the composition contract.  The state after a
leapfrog call is, bit for bit, what the caller composes from get_data, the numpy float32 open / close of tests/leapfrog_ref.py,
set_data and update(1, 0) of the same object -- at one size per step route, across call boundaries, for ensembles, for the
adaptive calls with leapfrog=True, through the World layer and for non-finite values."""
import math

import numpy as np
import pytest

import leapfrog_ref as lr
import nbody_amd as nb
import timestep_ref as tr
from gpu_common import DISPLACEMENT_TOL, rel_displacement, synth

pytestmark = pytest.mark.gpu

DT = 0.01
ETA, DT_MAX = 0.1, 1.0


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


def partitioned(ic):
    """(the World's own order of these particles, massive first; mass_len)"""
    w = nb.World(ic)
    p = w.particles()
    w.close()
    return p, int((p[:, 6] > 0).sum())


def first_size(want):
    return next(n for n in range(2, 65537) if want(nb.plan_launch(n, n)))


# The smallest N <= 65 536 for which nb.plan_launch reports split > 1 is 513 -- but an all-auto step of that size runs as a
# lane-split launch (plan_launch's "lanes" > 1), which walks one source range.  The smallest size at which the source split
# really runs (lanes == 1) is 3 001; both are in the list, and the test asserts what the second one launched.
FIRST_PLANNED_SPLIT = 513
FIRST_SPLIT_THAT_RUNS = 3001
SIZES = [2, 130, 333, 512, FIRST_PLANNED_SPLIT, FIRST_SPLIT_THAT_RUNS, 4096]

_worlds = {}


def world(n, golden):
    """(partitioned particles, mass_len): 333 and 4 096 the committed fixtures (4 096 with its massless tail), else all massive."""
    if n not in _worlds:
        if n in (333, 4096):
            _worlds[n] = partitioned(golden(f"ic_{n}.bin"))
        else:
            _worlds[n] = synth(n, frac_massive=1.0, seed=n)
    return _worlds[n]


def pipeline(part, m):
    s = nb.SimPipeline(part.shape[0], m)
    s.set_data(part)
    return s


def force_of(s):
    """The composition's force: set_data, update(1, 0), get_data of the object itself."""
    def force(p):
        s.set_data(p)
        s.update(1, 0.0)
        return s.get_data()
    return force


def composed(part, m, dts, **kw):
    s = nb.SimPipeline(part.shape[0], m)
    out = lr.compose(force_of(s), part, dts, **kw)
    s.close()
    return out


def leapfrog(part, m, calls, dt=DT):
    s = pipeline(part, m)
    info = []
    for n in calls:
        s.update_leapfrog(n, dt)
        info.append(s.last_leapfrog_info())
    out, shape = s.get_data(), s.launch_shape()
    s.close()
    return out, info, shape


def test_the_sizes_named_above_are_what_the_plan_says():
    assert first_size(lambda p: p["split"] > 1) == FIRST_PLANNED_SPLIT
    assert first_size(lambda p: p["split"] > 1 and p["lanes"] == 1) == FIRST_SPLIT_THAT_RUNS


# ---- one world ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_pipeline_leapfrog_equals_the_composition_bitwise(golden, n):
    part, m = world(n, golden)
    for steps in (1, 3):
        got, info, shape = leapfrog(part, m, [steps])
        want = composed(part, m, [DT] * steps)
        assert lr.same_bits(got, want), (n, steps, lr.differing(got, want))
        assert info == [(steps + 1, True)]
    if n == FIRST_SPLIT_THAT_RUNS:
        assert shape["split"] > 1 and shape["lanes"] == 1, shape
    if n == 4096:
        assert m < n and np.any(got[m:, 0:2] != part[m:, 0:2])          # the massless tail moves too
    if n == 333:          # the checker tells the wrong statements apart on the device's own force as well
        for mutant in lr.MUTANTS:
            assert lr.differing(got, composed(part, m, [DT] * 3, mutant=mutant)) > 0, mutant
        assert not lr.same_bits(got, composed(part, m, [DT] * 3, prime=False))


@pytest.mark.parametrize("n", [333, FIRST_SPLIT_THAT_RUNS])
def test_five_steps_are_two_plus_three_and_the_hook_counts_force_launches(golden, n):
    part, m = world(n, golden)
    whole, info5, _ = leapfrog(part, m, [5])
    split, info23, _ = leapfrog(part, m, [2, 3])
    assert lr.same_bits(whole, split), lr.differing(whole, split)
    assert info5 == [(6, True)] and info23 == [(3, True), (3, False)]
    assert lr.same_bits(whole, composed(part, m, [DT] * 5))


@pytest.mark.parametrize("what", ["update", "set_data", "euler adaptive"])
def test_the_next_call_primes_again_after(golden, what):
    part, m = world(333, golden)
    s = pipeline(part, m)
    s.update_leapfrog(2, DT)
    if what == "update":
        s.update(1, DT)
    elif what == "set_data":
        s.set_data(s.get_data())
    else:
        s.update_adaptive(1, ETA, DT_MAX)
    mid = s.get_data()
    s.update_leapfrog(2, DT)
    got, info = s.get_data(), s.last_leapfrog_info()
    s.update_leapfrog(1, DT)
    again = s.last_leapfrog_info()
    s.close()
    assert info == (3, True) and again == (1, False)
    assert lr.same_bits(got, composed(mid, m, [DT] * 2, prime=True))


def test_a_fixed_step_update_after_a_leapfrog_call_uploads_its_own_step_size(golden):
    part, m = world(333, golden)
    a = pipeline(part, m)
    a.update(1, DT)                 # the step kernels' word holds DT, and the host knows it
    a.update_leapfrog(2, DT)        # ... now it holds 0
    mid = a.get_data()
    a.update(3, DT)
    b = pipeline(mid, m)
    b.update(3, DT)
    got, want = a.get_data(), b.get_data()
    a.close()
    b.close()
    assert got.tobytes() == want.tobytes() and np.any(got[:, 0:2] != mid[:, 0:2])


def test_the_async_form_equals_the_blocking_one(golden):
    part, m = world(333, golden)
    a, b = pipeline(part, m), pipeline(part, m)
    a.update_leapfrog_async(2, DT)
    a.update_leapfrog_async(1, 0.5 * DT)
    a.sync()
    b.update_leapfrog(2, DT)
    b.update_leapfrog(1, 0.5 * DT)
    got, want = a.get_data(), b.get_data()
    a.close()
    b.close()
    assert got.tobytes() == want.tobytes()


# ---- ensembles -----------------------------------------------------------------------------------------------------------------

_members = {}


def members(n, count):
    if (n, count) not in _members:
        worlds = [synth(n, frac_massive=0.5, seed=1000 * n + b) for b in range(count)]
        _members[n, count] = (np.stack([p for p, _ in worlds]), [m for _, m in worlds])
    return _members[n, count]


def batch(parts, ms):
    s = nb.SimBatch(parts.shape[1], ms)
    s.set_data(parts)
    return s


def batch_force_of(s):
    def force(p):
        s.set_data(p)
        s.update(1, 0.0)
        return s.get_data()
    return force


@pytest.mark.parametrize("n,count,path", [(250, 5, "chain"), (1000, 3, "lanes")])
def test_ensemble_members_are_the_composition_and_do_not_depend_on_their_neighbours(n, count, path):
    parts, ms = members(n, count)
    dts = np.array([DT * (b + 1) for b in range(count)], dtype=np.float32)
    dts[1] = 0.0
    order = list(range(count))[::-1]
    for dt in (DT, dts):
        a = batch(parts, ms)
        assert a.launch_shape()["path"] == path
        a.update_leapfrog(2, dt)
        first = a.last_leapfrog_info()
        a.update_leapfrog(1, dt)
        got, second = a.get_data(), a.last_leapfrog_info()
        a.close()
        assert first == (3, True) and second == (1, False)
        r = nb.SimBatch(n, ms)
        want = lr.compose(batch_force_of(r), parts, [dt] * 3)
        r.close()
        assert lr.same_bits(got, want), (n, count, lr.differing(got, want))
        # the members in another order, each with its own step size
        b = batch(parts[order], [ms[i] for i in order])
        b.update_leapfrog(3, dt if np.ndim(dt) == 0 else dt[order])
        moved = b.get_data()
        b.close()
        assert lr.same_bits(moved, got[order])
    # dt = 0: an idle member keeps its positions and velocities through all three steps
    r = nb.SimBatch(n, ms)
    idle = lr.compose(batch_force_of(r), parts, [0.0])
    r.close()
    assert lr.same_bits(got[1, :, 0:4], idle[1, :, 0:4])


# The ensemble twins of the two pipeline tests above: what a call leaves behind (acc_current, dt_valid) is kept by the same
# code for a world and for an ensemble.  250 particles x 3 members on the chain path, 600 x 2 on the lane-split path.
BATCH_SHAPES = [(250, 3, "chain"), (600, 2, "lanes")]


@pytest.mark.parametrize("what", ["update", "set_data", "euler adaptive", "trace"])
@pytest.mark.parametrize("n,count,path", BATCH_SHAPES)
def test_the_next_ensemble_call_primes_again_after(n, count, path, what):
    parts, ms = members(n, count)
    s = batch(parts, ms)
    assert s.launch_shape()["path"] == path
    s.update_leapfrog(2, DT)
    if what == "update":
        s.update(1, DT)
    elif what == "set_data":
        s.set_data(s.get_data())
    elif what == "euler adaptive":
        s.update_adaptive(1, ETA, DT_MAX)
    else:
        s.trace(1, DT, 1)
    mid = s.get_data()
    s.update_leapfrog(2, DT)
    got, info = s.get_data(), s.last_leapfrog_info()
    s.update_leapfrog(1, DT)
    again = s.last_leapfrog_info()
    s.close()
    assert info == (3, True) and again == (1, False)
    r = nb.SimBatch(n, ms)
    want = lr.compose(batch_force_of(r), mid, [DT] * 2, prime=True)
    r.close()
    assert lr.same_bits(got, want), (n, count, what, lr.differing(got, want))


@pytest.mark.parametrize("per_member", [False, True])
@pytest.mark.parametrize("n,count,path", BATCH_SHAPES)
def test_a_fixed_step_ensemble_update_after_a_leapfrog_call_uploads_its_own_step_sizes(n, count, path, per_member):
    parts, ms = members(n, count)
    dt = np.array([DT * (b + 1) for b in range(count)], dtype=np.float32) if per_member else DT
    a = batch(parts, ms)
    assert a.launch_shape()["path"] == path
    a.update(1, dt)                 # the step kernels' words hold dt, and the host knows it
    a.update_leapfrog(2, dt)        # ... now they hold 0
    mid = a.get_data()
    a.update(3, dt)
    b = batch(mid, ms)
    b.update(3, dt)
    got, want = a.get_data(), b.get_data()
    a.close()
    b.close()
    assert got.tobytes() == want.tobytes() and np.any(got[:, :, 0:2] != mid[:, :, 0:2])


# ---- adaptive leapfrog -------------------------------------------------------------------------------------------------------

STEPS = 6


def replay_pipeline(part, m, log, span):
    """Drive a second pipeline by update_leapfrog(1, log[i]); before every step the host criterion of its state, whose acc is
    its own, must give log[i] bit for bit."""
    b, clock = pipeline(part, m), tr.Clock(span)
    b.update(1, 0.0)
    for i, dt in enumerate(log):
        want = clock.step(tr.timestep(b.get_data(), ETA, DT_MAX))
        assert bits(dt) == bits(want), (i, float(dt), float(want))
        b.update_leapfrog(1, float(dt))
    out = b.get_data()
    b.close()
    return out, clock.result()


@pytest.mark.parametrize("n", [333, 4096])
def test_adaptive_leapfrog_logs_the_criterion_and_replays(golden, n):
    part, m = world(n, golden)
    a = pipeline(part, m)
    free, _ = a.update_adaptive(3, ETA, DT_MAX, leapfrog=True)
    assert a.last_leapfrog_info() == (4, True)
    a.close()
    assert np.all(free > 0) and np.all(free < np.float32(DT_MAX))          # the implied prime: not the fresh world's dt_max
    span = float(free[0]) + float(free[1]) + 0.5 * float(free[2])
    a = pipeline(part, m)
    log, res = a.update_adaptive(STEPS, ETA, DT_MAX, span=span, leapfrog=True)
    got = a.get_data()
    a.close()
    want, want_res = replay_pipeline(part, m, log, span)
    assert lr.same_bits(got, want), lr.differing(got, want)
    assert res == want_res and res["elapsed"] == span and res["steps"] == 3 and res["idle_steps"] == 3
    assert bits(log[:2]) == bits(free[:2]) and not log[3:].any()
    # the same in two calls, the second resumed: the clock and the counts go on, and no second prime
    a = pipeline(part, m)
    log1, _ = a.update_adaptive(2, ETA, DT_MAX, span=span, leapfrog=True)
    log2, res2 = a.update_adaptive(STEPS - 2, ETA, DT_MAX, span=span, leapfrog=True, resume=True, prime=True)
    assert a.last_leapfrog_info() == (STEPS - 2, False)
    again = a.get_data()
    a.close()
    assert bits(np.concatenate([log1, log2])) == bits(log) and res2 == res and lr.same_bits(again, got)


def test_adaptive_leapfrog_of_an_ensemble_logs_the_criterion_and_replays():
    parts, ms = members(250, 4)
    count = 4
    a = batch(parts, ms)
    free, _ = a.update_adaptive(3, ETA, DT_MAX, leapfrog=True)
    a.close()
    spans = [float(free[0, b]) + float(free[1, b]) + 0.5 * float(free[2, b]) for b in range(count)]
    span = min(spans)                  # ends inside the call for every member, after a different number of steps
    a = batch(parts, ms)
    log, res = a.update_adaptive(STEPS, ETA, DT_MAX, span=span, leapfrog=True)
    got, info = a.get_data(), a.last_leapfrog_info()
    a.close()
    assert info == (STEPS + 1, True) and log.shape == (STEPS, count)
    r, clocks = batch(parts, ms), [tr.Clock(span) for _ in range(count)]
    r.update(1, 0.0)
    for i in range(STEPS):
        state = r.get_data()
        want = [clocks[b].step(tr.timestep(state[b], ETA, DT_MAX)) for b in range(count)]
        assert bits(log[i]) == bits(want), (i, log[i], want)
        r.update_leapfrog(1, log[i])
    want = r.get_data()
    r.close()
    assert lr.same_bits(got, want), lr.differing(got, want)
    assert res == [c.result() for c in clocks]
    assert all(x["elapsed"] == span and x["idle_steps"] >= 3 and x["steps"] + x["idle_steps"] == STEPS for x in res), res
    # two calls, the second resumed
    a = batch(parts, ms)
    log1, _ = a.update_adaptive(2, ETA, DT_MAX, span=span, leapfrog=True)
    log2, res2 = a.update_adaptive(STEPS - 2, ETA, DT_MAX, span=span, leapfrog=True, resume=True)
    again, info = a.get_data(), a.last_leapfrog_info()
    a.close()
    assert info == (STEPS - 2, False)
    assert bits(np.concatenate([log1, log2])) == bits(log) and res2 == res and lr.same_bits(again, got)


# ---- the World layer -----------------------------------------------------------------------------------------------------------

def world_leapfrog_info(w):
    import ctypes as C
    k, primed = C.c_uint32(0), C.c_int(0)
    nb.hip_lib().nb_hip_last_leapfrog_info(w.pipeline(), C.byref(k), C.byref(primed))
    return int(k.value), bool(primed.value)


def test_world_layer_equals_the_seam_and_keeps_the_coherence_rules(golden):
    ic = golden("ic_333.bin")
    part, m = partitioned(ic)
    w = nb.World(ic)
    w.update_gpu_leapfrog(DT, 3)
    seam, _, _ = leapfrog(part, m, [3])
    assert lr.same_bits(w.particles(), seam)
    w.update_gpu_leapfrog(DT, 2)                  # nothing changed on the host: no upload, no second prime
    assert world_leapfrog_info(w) == (2, False)
    assert lr.same_bits(w.particles(), leapfrog(part, m, [3, 2])[0])
    w.close()
    # CPU leapfrog, GPU leapfrog, CPU leapfrog: every change of side is a transfer, and the side that receives primes
    w = nb.World(ic)
    w.update_cpu_leapfrog(DT, 2)
    w.update_gpu_leapfrog(DT, 2)
    w.update_cpu_leapfrog(DT, 1)
    got = w.particles()
    w.close()
    c = nb.World(ic)
    c.update_cpu_leapfrog(DT, 2)
    on_gpu, info, _ = leapfrog(c.particles(), m, [2])
    c.close()
    c = nb.World(on_gpu)
    c.update_cpu_leapfrog(DT, 1)
    want = c.particles()
    c.close()
    assert info == [(3, True)] and lr.same_bits(got, want), lr.differing(got, want)


def test_ten_gpu_steps_stay_within_the_displacement_bound_of_ten_cpu_steps(golden):
    ic = golden("ic_4096.bin")
    g, c = nb.World(ic), nb.World(ic)
    start = g.particles()
    g.update_gpu_leapfrog(DT, 10)
    c.update_cpu_leapfrog(DT, 10)
    got, want = g.particles(), c.particles()
    g.close()
    c.close()
    err = rel_displacement(got, want, start)
    print(f"[leapfrog] ic_4096, ten steps: displacement error GPU vs CPU {err:.3e}")
    assert err <= DISPLACEMENT_TOL, err


def test_advance_with_leapfrog_reaches_its_span_and_replays(golden):
    ic = golden("ic_333.bin")
    part, m = partitioned(ic)
    w = nb.World(ic)
    first, _ = w.update_gpu_adaptive(1, ETA, DT_MAX, leapfrog=True)
    span = 7.3 * float(first[0])
    log, res = w.advance_gpu(span, ETA, DT_MAX, chunk=4, leapfrog=True)
    got = w.particles()
    w.close()
    assert res["elapsed"] == span and len(log) == res["steps"] + res["idle_steps"] and res["steps"] >= 7
    s = pipeline(part, m)
    for dt in np.concatenate([first, log]):
        s.update_leapfrog(1, float(dt))
    want = s.get_data()
    s.close()
    assert lr.same_bits(got, want), lr.differing(got, want)


def test_world_batch_leapfrog_equals_the_ensemble_and_advance_reaches_its_span():
    parts, ms = members(250, 4)
    wb = nb.WorldBatch(parts)
    wb.update_gpu_leapfrog(DT, 2)
    dts = [DT, 0.0, 2 * DT, 0.5 * DT]
    wb.update_gpu_leapfrog(dts, 1)
    s = batch(parts, ms)
    s.update_leapfrog(2, DT)
    s.update_leapfrog(1, dts)
    assert lr.same_bits(wb.particles(), s.get_data())
    s.close()
    first, _ = wb.update_gpu_adaptive(1, ETA, DT_MAX, leapfrog=True)
    span = 5.5 * float(first.max())
    log, res = wb.advance_gpu(span, ETA, DT_MAX, chunk=8, max_steps=1 << 12, leapfrog=True)
    wb.close()
    assert all(x["elapsed"] == span for x in res) and all(x["steps"] + x["idle_steps"] == log.shape[0] for x in res)


# ---- non-finite values -------------------------------------------------------------------------------------------------------

def classes(a):
    """per value: 0 finite, 1 +inf, 2 -inf, 3 NaN"""
    a = np.asarray(a, dtype=np.float32)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


@pytest.mark.parametrize("case", ["infinite velocity", "NaN position"])
def test_non_finite_values_take_the_class_of_the_cpu_leapfrog_path(golden, case):
    part, m = world(4096, golden)
    assert m < part.shape[0]
    for j in (part.shape[0] - 1, 0):          # a massless particle of the tail, then a massive one
        odd = part.copy()
        if case == "infinite velocity":
            odd[j, 2] = np.inf
        else:
            odd[j, 1] = np.nan
        got, _, _ = leapfrog(odd, m, [2])
        c = nb.World(odd)
        c.update_cpu_leapfrog(DT, 2)
        want = c.particles()
        c.close()
        assert np.array_equal(classes(got), classes(want)), (case, j, np.argwhere(classes(got) != classes(want))[:4])
        assert classes(got[j]).any()
        if j >= m:          # massless: nobody feels it, so every other particle has the bits of the world without the odd value
            clean, _, _ = leapfrog(part, m, [2])
            others = np.arange(part.shape[0]) != j
            assert lr.same_bits(got[others], clean[others]), lr.differing(got[others], clean[others])
            assert not classes(got[others]).any()
