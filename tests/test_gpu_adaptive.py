"""Adaptive time steps on the MI355X (include/nbody_adaptive.h): the replay contract.  Every logged step size is, bit for bit,
the host criterion (tests/timestep_ref.py) of the state before its step, and a second pipeline driven by update(1, dt_log[i])
ends in the same bits -- for one world at sizes that take every step route and a criterion grid of several workgroups with a
ragged tail, with the particle that sets the minimum planted at either end of the arrays, with a span that ends inside the
call, for ensembles, and through the World layer."""
import math

import numpy as np
import pytest

import nbody_amd as nb
import oracle_binding as ob
import sequence_driver as sd
import timestep_ref as tr
from gpu_common import synth

pytestmark = pytest.mark.gpu

ETA, DT_MAX = 0.1, 1.0
WARM = (2, 0.01)          # two fixed steps first, so that acc is not trivial
STEPS = 6
SIZES = [1, 333, 600, 4133]


def bits(x):
    return np.asarray(x, dtype=np.float32).view(np.uint32).tolist()


_worlds = {}


def world(n, golden):
    """(partitioned particles, mass_len): N = 1 one body; 333 the committed fixture; 600 half massive (the lane-split route);
    4 133 all massive (N x M > 9e6: the classic route; 17 criterion workgroups, the last one 37 rows)."""
    if n not in _worlds:
        if n == 1:
            a = np.zeros((1, 8), dtype=np.float32)
            a[0, 6], a[0, 7] = 5.0, 0.5
            _worlds[n] = (a, 1)
        elif n == 333:
            _worlds[n] = ob.partition(golden("ic_333.bin"))
        else:
            _worlds[n] = synth(n, frac_massive=0.5 if n == 600 else 1.0, seed=n)
    return _worlds[n]


def pipeline(part, m, warm=True, **knobs):
    """warm: True = the two fixed steps; "zero" = one dt = 0 step (acc of exactly this state); False = as uploaded.
    knobs: the launch shape (configure), applied before set_data."""
    s = nb.SimPipeline(part.shape[0], m)
    s.configure(**knobs)
    s.set_data(part)
    if warm == "zero":
        s.update(1, 0.0)
    elif warm:
        s.update(*WARM)
    return s


def replay(b, log, clock, eta=ETA, dt_max=DT_MAX, dt_min=0.0):
    """Drive pipeline b by update(1, log[i]); before every step the host criterion of b's state must give log[i] bit for bit."""
    for i, dt in enumerate(log):
        want = clock.step(tr.timestep(b.get_data(), eta, dt_max, dt_min))
        assert bits(dt) == bits(want), (i, float(dt), float(want))
        b.update(1, float(dt))


def check_contract(part, m, label, warm=True, knobs=None, **cfg):
    """knobs: configure() arguments for BOTH pipelines, the adaptive one and the one that replays."""
    knobs = knobs or {}
    a, b = pipeline(part, m, warm, **knobs), pipeline(part, m, warm, **knobs)
    log, res = a.update_adaptive(STEPS, ETA, DT_MAX, **cfg)
    clock = tr.Clock(cfg.get("span", math.inf))
    replay(b, log, clock)
    got, want = a.get_data(), b.get_data()
    a.close()
    b.close()
    assert got.tobytes() == want.tobytes(), (label, "pos / vel / acc differ from the replay through update(1, dt_log[i])")
    assert res == clock.result(), (label, res, clock.result())
    return log, res


@pytest.mark.parametrize("n", SIZES)
def test_log_is_the_host_criterion_and_the_state_is_the_replay(golden, n):
    part, m = world(n, golden)
    log, res = check_contract(part, m, f"N={n}")
    assert res["steps"] == STEPS and res["idle_steps"] == 0
    if n == 1:
        assert bits(log) == bits([DT_MAX] * STEPS)          # one body feels nothing: every particle is skipped
    else:
        assert np.all(log > 0) and np.all(log < np.float32(DT_MAX)) and len(set(bits(log))) > 1, log


@pytest.mark.parametrize("n", SIZES[1:])
@pytest.mark.parametrize("where", ["last", "first"])
def test_planted_minimum_at_either_end(golden, n, where):
    """The particle that sets the minimum sits at index N - 1 / index 0: a criterion that reads a pad row or drops the tail of
    its grid fails here."""
    m = world(n, golden)[1]
    j = n - 1 if where == "last" else 0
    near = 1 if j == 0 else 0
    part = tr.plant(pipeline_state(n, golden), j, near)          # planted into the warmed-up state: a close pair, not yet flung apart
    probe = pipeline(part, m, "zero")
    assert int(np.argmin(tr.q_all(probe.get_data()))) == j
    free = probe.timestep(ETA, DT_MAX)
    probe.close()
    log, _ = check_contract(part, m, f"N={n} minimum at {j}", warm="zero")
    assert bits(log[0]) == bits(free) and log[0] < 0.1 * tr.timestep(pipeline_state(n, golden), ETA, DT_MAX)


_states = {}


def pipeline_state(n, golden):
    """The warmed-up state of the unplanted world (computed once)."""
    if n not in _states:
        s = pipeline(*world(n, golden))
        _states[n] = s.get_data()
        s.close()
    return _states[n]


@pytest.mark.parametrize("n", [333, 4133])
def test_span_clip_idle_steps_and_prime(golden, n):
    part, m = world(n, golden)
    a = pipeline(part, m)
    free, _ = a.update_adaptive(3, ETA, DT_MAX)
    a.close()
    span = float(free[0]) + float(free[1]) + 0.5 * float(free[2])
    log, res = check_contract(part, m, f"N={n} span", span=span)
    assert res["elapsed"] == span and res["steps"] == 3 and res["idle_steps"] == 3
    assert bits(log[:2]) == bits(free[:2]) and bits(log[2]) == bits(np.float32(span - (float(free[0]) + float(free[1]))))
    assert not log[3:].any()
    # an idle step is a dt = 0 step: pos and vel stay, acc is re-evaluated
    a, b = pipeline(part, m), pipeline(part, m)
    a.update_adaptive(3, ETA, DT_MAX, span=span)
    b.update_adaptive(STEPS, ETA, DT_MAX, span=span)
    pa, pb = a.get_data(), b.get_data()
    a.close()
    b.close()
    assert pa[:, 0:4].tobytes() == pb[:, 0:4].tobytes()
    # prime equals a preceding update(1, 0.0), on a fresh world (acc = 0 would give dt_max)
    a, b = pipeline(part, m, warm=False), pipeline(part, m, warm=False)
    log_a, res_a = a.update_adaptive(3, ETA, DT_MAX, prime=True)
    b.update(1, 0.0)
    log_b, res_b = b.update_adaptive(3, ETA, DT_MAX)
    pa, pb = a.get_data(), b.get_data()
    c = pipeline(part, m, warm=False)
    unprimed, _ = c.update_adaptive(1, ETA, DT_MAX)
    a.close()
    b.close()
    c.close()
    assert bits(log_a) == bits(log_b) and res_a == res_b and pa.tobytes() == pb.tobytes()
    assert unprimed[0] == np.float32(DT_MAX) and log_a[0] < np.float32(DT_MAX)


def test_async_twin_and_timestep_change_nothing(golden):
    part, m = world(333, golden)
    a, b = pipeline(part, m), pipeline(part, m)
    before = a.get_data()
    dt = a.timestep(ETA, DT_MAX)
    assert bits(dt) == bits(tr.timestep(before, ETA, DT_MAX)) and a.get_data().tobytes() == before.tobytes()
    a.update_adaptive_async(STEPS, ETA, DT_MAX)
    log_a, res_a = a.adaptive_collect(STEPS)
    log_b, res_b = b.update_adaptive(STEPS, ETA, DT_MAX)
    assert bits(log_a) == bits(log_b) and res_a == res_b and bits(log_a[0]) == bits(dt)
    # a fixed-step call afterwards uploads its own step size again
    a.update(1, 0.01)
    b.update(1, 0.01)
    pa, pb = a.get_data(), b.get_data()
    a.close()
    b.close()
    assert pa.tobytes() == pb.tobytes()


# ---- every launch shape --------------------------------------------------------------------------------------------------------
# enqueue_adaptive launches its steps through the shape the fixed steps have, so the contract holds on each of them: the
# rows of tests/sequence_driver.py PIPE_ROWS at their sizes (the smallest at which each route exists).

_shape_worlds = {}


def shape_world(n, frac):
    """(partitioned particles, mass_len, the state after the two fixed steps at the default shape); computed once"""
    if (n, frac) not in _shape_worlds:
        part, m = synth(n, frac_massive=frac, seed=n)
        s = pipeline(part, m)
        _shape_worlds[(n, frac)] = (part, m, s.get_data())
        s.close()
    return _shape_worlds[(n, frac)]


def assert_the_row_runs_its_shape(row, part, m, knobs):
    """What the knobs were set for really happens in an adaptive call: the finish kernel, its absence, the second pass, the LDS
    variant, the lane split."""
    s = pipeline(part, m, **knobs)
    s.update_adaptive(2, ETA, DT_MAX)
    shape, finish, launches = s.launch_shape(), s.finish_launches(), s.last_step_ms()[1]
    s.close()
    if row == "split3-finish-9000":
        assert shape["split"] == 3 and finish == 2, (shape, finish)
    elif row == "fused-finish-9000":
        assert shape["split"] > 1 and finish == 0, (shape, finish)
    elif row == "passes2-1500":
        assert launches == 4, launches
    elif row == "classic-4133-lds":
        assert shape["variant"] == "lds", shape
    elif row == "lanes4-w8-900":
        assert shape["lanes"] == 4 and shape["w"] == 8, shape
    elif row.startswith("lanes-600"):
        assert shape["lanes"] > 1, shape
    elif row.startswith("classic-4133"):
        assert shape["lanes"] == 1 and shape["variant"] == "smem", shape


@pytest.mark.parametrize("row", list(sd.PIPE_ROWS))
def test_the_contract_holds_on_every_launch_shape(row):
    n, frac, knobs = sd.PIPE_ROWS[row]
    part, m, _ = shape_world(n, frac)
    assert_the_row_runs_its_shape(row, part, m, knobs)
    log, res = check_contract(part, m, row, knobs=knobs)
    assert res["steps"] == STEPS and res["idle_steps"] == 0
    assert np.all(log > 0) and np.all(log < np.float32(DT_MAX)) and len(set(bits(log))) > 1, log


@pytest.mark.parametrize("row", ["split3-finish-9000", "passes2-1500"])
def test_planted_minimum_at_the_last_row_on_split_and_two_pass_shapes(row):
    """The step size the device chose is read by the finish kernel of a split launch, and by both passes of a two-pass step;
    the particle that sets it sits at index N - 1."""
    n, frac, knobs = sd.PIPE_ROWS[row]
    _, m, warmed = shape_world(n, frac)
    part = tr.plant(warmed, n - 1, 0)
    probe = pipeline(part, m, "zero", **knobs)
    assert int(np.argmin(tr.q_all(probe.get_data()))) == n - 1
    free = probe.timestep(ETA, DT_MAX)
    probe.close()
    log, _ = check_contract(part, m, f"{row} minimum at {n - 1}", warm="zero", knobs=knobs)
    assert bits(log[0]) == bits(free) and log[0] < 0.1 * tr.timestep(warmed, ETA, DT_MAX)


# ---- ensembles -----------------------------------------------------------------------------------------------------------------

_members = {}


def members(n):
    """Three worlds of n particles after the two fixed steps, then a different close pair planted in each (at the last row,
    the first row and in the middle)."""
    if n not in _members:
        worlds = [synth(n, frac_massive=0.5, seed=100 * n + b) for b in range(3)]
        ms = [m for _, m in worlds]
        s = nb.SimBatch(n, ms)
        s.set_data(np.stack([p for p, _ in worlds]))
        s.update(*WARM)
        state = s.get_data()
        s.close()
        spots = ((n - 1, 0), (0, 1), (n // 2, 2))
        _members[n] = (np.stack([tr.plant(state[b], j, near, gap=1.0e-3 * (b + 1)) for b, (j, near) in enumerate(spots)]), ms)
    return _members[n]


def batch(parts, ms):
    s = nb.SimBatch(parts.shape[1], ms)
    s.set_data(parts)
    s.update(1, 0.0)          # acc of exactly this state
    return s


@pytest.mark.parametrize("n", [69, 600])
def test_ensemble_rows_are_those_of_a_member_alone_and_of_the_replay(n):
    parts, ms = members(n)
    a = batch(parts, ms)
    log, res = a.update_adaptive(STEPS, ETA, DT_MAX)
    got = a.get_data()
    a.close()
    assert log.shape == (STEPS, 3) and len({tuple(bits(log[:, b])) for b in range(3)}) == 3
    # the replay through update(1, dts): before every step each member's host criterion gives its entry
    r = batch(parts, ms)
    clocks = [tr.Clock() for _ in ms]
    for i in range(STEPS):
        state = r.get_data()
        want = [clocks[b].step(tr.timestep(state[b], ETA, DT_MAX)) for b in range(3)]
        assert bits(log[i]) == bits(want), (i, log[i], want)
        r.update(1, log[i])
    want = r.get_data()
    r.close()
    assert got.tobytes() == want.tobytes() and res == [c.result() for c in clocks]
    for b in range(3):          # a one-member ensemble run alone
        one = batch(parts[b:b + 1], ms[b:b + 1])
        log1, res1 = one.update_adaptive(STEPS, ETA, DT_MAX)
        p1 = one.get_data()
        one.close()
        assert bits(log1[:, 0]) == bits(log[:, b]) and res1[0] == res[b] and p1[0].tobytes() == got[b].tobytes(), b


# ---- the World layer -----------------------------------------------------------------------------------------------------------

def test_world_layer_equals_the_pipeline_and_advance_covers_its_span(golden):
    ic = golden("ic_333.bin")
    part, m = ob.partition(ic)
    w = nb.World(ic)
    w.update_gpu(WARM[1], WARM[0])
    assert bits(w.timestep(ETA, DT_MAX)) == bits(tr.timestep(w.particles(), ETA, DT_MAX))
    log_w, res_w = w.update_gpu_adaptive(STEPS, ETA, DT_MAX)
    s = pipeline(part, m)
    log_s, res_s = s.update_adaptive(STEPS, ETA, DT_MAX)
    assert bits(log_w) == bits(log_s) and res_w == res_s and w.particles().tobytes() == s.get_data().tobytes()
    # advance: elapsed == span exactly, and the state is the replay of the concatenated log, idle steps included
    span = 7.3 * float(log_s[-1])
    log, res = w.advance_gpu(span, ETA, DT_MAX, chunk=4)
    assert res["elapsed"] == span and len(log) == res["steps"] + res["idle_steps"] and res["steps"] >= 7
    assert math.fsum(float(x) for x in log[:-1]) < span
    for dt in log:
        s.update(1, float(dt))
    got, want = w.particles(), s.get_data()
    w.close()
    s.close()
    assert got.tobytes() == want.tobytes()


def test_world_batch_advance_covers_the_span_for_every_member():
    parts, ms = members(69)
    wb = nb.WorldBatch(parts)
    order = wb.particles()
    r = nb.SimBatch(69, [int((order[b][:, 6] > 0).sum()) for b in range(3)])
    r.set_data(order)
    wb.update_gpu(0.0, 1)
    r.update(1, 0.0)
    first, _ = wb.update_gpu_adaptive(1, ETA, DT_MAX)
    r.update(1, first[0])
    span = 5.5 * float(first.max())
    log, res = wb.advance_gpu(span, ETA, DT_MAX, chunk=8, max_steps=1 << 16)
    assert all(x["elapsed"] == span for x in res) and log.shape[0] == max(x["steps"] + x["idle_steps"] for x in res)
    assert all(x["steps"] + x["idle_steps"] == log.shape[0] for x in res)
    for row in log:
        r.update(1, row)
    got, want = wb.particles(), r.get_data()
    wb.close()
    r.close()
    assert got.tobytes() == want.tobytes()
