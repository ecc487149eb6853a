"""Adaptive time steps on the MI355X at the edges tests/test_gpu_adaptive.py leaves out.  Nothing here measures or sets a
tolerance: every assertion is bit equality against the exact numpy restatement (tests/timestep_ref.py).

  * the device's fmaf / divide / sqrtf(sqrtf()) / clamp chain over the case tables of tests/timestep_cases.py -- a sweep over the
    whole float32 exponent range (subnormal and overflowing a2 and q, negative radii) and a directed list of edge values --
    through the ensemble kernel (one case per member) and through the one-world kernel's atomic-bits path;
  * the one-world kernel's grid-stride loop past one sweep (N > 32 x 256), at exactly 32 full workgroups and one row more,
    with the minimum planted at every sweep boundary; the ensemble kernel over many sweeps with a ragged tail;
  * dt_min on the device, NB_ADAPT_CONTINUE on its own and across the regrow of the log buffer, and the corners of the span
    clip (equality, a span below the first step, a remainder that is a float32 subnormal, one that is 0 in float32).

tests/test_adaptive_cpu.py shows that the tables tell the statement from five wrong ones, and that the host agrees with the
restatement over them."""
import math

import numpy as np
import pytest

import nbody_amd as nb
import timestep_cases as tc
import timestep_ref as tr
from gpu_common import synth
from test_gpu_adaptive import DT_MAX, ETA, batch, bits, members, pipeline, replay, world

pytestmark = pytest.mark.gpu

SWEEP = 4096
WIDE = 3.0e38          # a dt_max that clamps nothing a finite q can give (eta <= 1)


def hexes(x):
    return " ".join(f"{b:08x}" for b in bits(x))


def assert_same_bits(got, want, cases, label):
    """Bit equality of two float32 vectors; on failure the count and the first ten offenders with their inputs in hex."""
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        rows = [f"  case {i}: ax ay radius = {hexes(cases[i])}  ({cases[i]})  device {hexes(got[i])} ({got[i]!r})  "
                f"restatement {hexes(want[i])} ({want[i]!r})" for i in bad[:10]]
        pytest.fail(f"{label}: {bad.size} of {got.size} step sizes differ from the restatement\n" + "\n".join(rows))


_table = []


def table():
    """sweep(4096) + directed(), built once and never written to."""
    if not _table:
        t = np.concatenate([tc.sweep(SWEEP), tc.directed()])
        t.setflags(write=False)
        _table.append(t)
    return _table[0]


# ---- the arithmetic, value by value ----------------------------------------------------------------------------------------

def test_ensemble_kernel_value_sweep():
    """One case per member in particle 0; particles 1 and 2 hold acc = 0 and are skipped.  Only the log is asserted: the step
    each call takes moves these worlds by up to 3e38 and the state is of no interest."""
    cases = table()
    count = cases.shape[0]
    assert count == SWEEP + len(tc.directed())
    parts = np.zeros((count, 3, 8), dtype=np.float32)
    parts[:, :, 0] = np.array([0.0, 1.0e3, -1.0e3], dtype=np.float32)
    parts[:, 0, 4:6], parts[:, 0, 6], parts[:, 0, 7] = cases[:, 0:2], 1.0, cases[:, 2]
    parts[:, 1:, 7] = 0.5
    s = nb.SimBatch(3, [1] * count)
    try:
        for eta in (1.0, 0.1, 3.0e-5):
            s.set_data(parts)
            log, _ = s.update_adaptive(1, eta, WIDE)
            assert_same_bits(log[0], tc.expected(cases, eta, WIDE), cases, f"eta {eta}")
        lo, hi = 1.0e-3, 10.0
        want = tc.expected(cases, 1.0, hi, lo)
        at_lo, at_hi = int(np.sum(want == np.float32(lo))), int(np.sum(want == np.float32(hi)))
        assert at_lo >= 100 and at_hi >= 100 and count - at_lo - at_hi >= 100, (at_lo, at_hi, count)
        s.set_data(parts)
        log, _ = s.update_adaptive(1, 1.0, hi, dt_min=lo)
        assert_same_bits(log[0], want, cases, "dt_min 1e-3, dt_max 10")
    finally:
        s.close()


def test_one_world_kernel_value_sweep_and_pairs():
    """The same values through timestep_kernel: the minimum leaves the workgroup as unsigned bits through an atomic min, and
    nb_hip_timestep reads the uncommitted result.  Then two-particle worlds whose q_i must order as bits the way they do as
    floats: +0 from a -0.0 / negative / NaN radius, 0 against a subnormal, +inf against a finite q, every particle skipped."""
    cases = np.concatenate([tc.directed(), tc.sweep(256)])
    configs = ((1.0, WIDE, 0.0), (0.1, 10.0, 1.0e-3))
    got = np.zeros((len(configs), cases.shape[0]), dtype=np.float32)
    s = nb.SimPipeline(1, 1)
    try:
        for i, c in enumerate(cases):
            s.set_data(tc.particles(c))
            for k, (eta, dt_max, dt_min) in enumerate(configs):
                got[k, i] = s.timestep(eta, dt_max, dt_min)
    finally:
        s.close()
    for k, (eta, dt_max, dt_min) in enumerate(configs):
        assert_same_bits(got[k], tc.expected(cases, eta, dt_max, dt_min), cases, f"one world, eta {eta}, dt in [{dt_min}, {dt_max}]")
    s = nb.SimPipeline(2, 1)
    try:
        for a, b in tc.PAIRS:
            pair = tc.particles(np.stack([tc.named(a), tc.named(b)]))
            for p in (pair, pair[::-1].copy()):
                p[0, 6], p[1, 6] = 1.0, 0.0
                s.set_data(p)
                dt, want = np.float32(s.timestep(1.0, WIDE)), tr.timestep(p, 1.0, WIDE)
                assert bits(dt) == bits(want), (a, b, hexes(p[:, [4, 5, 7]]), float(dt), float(want))
    finally:
        s.close()
    assert bits(tc.expected_world(np.stack([tc.named("radius -0"), tc.named("q = 1")]), 1.0, WIDE)) == bits(0.0)
    assert bits(tc.expected_world(np.stack([tc.named("acc (0, 0)"), tc.named("acc (NaN, 1)")]), 1.0, WIDE)) == bits(WIDE)


# ---- more than one sweep of the grid ------------------------------------------------------------------------------------------

MASSIVE = 64               # so that a step costs little
PLANT = (1.0e7, 0.0, 1.0e-6)          # q = 1e-20
_backgrounds = {}


def background(n, mass_len=MASSIVE):
    """synth(n) with `mass_len` massive particles and acc / radius from the sweep, so subnormals and skipped rows are
    present; the exponents are clamped so that every q stays above 1e-12 (a2 < 2^19, radius >= 2^-16 and positive)."""
    if (n, mass_len) not in _backgrounds:
        part, _ = synth(n, frac_massive=1.0, seed=n)
        part[mass_len:, 6] = 0.0
        cases = tc.sweep(n, seed=n, acc_exp=(tc.ACC_EXP[0], 8), radius_exp=(-16, tc.RADIUS_EXP[1]), negative_radius=0.0)
        part[:, 4:6], part[:, 7] = cases[:, 0:2], cases[:, 2]
        part[5::97, 4:6] = 0.0                  # skipped rows: acc = 0, and a NaN acc
        part[7::101, 4] = np.nan
        q = tr.q_all(part)
        assert q.min() > 1.0e-12 and np.isinf(q).sum() > n // 64
        part.setflags(write=False)
        _backgrounds[(n, mass_len)] = part
    return _backgrounds[(n, mass_len)]


def planted(base, j):
    p = np.array(base, copy=True)
    p[j, 4:6], p[j, 7] = PLANT[0:2], PLANT[2]
    assert int(np.argmin(tr.q_all(p))) == j
    return p


@pytest.mark.parametrize("n,spots", [(2 * 8192 + 300, (0, 8191, 8192, 16383, 16384, -1)), (8192, (-1,)), (8193, (-1,))],
                         ids=["two sweeps and 300 rows", "exactly 32 full workgroups", "32 workgroups and one row"])
def test_one_world_grid_stride_past_one_sweep(n, spots):
    """timestep_groups caps the grid at 32 x 256 threads: beyond 8 192 rows a thread takes a second and a third row.  The
    minimum sits at each sweep boundary in turn; a wrong stride or a dropped tail misses it."""
    base = background(n)
    s = nb.SimPipeline(n, MASSIVE)
    try:
        s.set_data(base)
        free = np.float32(s.timestep(ETA, DT_MAX))
        assert bits(free) == bits(tr.timestep(base, ETA, DT_MAX)) and free < np.float32(DT_MAX)
        for j in spots:
            j = j % n
            p = planted(base, j)
            s.set_data(p)
            dt, want = np.float32(s.timestep(ETA, DT_MAX)), tr.timestep(p, ETA, DT_MAX)
            assert bits(dt) == bits(want) and dt < free, (n, j, float(dt), float(want), float(free))
    finally:
        s.close()


def test_one_world_replay_past_one_sweep():
    """The replay contract at N = 16 684: the first step size comes from the uploaded acc, the next two from the stepper's."""
    n = 2 * 8192 + 300
    p = planted(background(n), n - 1)
    a, b = pipeline(p, MASSIVE, warm=False), pipeline(p, MASSIVE, warm=False)
    try:
        log, res = a.update_adaptive(3, ETA, DT_MAX)
        clock = tr.Clock()
        replay(b, log, clock)
        assert a.get_data().tobytes() == b.get_data().tobytes() and res == clock.result(), (res, clock.result())
        assert res["steps"] == 3 and bits(log[0]) == bits(tr.timestep(p, ETA, DT_MAX))
    finally:
        a.close()
        b.close()


def test_ensemble_many_sweeps_with_a_ragged_tail():
    """2 999 rows are 11 full sweeps of a member's one workgroup plus 183 rows; member b holds its minimum at spots[b]."""
    n, spots = 2999, (0, 255, 256, 2815, 2816, 2998)
    base = background(n, 1)
    parts = np.stack([planted(base, j) for j in spots])
    s = nb.SimBatch(n, [1] * len(spots))
    try:
        s.set_data(parts)
        log, _ = s.update_adaptive(1, ETA, DT_MAX)
    finally:
        s.close()
    want = [tr.timestep(parts[b], ETA, DT_MAX) for b in range(len(spots))]
    assert bits(log[0]) == bits(want), (log[0], want)
    assert np.all(log[0] < tr.timestep(base, ETA, DT_MAX))


# ---- dt_min ---------------------------------------------------------------------------------------------------------------------

def contract(part, m, steps, warm=True, **cfg):
    """update_adaptive(steps, **cfg) against the replay through update(1, log[i]) on a twin: the log is the host criterion of
    the state before each step, the states and the result agree.  Returns (log, result, state)."""
    a, b = pipeline(part, m, warm), pipeline(part, m, warm)
    try:
        log, res = a.update_adaptive(steps, ETA, DT_MAX, **cfg)
        clock = tr.Clock(cfg.get("span", math.inf))
        replay(b, log, clock, dt_min=cfg.get("dt_min", 0.0))
        got, want = a.get_data(), b.get_data()
    finally:
        a.close()
        b.close()
    assert got.tobytes() == want.tobytes() and res == clock.result(), (cfg, res, clock.result())
    return log, res, got


def free_log(golden, steps):
    part, m = world(333, golden)
    a = pipeline(part, m)
    log, _ = a.update_adaptive(steps, ETA, DT_MAX)
    a.close()
    return log


def test_dt_min_binds_on_the_device(golden):
    part, m = world(333, golden)
    dt_min = float(np.float32(np.median(free_log(golden, 6))))
    log, res, _ = contract(part, m, 6, dt_min=dt_min)
    assert np.sum(log == np.float32(dt_min)) >= 1 and np.sum(log > np.float32(dt_min)) >= 1 and np.all(log >= np.float32(dt_min)), (log, dt_min)
    assert res["dt_smallest"] == dt_min
    # dt_min == dt_max: every step is that size, and the state is the fixed-step one
    d = 0.01
    a, b = pipeline(part, m), pipeline(part, m)
    try:
        log, res = a.update_adaptive(6, ETA, d, dt_min=d)
        b.update(6, d)
        assert bits(log) == bits([d] * 6) and a.get_data().tobytes() == b.get_data().tobytes()
        assert res["steps"] == 6 and res["dt_last"] == float(np.float32(d)) == res["dt_smallest"]
    finally:
        a.close()
        b.close()


# ---- NB_ADAPT_CONTINUE ------------------------------------------------------------------------------------------------------------

def test_continue_across_the_regrow_of_the_log(golden):
    """5 steps, then 70 more with resume=True (more than the 64 floats the first call allocated: the buffer is regrown and the
    records are carried over), against 75 in one call."""
    part, m = world(333, golden)
    whole = pipeline(part, m)
    log, res = whole.update_adaptive(75, ETA, DT_MAX)
    whole.close()
    assert res["steps"] == 75
    span = math.fsum(float(x) for x in log[:20]) + 0.5 * float(log[20])          # ends inside the second call
    for cfg in ({}, {"span": span}):
        one, two = pipeline(part, m), pipeline(part, m)
        try:
            log1, res1 = one.update_adaptive(75, ETA, DT_MAX, **cfg)
            head, first = two.update_adaptive(5, ETA, DT_MAX, **cfg)
            tail, second = two.update_adaptive(70, ETA, DT_MAX, resume=True, **cfg)
            assert bits(np.concatenate([head, tail])) == bits(log1) and second == res1, (cfg, second, res1)
            assert first["steps"] == 5 and one.get_data().tobytes() == two.get_data().tobytes()
        finally:
            one.close()
            two.close()
        if cfg:
            assert res1["elapsed"] == span and res1["steps"] == 21 and res1["idle_steps"] == 54 and bits(log1[:20]) == bits(log[:20])
        else:
            assert bits(log1) == bits(log) and res1 == res
    # resume without a previous call is ignored
    a, b = pipeline(part, m), pipeline(part, m)
    try:
        la, ra = a.update_adaptive(5, ETA, DT_MAX, resume=True)
        lb, rb = b.update_adaptive(5, ETA, DT_MAX)
        assert bits(la) == bits(lb) == bits(log[:5]) and ra == rb and a.get_data().tobytes() == b.get_data().tobytes()
    finally:
        a.close()
        b.close()


def test_ensemble_continue_across_the_regrow_of_the_log():
    parts, ms = members(69)
    whole = batch(parts, ms)
    log, res = whole.update_adaptive(42, ETA, DT_MAX)
    whole.close()
    span = math.fsum(float(x) for x in log[:10, 0]) + 0.5 * float(log[10, 0])          # member 0 ends inside the second call
    for cfg in ({}, {"span": span}):
        one, two = batch(parts, ms), batch(parts, ms)
        try:
            log1, res1 = one.update_adaptive(42, ETA, DT_MAX, **cfg)
            head, first = two.update_adaptive(2, ETA, DT_MAX, **cfg)
            tail, second = two.update_adaptive(40, ETA, DT_MAX, resume=True, **cfg)
            assert bits(np.concatenate([head, tail])) == bits(log1) and second == res1, (cfg, second, res1)
            assert all(r["steps"] == 2 for r in first) and one.get_data().tobytes() == two.get_data().tobytes()
        finally:
            one.close()
            two.close()
        if cfg:
            assert res1[0]["elapsed"] == span and res1[0]["steps"] == 11 and res1[0]["idle_steps"] == 31
        else:
            assert bits(log1) == bits(log) and res1 == res
    a, b = batch(parts, ms), batch(parts, ms)
    try:
        la, ra = a.update_adaptive(2, ETA, DT_MAX, resume=True)
        lb, rb = b.update_adaptive(2, ETA, DT_MAX)
        assert bits(la) == bits(lb) == bits(log[:2]) and ra == rb and a.get_data().tobytes() == b.get_data().tobytes()
    finally:
        a.close()
        b.close()


# ---- the corners of the span clip -------------------------------------------------------------------------------------------------

def test_span_clip_corners(golden):
    part, m = world(333, golden)
    free = free_log(golden, 3)
    before = pipeline(part, m)
    start = before.get_data()
    before.close()
    # (double)dt == rem: the left-to-right float64 sum of three float32 step sizes is exact, so the third remainder is the
    # third free step size itself
    span = float(free[0]) + float(free[1]) + float(free[2])
    assert span - (float(free[0]) + float(free[1])) == float(free[2])
    log, res, _ = contract(part, m, 6, span=span)
    assert bits(log[:3]) == bits(free) and not log[3:].any() and res["elapsed"] == span and (res["steps"], res["idle_steps"]) == (3, 3)
    # a span below the first free step
    span = 0.375 * float(free[0])
    log, res, _ = contract(part, m, 6, span=span)
    assert bits(log[0]) == bits(np.float32(span)) and not log[1:].any() and res["elapsed"] == span and (res["steps"], res["idle_steps"]) == (1, 5)
    # (float)rem is a float32 subnormal: one step of that size
    log, res, _ = contract(part, m, 6, span=1.0e-40)
    assert bits(log[0]) == bits(np.float32(1.0e-40)) and 0 < log[0] < np.float32(2.0 ** -126) and not log[1:].any()
    assert res["elapsed"] == 1.0e-40 and (res["steps"], res["idle_steps"]) == (1, 5) and res["dt_last"] == float(np.float32(1.0e-40))
    # (float)rem is 0: the span is covered by a step of size 0, which counts as idle
    log, res, state = contract(part, m, 6, span=1.0e-50)
    assert not log.any() and res["elapsed"] == 1.0e-50 and (res["steps"], res["idle_steps"]) == (0, 6)
    assert res["dt_last"] == 0.0 and res["dt_smallest"] == 0.0
    assert np.array_equal(state[:, 0:4], start[:, 0:4])


def ensemble_contract(parts, ms, steps, span):
    """The ensemble's replay contract: before every step each member's host criterion, clipped by its own clock, is its entry."""
    a, r = batch(parts, ms), batch(parts, ms)
    try:
        log, res = a.update_adaptive(steps, ETA, DT_MAX, span=span)
        clocks = [tr.Clock(span) for _ in ms]
        for i in range(steps):
            state = r.get_data()
            want = [clocks[b].step(tr.timestep(state[b], ETA, DT_MAX)) for b in range(len(ms))]
            assert bits(log[i]) == bits(want), (i, log[i], want)
            r.update(1, log[i])
        assert a.get_data().tobytes() == r.get_data().tobytes() and res == [c.result() for c in clocks]
        return log, res, a.get_data()
    finally:
        a.close()
        r.close()


def test_ensemble_span_clip_corners():
    parts, ms = members(69)
    s = batch(parts, ms)
    free, _ = s.update_adaptive(3, ETA, DT_MAX)
    s.close()
    s = batch(parts, ms)
    start = s.get_data()
    s.close()
    span = float(free[0, 0]) + float(free[1, 0]) + float(free[2, 0])          # equality for member 0; the others clip where they may
    log, res, _ = ensemble_contract(parts, ms, 6, span)
    assert bits(log[:3, 0]) == bits(free[:, 0]) and not log[3:, 0].any() and (res[0]["steps"], res[0]["idle_steps"]) == (3, 3)
    assert res[0]["elapsed"] == span
    log, res, state = ensemble_contract(parts, ms, 6, 1.0e-50)
    assert not log.any() and all(r["elapsed"] == 1.0e-50 and (r["steps"], r["idle_steps"]) == (0, 6) for r in res)
    assert np.array_equal(state[:, :, 0:4], start[:, :, 0:4])
