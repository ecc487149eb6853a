"""Case tables for the adaptive step-size criterion (a plain helper module, no GPU): deterministic (ax, ay, radius) triples as
float32 -- a random sweep over the whole float32 exponent range and a directed list of edge values -- with the step size the
exact restatement (tests/timestep_ref.py) gives for each as a one-particle world, and the step size five WRONG statements would
give.  The mutants exist only so that tests/test_adaptive_cpu.py can show that the tables tell the real statement from them; a
GPU test that compares the device with the restatement over these tables is then not vacuous."""
import numpy as np

import timestep_ref as tr

F32, F64 = np.float32, np.float64
FLT_MIN, FLT_MAX, SUB_MIN = F32(2.0 ** -126), np.finfo(F32).max, F32(2.0 ** -149)
NAN, INF = F32(np.nan), F32(np.inf)
ACC_EXP, RADIUS_EXP = (-75, 64), (-149, 127)
NEAR = 0.25


def _values(rng, exps):
    """Positive float32 values 1.m x 2^e with random 23-bit mantissas (rounded into the subnormals where e is below -126)."""
    mant = 1.0 + rng.integers(0, 1 << 23, exps.shape[0]) / float(1 << 23)
    return np.ldexp(mant, exps).astype(F32)


def sweep(count, seed=20240, acc_exp=ACC_EXP, radius_exp=RADIUS_EXP, negative_radius=0.125):
    """(count, 3) random triples.  The binary exponents of ax and ay are uniform in acc_exp (a2 from below the subnormals,
    through them, to overflow), that of the radius in radius_exp; signs of ax and ay are random and the radius is negative in
    `negative_radius` of the cases.  About one case in eight has ay = 0.  A share of NEAR has |ax| and |ay| within a factor of 4
    of each other, a positive radius and a q inside the normal numbers: there the fused sum rounds differently from the unfused
    and the once-rounded one, and only there can dt show it.  The fourth root hides three of four one-ulp differences of q, so
    a share of one in eight left mutants (a) and (b) at 35 and 26 differing cases of 4 096, below the 50 that
    tests/test_adaptive_cpu.py asks for; a quarter gives 57 and 59."""
    rng = np.random.default_rng(seed)
    ex = rng.integers(acc_exp[0], acc_exp[1] + 1, count)
    ey = rng.integers(acc_exp[0], acc_exp[1] + 1, count)
    kind = rng.random(count)
    near = kind < NEAR
    ey = np.where(near, np.clip(ex + rng.integers(-1, 2, count), acc_exp[0], acc_exp[1]), ey)
    ax = _values(rng, ex) * np.where(rng.random(count) < 0.5, F32(-1), F32(1))
    ay = _values(rng, ey) * np.where(rng.random(count) < 0.5, F32(-1), F32(1))
    ay = np.where((kind >= NEAR) & (kind < NEAR + 0.125), F32(0), ay)
    er = rng.integers(radius_exp[0], radius_exp[1] + 1, count)
    # a near case is there to show a one-ulp difference of a2 in dt, which it cannot where q leaves the float32 range: its
    # radius exponent is uniform over the part of radius_exp that keeps q = radius / a2 inside the normal numbers
    ea2 = 2 * np.maximum(ex, ey) + 1
    lo, hi = np.clip(ea2 - 124, radius_exp[0], radius_exp[1]), np.clip(ea2 + 124, radius_exp[0], radius_exp[1])
    er = np.where(near, lo + (rng.integers(0, 1 << 30, count) % (hi - lo + 1)), er)
    radius = _values(rng, er)
    radius = radius * np.where((rng.random(count) < negative_radius) & ~near, F32(-1), F32(1))
    return np.stack([ax, ay, radius], axis=1).astype(F32)


_DIRECTED = [
    # the radius, over an ordinary a2 = 25
    ("radius +0", 3.0, 4.0, 0.0),
    ("radius -0", 3.0, 4.0, -0.0),
    ("radius -1", 3.0, 4.0, -1.0),
    ("radius NaN", 3.0, 4.0, NAN),
    ("radius +inf", 3.0, 4.0, INF),
    ("radius -inf", 3.0, 4.0, -INF),
    ("radius smallest subnormal", 3.0, 4.0, SUB_MIN),
    ("radius -smallest subnormal", 3.0, 4.0, -SUB_MIN),
    ("radius FLT_MAX", 3.0, 4.0, FLT_MAX),
    ("radius FLT_MAX over a2 < 1", 0.5, 0.25, FLT_MAX),
    # the acceleration, under an ordinary radius
    ("acc (0, 0)", 0.0, 0.0, 0.5),
    ("acc (-0, -0)", -0.0, -0.0, 0.5),
    ("acc (NaN, 1)", NAN, 1.0, 0.5),
    ("acc (1, NaN)", 1.0, NAN, 0.5),
    ("acc (inf, 0)", INF, 0.0, 0.5),
    ("acc (-inf, NaN)", -INF, NAN, 0.5),
    ("acc (1e-23, 0): a2 below half the smallest subnormal", 1.0e-23, 0.0, 0.5),
    ("acc (3e-23, 0): a2 the smallest subnormal", 3.0e-23, 0.0, 0.5),
    ("acc (1e-20, 0): a2 subnormal", 1.0e-20, 0.0, 0.5),
    ("acc (0, 1e-20): ay * ay subnormal", 0.0, 1.0e-20, 0.5),
    ("acc (7e-21, 8e-21): both products subnormal", 7.0e-21, 8.0e-21, 0.5),
    ("acc (1e-30, 0): a2 = 0 after rounding", 1.0e-30, 0.0, 0.5),
    ("acc (1.9e19, 1.9e19): each product overflows", 1.9e19, 1.9e19, 0.5),
    ("acc (1.4e19, 1.4e19): a2 overflows only in the sum", 1.4e19, 1.4e19, 0.5),
    ("acc (1.8e19, 4e18): a2 just below overflow", 1.8e19, 4.0e18, 0.5),
    ("acc (FLT_MAX, 0)", FLT_MAX, 0.0, 0.5),
    # q
    ("q subnormal", 1.0e5, 0.0, 1.0e-30),
    ("q the smallest subnormal", 1.0, 0.0, SUB_MIN),
    ("q the smallest subnormal from a normal radius", 2048.0, 2048.0, FLT_MIN),
    ("q rounds to 0", 2.0, 0.0, SUB_MIN),
    ("q = 2^-150: a tie that rounds to 0", 1.0, 1.0, SUB_MIN),
    ("q = 1.5 x 2^-149: a tie that rounds up", 1.0, 1.0, 3.0 * float(SUB_MIN)),
    ("q rounds to 0 from a normal radius", 1.0e19, 0.0, 1.0e-10),
    ("q overflows from a finite radius and a subnormal a2", 1.0e-20, 0.0, 1.0),
    ("q overflows from FLT_MAX and a subnormal a2", 3.0e-23, 0.0, FLT_MAX),
    ("q finite from a subnormal radius and a subnormal a2", 1.0e-20, 0.0, 1.0e-42),
    ("q = 2^-126", 1.0, 0.0, FLT_MIN),
    ("q the largest subnormal", 1.0, 0.0, np.nextafter(FLT_MIN, F32(0))),
    ("q just above 2^-126", 1.0, 0.0, np.nextafter(FLT_MIN, F32(1))),
    ("q just below 2^-126 by division", 3.0, 0.0, 9.0 * float(np.nextafter(FLT_MIN, F32(0)))),
    ("q = FLT_MAX", 1.0, 0.0, FLT_MAX),
    ("q = 1", 0.6, 0.8, 1.0),
]


def directed_names():
    return [c[0] for c in _DIRECTED]


def directed():
    """(len, 3) float32: the fixed list of edge cases; directed_names() names the rows."""
    return np.array([c[1:] for c in _DIRECTED], dtype=F64).astype(F32)


def named(name):
    """The (ax, ay, radius) row of one directed case."""
    return directed()[directed_names().index(name)]


# two-particle worlds (names of directed cases): what crosses workgroups as unsigned bits must order as the floats do
PAIRS = [
    ("radius -0", "q = 1"),                                       # q = +0 from a -0.0 radius wins against a positive q
    ("radius -1", "q the smallest subnormal"),
    ("radius NaN", "q = FLT_MAX"),
    ("q rounds to 0", "q subnormal"),                             # q = 0 against a subnormal q
    ("q the smallest subnormal", "q subnormal"),
    ("q the largest subnormal", "q = 2^-126"),
    ("radius +inf", "q = 1"),                                     # a q of +inf from a particle that is NOT skipped loses
    ("q overflows from a finite radius and a subnormal a2", "q = FLT_MAX"),
    ("acc (0, 0)", "acc (NaN, 1)"),                               # every particle skipped: dt_max
    ("acc (inf, 0)", "acc (1.4e19, 1.4e19): a2 overflows only in the sum"),
]


def particles(cases, mass=1.0):
    """(n, 8) particle rows at the origin holding the cases' acc and radius."""
    cases = np.asarray(cases, dtype=F32).reshape(-1, 3)
    a = np.zeros((cases.shape[0], 8), dtype=F32)
    a[:, 4:6], a[:, 6], a[:, 7] = cases[:, 0:2], mass, cases[:, 2]
    return a


def expected(cases, eta, dt_max, dt_min=0.0):
    """The restatement's float32 dt of every case as a one-particle world (q_all of n rows is n one-particle minima)."""
    q = tr.q_all(particles(cases))
    assert not np.isnan(q).any()
    return np.array([tr.dt_of_q(x, eta, dt_min, dt_max) for x in q], dtype=F32)


def expected_world(cases, eta, dt_max, dt_min=0.0):
    """The restatement's dt of ONE world that holds all the cases."""
    return tr.timestep(particles(cases), eta, dt_max, dt_min)


# ---- the mutants: wrong statements, written next to the real one ----------------------------------------------------------

def _add_f32(p, y):
    """float32(p + y) of float64 p, y, rounded once: the float64 sum's error is recovered (two-sum) and folded back as a
    sticky bit (round to odd), as tests/timestep_ref.py a2_f32 does."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + y
        bb = s - p
        err = (p - (s - bb)) + (y - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def _ftz(x):
    return np.where(np.abs(x) < FLT_MIN, np.copysign(F32(0), x), x).astype(F32)


def _q(cases, mutant):
    ax, ay, r = (np.ascontiguousarray(cases[:, k], dtype=F32) for k in range(3))
    flush = _ftz if mutant == "d" else (lambda x: x)
    ax, ay, r = flush(ax), flush(ay), flush(r)
    with np.errstate(all="ignore"):
        x2, y2 = ax.astype(F64) * ax.astype(F64), ay.astype(F64) * ay.astype(F64)          # exact
        if mutant == "a":            # both products rounded, then added: no fma
            a2 = (x2.astype(F32).astype(F64) + y2.astype(F32).astype(F64)).astype(F32)
        elif mutant == "b":          # ax^2 + ay^2 rounded once
            a2 = _add_f32(x2, y2)
        else:                        # the statement: fmaf(ax, ax, ay * ay)
            a2 = _add_f32(x2, y2.astype(F32).astype(F64))
        a2 = flush(a2)
        use = (a2 > 0) & np.isfinite(a2)
        rr = (r if mutant == "e" else np.where(r > 0, r, F32(0))).astype(F64)
        if mutant == "c":            # radius * (1 / a2), the reciprocal rounded
            q = (rr * (1.0 / a2.astype(F64)).astype(F32).astype(F64)).astype(F32)
        else:
            q = (rr / a2.astype(F64)).astype(F32)
        return flush(np.where(use, q, INF).astype(F32))


def _dt(q, eta, dt_min, dt_max, mutant):
    flush = _ftz if mutant == "d" else (lambda x: x)
    with np.errstate(all="ignore"):
        s = flush(np.sqrt(q.astype(F64)).astype(F32))
        s = flush(np.sqrt(s.astype(F64)).astype(F32))
        raw = flush((F64(F32(eta)) * s.astype(F64)).astype(F32))
        return np.fmin(np.fmax(raw, F32(dt_min)), F32(dt_max)).astype(F32)          # C's fmaxf / fminf: a NaN loses


def mutant_dt(cases, mutant, eta, dt_max, dt_min=0.0):
    """dt of every case as a one-particle world under a wrong statement; mutant None is the real statement (vectorised: it must
    equal expected()).
      "a"  both products rounded and then added, no fma
      "b"  the fully fused ax^2 + ay^2, rounded once
      "c"  radius * (1 / a2) with the reciprocal rounded
      "d"  subnormals flushed to zero, on input and on the output of every operation
      "e"  the radius not clamped at +0 (see mutant_e_world for what it is for)"""
    cases = np.asarray(cases, dtype=F32).reshape(-1, 3)
    return _dt(_q(cases, mutant), eta, dt_min, dt_max, mutant)


def mutant_e_world(cases, eta, dt_max, dt_min=0.0):
    """(e) dt of one world holding the cases when q_i = radius / a2 without the clamp of the radius at +0 and the minimum is taken on the raw
    unsigned bits: a q of -0.0 or below loses against everything instead of winning as +0."""
    q = _q(np.asarray(cases, dtype=F32).reshape(-1, 3), "e")
    low = q.view(np.uint32).min()
    return _dt(np.array([low], dtype=np.uint32).view(F32), eta, dt_min, dt_max, "e")[0]
