"""The adaptive step-size criterion of include/nbody_adaptive.h restated in numpy, exactly (a plain helper module, no GPU).

Every float32 operation of the statement is evaluated in float64 and rounded once to float32, which is the correctly rounded
float32 result for each of them:
  * ay * ay: the float64 product of two float32 values is exact (48 bits), so its rounding to float32 is the float32 product;
  * fmaf(ax, ax, ay2): ax * ax is exact in float64; the float64 sum with ay2 can be inexact, so its error is recovered exactly
    (two-sum) and folded back as a sticky bit -- the sum is moved to the ODD neighbour on the error's side ("round to odd"),
    after which the rounding to float32 (53 >= 24 + 2 bits) is the rounding of the exact sum;
  * radius / a2, sqrtf: float64 division / square root of float32 operands rounded to float32 is correctly rounded
    (53 >= 2 * 24 + 2 bits: double rounding is innocuous for these operations);
  * eta * s: the float64 product is exact.
numpy's float64 -> float32 cast rounds to nearest even and produces subnormals.  The span clip is float64 in the statement."""
import math

import numpy as np

F32, F64 = np.float32, np.float64


def a2_f32(ax, ay):
    """fmaf(ax, ax, ay * ay) in float32, exactly; arrays of float32."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        ay2 = (ay.astype(F64) * ay.astype(F64)).astype(F32).astype(F64)
        p = ax.astype(F64) * ax.astype(F64)
        s = p + ay2
        bb = s - p
        err = (p - (s - bb)) + (ay2 - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.uint64) & np.uint64(1)) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def q_all(particles):
    """q_i of every particle (float32); +inf for a skipped one."""
    a = np.ascontiguousarray(particles, dtype=F32)
    a2 = a2_f32(a[:, 4], a[:, 5])
    use = (a2 > 0) & np.isfinite(a2)
    r = np.where(a[:, 7] > 0, a[:, 7], F32(0)).astype(F64)          # radius > 0 ? radius : +0 (-0, < 0, NaN -> +0)
    q = np.full(a.shape[0], np.inf, dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        q[use] = (r[use] / a2[use].astype(F64)).astype(F32)
    return q


def q_min(particles):
    """min_i q_i; no q_i is a NaN, so numpy's minimum is the one the statement takes with `<`."""
    q = q_all(particles)
    assert not np.isnan(q).any()
    return q.min() if q.size else F32(np.inf)


def dt_of_q(q, eta, dt_min, dt_max):
    with np.errstate(over="ignore", under="ignore"):
        s = np.sqrt(F64(np.sqrt(F64(q)).astype(F32))).astype(F32) if np.isfinite(q) else F32(np.inf)
        raw = F32(F64(F32(eta)) * F64(s))
    return F32(min(max(raw, F32(dt_min)), F32(dt_max)))


def timestep(particles, eta, dt_max, dt_min=0.0):
    """The criterion without the span clip: what GetWorldTimestep / nb_hip_timestep return, as numpy float32."""
    return dt_of_q(q_min(particles), eta, dt_min, dt_max)


def clip(dt, span, t):
    """The span clip: (float32 dt, float64 t) after one step."""
    rem = float(span) - float(t)
    if rem <= 0.0:
        return F32(0.0), float(t)
    if float(dt) >= rem:
        return F32(rem), float(span)
    return F32(dt), float(t) + float(dt)


class Clock:
    """The bookkeeping of one adaptive call: feed it each step's unclipped dt, read the clipped one and the result."""

    def __init__(self, span=math.inf):
        self.span, self.t, self.steps, self.idle_steps, self.dt_last, self.dt_smallest = span, 0.0, 0, 0, F32(0), F32(0)

    def step(self, dt):
        dt, self.t = clip(dt, self.span, self.t)
        if dt > 0:
            self.steps += 1
            self.dt_last = dt
            if self.dt_smallest == 0 or dt < self.dt_smallest:
                self.dt_smallest = dt
        else:
            self.idle_steps += 1
        return dt

    def result(self):
        return {"elapsed": self.t, "steps": self.steps, "idle_steps": self.idle_steps, "dt_last": float(self.dt_last),
                "dt_smallest": float(self.dt_smallest)}


def plant(particles, j, near, gap=1.0e-3):
    """A copy in which particle j sits `gap` beside particle `near` (a massive one) with a radius of 1e-6: after one step j
    holds by far the largest |acc| over the smallest softening, so it alone sets the minimum q."""
    a = np.array(particles, dtype=F32, copy=True)
    a[j, 0:2] = a[near, 0:2] + F32(gap)
    a[j, 2:4] = a[near, 2:4]
    a[j, 7] = F32(1.0e-6)
    return a
