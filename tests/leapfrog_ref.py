"""The kick-drift-kick statement of include/nbody_leapfrog.h (nbody_amd/csrc/leapfrog_common.h) restated in numpy, exactly
(a plain helper module, no GPU), the composition of a leapfrog call from public calls, and wrong statements a checker must
tell from the real one.

numpy evaluates `a * h` and `v + (a * h)` on float32 arrays as two separate float32 operations, each correctly rounded:
that is the statement's mul-then-add, with no fused multiply-add anywhere.  h = 0.5f * dt is one float32 product.

A composition needs one thing from its caller: `force(particles) -> particles`, the one-step dt = 0 update of the object
under test (a World's update_cpu(0, 1), a SimPipeline's set_data / update(1, 0) / get_data, ...).  Particle.acc survives
set_data, so the composition is exact.  An ensemble (B, N, 8) composes like one world; its step sizes may be one per member.

Mutants (compose(..., mutant=name)):
  "merged"     the close of step i - 1 and the open of step i merged into one kick v + a*(h + h') -- one rounding of v, not two
  "old_v"      the drift uses the velocity from before the opening kick
  "fma"        the kicks are fused multiply-adds: v + a*h rounded once
  "stale_acc"  the close uses the acc from before the force evaluation
"""
import numpy as np

F32, F64 = np.float32, np.float64
MUTANTS = ("merged", "old_v", "fma", "stale_acc")
POS, VEL, ACC = slice(0, 2), slice(2, 4), slice(4, 6)


def _dt(dt, particles):
    """dt as float32: a scalar, or one per member of an ensemble (B, N, 8), shaped to broadcast over its rows."""
    dt = np.asarray(dt, dtype=F32)
    return dt.reshape(-1, 1, 1) if dt.ndim == 1 and np.ndim(particles) == 3 else dt


def half(dt):
    with np.errstate(under="ignore"):
        return F32(0.5) * np.asarray(dt, dtype=F32)


def _kick(v, a, h, fused=False):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if fused:
            # a*h is exact in float64; the float64 sum then rounds once more, which moves a float32 result only in rare ties
            return (v.astype(F64) + a.astype(F64) * np.asarray(h, dtype=F64)).astype(F32)
        return v + a * h


def open_(particles, dt, mutant=None, extra_h=None):
    """open(dt): v = v + a*h; x = x + v*dt.  extra_h: the previous step's h, for the merged mutant."""
    p = np.array(particles, dtype=F32, copy=True)
    dt = _dt(dt, p)
    h = half(dt)
    old_v = p[..., VEL].copy()
    if extra_h is not None:
        with np.errstate(over="ignore", under="ignore"):
            h = h + extra_h
    p[..., VEL] = _kick(p[..., VEL], p[..., ACC], h, fused=mutant == "fma")
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        p[..., POS] = p[..., POS] + (old_v if mutant == "old_v" else p[..., VEL]) * dt
    return p


def close(particles, dt, mutant=None, acc=None):
    """close(dt): v = v + a*h with the acc the force step left (acc: another one, for the stale_acc mutant)."""
    p = np.array(particles, dtype=F32, copy=True)
    p[..., VEL] = _kick(p[..., VEL], p[..., ACC] if acc is None else acc, half(_dt(dt, p)), fused=mutant == "fma")
    return p


def compose(force, particles, dts, prime=True, mutant=None):
    """The state after leapfrog steps of sizes `dts`: open, force, close per step, nothing merged.  prime: one force
    evaluation first (what a call does whose object does not know acc to be current)."""
    p = np.array(particles, dtype=F32, copy=True)
    if prime:
        p = force(p)
    dts = [_dt(dt, p) for dt in dts]
    for i, dt in enumerate(dts):
        merged_in = mutant == "merged" and i > 0
        merged_out = mutant == "merged" and i + 1 < len(dts)
        before = p[..., ACC].copy()
        p = open_(p, dt, mutant, extra_h=half(dts[i - 1]) if merged_in else None)
        p = force(p)
        if not merged_out:
            p = close(p, dt, mutant, acc=before if mutant == "stale_acc" else None)
    return p


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=F32).tobytes() == np.ascontiguousarray(b, dtype=F32).tobytes()


def differing(a, b):
    """Particles whose records differ in any bit."""
    a = np.ascontiguousarray(a, dtype=F32).view(np.uint32).reshape(-1, 8)
    b = np.ascontiguousarray(b, dtype=F32).view(np.uint32).reshape(-1, 8)
    return int(np.sum(np.any(a != b, axis=1)))
