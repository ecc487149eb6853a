"""Non-finite state (TEST INFRASTRUCTURE): the case table and the checkers of tests/test_nonfinite_cpu.py and
tests/test_gpu_nonfinite.py.  Imports no GPU code of its own; the CPU file shows that the checkers have teeth.

A case is a name plus a function that plants one thing into a copy of a partitioned world (ob.partition has run, so the
index of the plant is known).  The base worlds are gpu_common.synth at extent 100: sources sit ~1e2 apart, G*m is ~1e3..4e5,
so an ordinary pair term is ~1e-1..1e2 and every overflow threshold is far away until a plant moves something to it.
Every planted magnitude is >= 1e3 away from the threshold it is meant to cross or to stay clear of (fp32 max 3.4e38):
the class of a value then cannot hinge on the last bit of G*m*rsq*rsq^2 against G*m/(r*r^2).

  3e38        dx^2 = 9e76 overflows: r^2 = inf, the term is dx * 0 = 0
  1e15        r * r^2 = 2.8e45 overflows: the term is 0 in the reference's form, ~1e-26 (a denormal factor) in the rsq form
  1e18        r^2 = 2e36 is finite, r*r^2 = 2.8e54 overflows: the term is 0 again (rsq route: 7e-19 * 5e-37 * G*m underflows)
  3.3e38      G*m = 3.3e39 = +inf: every receiver gets dx * inf
  1e37        G*m = 1e38 is finite; at r^2 = 2e-4 the factor is 3.5e43 = inf, at r ~ 1e2 the term is ~1e34
  1e-40       a denormal radius: the self term's r*r^2 = 1e-60 is 0 in fp32, G*m / 0 = inf, 0 * inf = NaN
  1e-36       a normal radius with the same effect on a coincident pair
"""
import numpy as np

import nbody_amd as nb
import oracle_binding as ob
from energy_ref import assert_energy_close, energy_f64
from gpu_common import acc_bound, synth

DT = 0.01
FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3
INF, QNAN = np.float32(np.inf), np.float32(np.nan)


def classes(x):
    """array -> uint8 array of the same shape: 0 finite, 1 +inf, 2 -inf, 3 NaN"""
    x = np.asarray(x)
    c = np.zeros(x.shape, dtype=np.uint8)
    c[np.isposinf(x)] = POS_INF
    c[np.isneginf(x)] = NEG_INF
    c[np.isnan(x)] = NAN
    return c


def class_counts(x):
    """(finite, +inf, -inf, NaN) counts"""
    return tuple(int(v) for v in np.bincount(classes(x).reshape(-1), minlength=4))


def world(n, frac=0.6, seed=0):
    """gpu_common.synth at extent 100, partitioned: (particles, M)"""
    return synth(n, frac_massive=frac, seed=seed, extent=100.0)


# ---- the case table ------------------------------------------------------------------------------------------------------------

class Case:
    """kind "contain": the plant sits on massless row `row(n, m)` and nothing else may change by a bit; "source": on source
    `row(n, m)`; "world": several rows.  fits(n, m) says whether the world has the rows the plant needs."""

    def __init__(self, name, kind, plant, row=None, fits=None):
        self.name, self.kind, self._plant, self._row, self._fits = name, kind, plant, row, fits

    def fits(self, n, m):
        return self._fits(n, m) if self._fits else True

    def row(self, n, m):
        return self._row(n, m) if self._row else None

    def plant(self, part, m):
        out = part.copy()
        n = part.shape[0]
        assert self.fits(n, m), (self.name, n, m)
        self._plant(out, m, self.row(n, m))
        assert np.array_equal(out[:, 6] > 0, part[:, 6] > 0), "a plant must leave the partition alone"
        return out

    def __repr__(self):
        return self.name


def _set(cols, values):
    def plant(a, m, i):
        a[i, cols] = values
    return plant


CONTAIN_VALUES = {
    "pos-nan": _set(slice(0, 2), QNAN),
    "pos-inf-finite": _set(slice(0, 1), INF),          # (+inf, the row's own y)
    "vel-inf": _set(slice(2, 4), INF),
    "vel-nan": _set(slice(2, 4), QNAN),
}
CONTAIN_ROWS = {"first-massless": lambda n, m: m, "last": lambda n, m: n - 1}

SOURCE_VALUES = {
    "pos-nan": _set(slice(0, 2), QNAN),
    "x-inf": _set(slice(0, 1), INF),
    "x-3e38": _set(slice(0, 1), np.float32(3e38)),
    "far-1e18": _set(slice(0, 2), np.float32(1e18)),
    "gm-inf": _set(slice(6, 7), np.float32(3.3e38)),
}
SOURCE_ROWS = {"0": lambda n, m: 0, "255": lambda n, m: 255, "256": lambda n, m: 256, "M-1": lambda n, m: m - 1}

NEAR = np.array([(1, 1), (1, -1), (-1, 1), (-1, -1), (2, 1), (-1, 2)], dtype=np.float32) * np.float32(1e-2)


def _near_overflow(a, m, _):
    """Source 0 at the origin with G*m = 1e38; the last six rows 1e-2 away with radius 1e-6: only their factor overflows.
    Everything else is kept more than 1 away from the origin, where the term is < 1e38 (and ~1e34 at the usual 1e2)."""
    n = a.shape[0]
    a[0, 0:2] = 0.0
    a[0, 6] = np.float32(1e37)
    close = np.hypot(a[1:n - 6, 0], a[1:n - 6, 1]) < 1.0
    a[1:n - 6, 0][close] += np.float32(5.0)
    a[n - 6:, 0:2] = NEAR
    a[n - 6:, 7] = np.float32(1e-6)


def _denormal_radii(a, m, _):
    a[:m, 7] = np.float32(1e-40)


def _zero_radius(a, m, _):
    """tests/test_gpu_parity.py's coincidences: body 0 has radius 0 and meets itself; the last row has radius 0 and sits on
    body 1"""
    a[0, 7] = 0.0
    a[-1, 0:2] = a[1, 0:2]
    a[-1, 7] = 0.0


def _tiny_radius(a, m, _):
    """the last row sits on body 1 with a radius whose r * r^2 underflows in fp32 and not in float64"""
    a[-1, 0:2] = a[1, 0:2]
    a[-1, 7] = np.float32(1e-36)


def _pad_seat(a, m, i):
    a[i, 0:2] = np.float32(1e15)
    a[i, 7] = 1.0


def _build():
    cases = []
    for rn, row in CONTAIN_ROWS.items():
        for vn, plant in CONTAIN_VALUES.items():
            first = rn == "first-massless"
            cases.append(Case(f"contain-{rn}-{vn}", "contain", plant, row,
                              (lambda n, m: m < n - 1) if first else (lambda n, m: m < n)))
    # where a sharded launch seats its inert pad sources (include/nbody_hip.h): a finite receiver exactly there
    cases.append(Case("contain-last-pad-seat", "contain", _pad_seat, CONTAIN_ROWS["last"], lambda n, m: m < n))
    for rn, row in SOURCE_ROWS.items():
        for vn, plant in SOURCE_VALUES.items():
            # M - 1 is its own case only where it is none of the fixed indices
            fits = {"0": lambda n, m: m >= 1, "255": lambda n, m: m >= 256, "256": lambda n, m: m >= 257,
                    "M-1": lambda n, m: m >= 2 and m - 1 not in (255, 256)}[rn]
            cases.append(Case(f"source-{rn}-{vn}", "source", plant, row, fits))
    cases.append(Case("near-overflow", "world", _near_overflow, fits=lambda n, m: m >= 2 and n >= 16))
    cases.append(Case("denormal-radii", "world", _denormal_radii, fits=lambda n, m: m >= 1))
    cases.append(Case("zero-radius-coincidence", "world", _zero_radius, fits=lambda n, m: m >= 2 and n >= 3))
    cases.append(Case("tiny-radius-coincidence", "world", _tiny_radius, fits=lambda n, m: m >= 2 and n >= 3))
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}


def cases_for(n, m, kinds=("contain", "source", "world")):
    return [c for c in CASES if c.kind in kinds and c.fits(n, m)]


def ordinary_tracer(part, i):
    """the same world with row i an ordinary finite tracer (mass and radius stay)"""
    out = part.copy()
    out[i, 0:4] = (12.5, -7.25, 1.0, -2.0)
    return out


# ---- the step checker ----------------------------------------------------------------------------------------------------------

FLT_MAX, FLT_MIN = float(np.finfo(np.float32).max), float(np.finfo(np.float32).tiny)


def lost_terms(start, m):
    """(n, 2) float64: per receiver and component, the sum of |pair term| over the pairs whose factor G*m / (r * r^2) fp32
    cannot hold: r * r^2 beyond 3.4e38 (the reference's form gives G*m / inf = 0, and so does an r^2 that overflows) or the
    factor below the smallest normal number (G*m * rsq * rsq^2 goes denormal or to 0).  Such a term may come out as anything
    between 0 and its float64 value, in the reference as in the kernels, so acc_bound, which is relative to float64, gets
    exactly these |terms| added.  An ordinary world has no such pair (r * r^2 ~ 1e6, factors ~ 1e-3) and the sum is 0.0."""
    x = start[:, 0:2].astype(np.float64)
    gm = float(np.float32(nb.NB_G)) * start[:m, 6].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dx = x[None, :m, 0] - x[:, None, 0]
        dy = x[None, :m, 1] - x[:, None, 1]
        r2 = dx * dx + dy * dy + start[:, 7].astype(np.float64)[:, None]
        r3 = np.sqrt(r2) * r2
        f = gm[None, :] / r3
        lost = (r3 > FLT_MAX / 2) | (f < 2 * FLT_MIN)
        return np.stack([np.where(lost, np.abs(dx * f), 0.0).sum(axis=1), np.where(lost, np.abs(dy * f), 0.0).sum(axis=1)], axis=1)


def bound_mask(start, m, dt, avx=None):
    """(mask (n, 2), acc64, bound, needed) of one step from `start`.  mask: the components that carry the standing bound --
    the AVX oracle's acc is finite there and so are float64's acc and sum of |terms|; mask.all(axis=1) is the row set.
    bound: gpu_common.acc_bound plus lost_terms.  needed: where the AVX oracle itself is inside `bound` only thanks to
    lost_terms (tests/test_nonfinite_cpu.py pins which components those are)."""
    avx = (ob.step(start, m, dt, 1) if avx is None else avx)[:, 4:6]          # avx: that step, where the caller has it
    acc64, mag = ob.acc_f64(start, m)
    with np.errstate(invalid="ignore"):
        plain = acc_bound(acc64, mag)
        bound = plain + lost_terms(start, m)
        mask = np.isfinite(avx) & np.isfinite(acc64) & np.isfinite(mag)
        needed = mask & ~(np.abs(avx.astype(np.float64) - acc64) <= plain)
    return mask, acc64, bound, needed


def assert_step_matches(got, part, m, dt, steps, prev=None, min_rows=0):
    """`got` = the state `steps` (1 or 2) steps after `part`; `prev` = the state under test one step before `got` (for
    steps = 1 that is `part`).  Classes against the AVX oracle over all `steps` steps; the last step's integrator identities
    and acc bound from `prev`, which the caller has put through this function already."""
    assert steps in (1, 2)
    prev = part if steps == 1 else prev
    assert prev is not None and got.shape == part.shape and got.dtype == np.float32
    want = ob.step(part, m, dt, steps)
    for lo, name in ((0, "pos"), (2, "vel"), (4, "acc")):
        g, w = classes(got[:, lo:lo + 2]), classes(want[:, lo:lo + 2])
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{name} after {steps} step(s): {len(bad)} classes differ from the AVX oracle's, first at " \
                              f"{bad[0].tolist()}: got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"
    assert got[:, 6:8].tobytes() == part[:, 6:8].tobytes(), "mass / radius must pass through untouched"
    with np.errstate(invalid="ignore", over="ignore"):
        v = prev[:, 2:4] + got[:, 4:6] * np.float32(dt)
        p = prev[:, 0:2] + v * np.float32(dt)
    assert np.array_equal(got[:, 2:4], v, equal_nan=True), "velocity is not vel + acc*dt in fp32"
    assert np.array_equal(got[:, 0:2], p, equal_nan=True), "position is not pos + vel*dt in fp32"
    mask, ref, bound, _ = bound_mask(prev, m, dt, avx=want if steps == 1 else None)
    rows = int(mask.all(axis=1).sum())
    assert rows >= min_rows, f"only {rows} rows carry the acc bound, {min_rows} must"
    with np.errstate(invalid="ignore"):
        err = np.abs(got[:, 4:6].astype(np.float64) - ref)
    # a component under the mask is finite in the oracle; got has the oracle's classes only if prev is the oracle's state
    # class for class, so ask again here: a non-finite got fails the comparison
    ok = err[mask] <= bound[mask]
    assert np.all(ok), f"{int((~ok).sum())} of {int(mask.sum())} finite acc components outside acc_bound after {steps} step(s)"
    return rows


# ---- diagnostics ---------------------------------------------------------------------------------------------------------------

ENERGY_FIELDS = ("kinetic", "potential", "mass", "momentum", "angular_momentum", "center_of_mass")


def energy_vector(e):
    """an energy dict -> its eight doubles in WorldEnergy order"""
    flat = []
    for k in ENERGY_FIELDS:
        v = e[k]
        flat += list(v) if isinstance(v, tuple) else [v]
    return np.array(flat, dtype=np.float64)


def diag_world(m, extra=40, seed=0):
    """m massive rows then `extra` massless ones, extent 100: partitioned as built"""
    rng = np.random.default_rng(500 + seed)
    a = np.zeros((m + extra, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((m + extra, 2)) * 100.0
    a[:, 2:4] = rng.standard_normal((m + extra, 2)) * 10
    a[:, 7] = 0.5 + rng.random(m + extra)
    a[:m, 6] = 10.0 + 990.0 * rng.random(m)
    return a


DIAG_M = (181, 256, 300)          # dead lanes in the second tile, none, dead lanes in the third tile
DIAG_VALUES = {
    "vel-inf": _set(slice(2, 3), INF),
    "vel-nan": _set(slice(2, 4), QNAN),
    "x-inf": _set(slice(0, 1), INF),
    "pos-nan": _set(slice(0, 2), QNAN),
}


def diag_rows(m):
    return {"0": 0, "M-1": m - 1, "mid": m // 2 + 3}


def diag_plants(m, extra=40):
    """(clean world, [(name, row, planted world)]) of the M-source diagnostics world: every value on every row, then the
    massless tracer"""
    base = diag_world(m, extra, seed=m)
    out = []
    for rn, i in diag_rows(m).items():
        for vn, plant in DIAG_VALUES.items():
            a = base.copy()
            plant(a, m, i)
            out.append((f"{rn}-{vn}", i, a))
    a = base.copy()
    a[m + 7, 0:2] = QNAN
    out.append(("massless-pos-nan", m + 7, a))
    return base, out


def assert_diag_matches(e, phi, want_e, want_phi, part, m, rel_u=1e-5, rel_phi=1e-5):
    """Every field of the energy dict `e` and every Phi_i has the class the host path gives (want_e, want_phi); the finite
    fields sit within energy_ref.assert_energy_close's bounds (rel_u on the potential, as tests/test_gpu_energy.py
    check_world), the finite Phi_i within rel_phi."""
    ge, we = energy_vector(e), energy_vector(want_e)
    bad = np.flatnonzero(classes(ge) != classes(we))
    assert bad.size == 0, f"energy fields {bad.tolist()} have classes {classes(ge)[bad].tolist()}, the host path " \
                          f"{classes(we)[bad].tolist()}: {e} / {want_e}"
    if phi is not None:          # None: a trace row has no Phi_i
        gp, wp = classes(phi), classes(want_phi)
        bad = np.flatnonzero(gp != wp)
        assert bad.size == 0, f"{bad.size} Phi_i differ in class from the host path, first at {int(bad[0])}"
        ok = wp == FINITE
        err = np.abs(phi[ok].astype(np.float64) - want_phi[ok].astype(np.float64))
        assert np.all(err <= rel_phi * np.abs(want_phi[ok].astype(np.float64)) + 1e-300), "finite Phi_i outside rel_phi"
    # the finite fields: the scales come from the rows whose terms are finite (a non-finite row makes its field
    # non-finite, and that field is compared by class above)
    with np.errstate(invalid="ignore", over="ignore"):
        _, scale = energy_f64(part, m, np.zeros(m))
    fin = dict(e), dict(want_e)
    for k in ENERGY_FIELDS:
        gv, wv = np.atleast_1d(np.array(e[k], dtype=np.float64)), np.atleast_1d(np.array(want_e[k], dtype=np.float64))
        if k == "center_of_mass":      # not one of assert_energy_close's fields: 1e-12 of sum |m x| / mass, like the others
            f = part[:m].astype(np.float64)
            with np.errstate(invalid="ignore", over="ignore"):
                sc = np.abs(f[:, 6:7] * f[:, 0:2]).sum(axis=0) / f[:, 6].sum()
            okc = np.isfinite(wv) & np.isfinite(sc)
            assert np.all(np.abs(gv[okc] - wv[okc]) <= 1e-12 * sc[okc] + 1e-300), (k, e[k], want_e[k])
            continue
        if not np.all(np.isfinite(wv)) or (k in scale and not np.all(np.isfinite(np.atleast_1d(scale[k])))):
            # keep assert_energy_close away from inf - inf: the finite components of a tuple are compared here
            okc = np.isfinite(wv)
            sc = np.atleast_1d(np.array(scale.get(k, np.abs(wv)), dtype=np.float64))
            okc &= np.isfinite(sc)
            assert np.all(np.abs(gv[okc] - wv[okc]) <= 1e-12 * sc[okc] + 1e-300), (k, e[k], want_e[k])
            for d in fin:
                d[k] = (0.0, 0.0) if isinstance(e[k], tuple) else 0.0
            if k in scale:
                scale[k] = (1.0, 1.0) if isinstance(scale[k], tuple) else 1.0
    assert_energy_close(fin[0], fin[1], scale, rel_u=rel_u)
