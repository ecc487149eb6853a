"""The pair term (TEST INFRASTRUCTURE, no GPU needed to import): the case table, the domain, the float64 reference, the bound of
DESIGN.md section 5 "The pair term", numpy float32 models of the two statements and of defective ones, and the worlds that put
one pair in front of every copy of the statements.

The statements (nbody_amd/csrc/interaction_asm.h, diag_common.h), one float32 rounding per line:
    dx = sx - px;  dy = sy - py;  q = fma(dx, dx, r);  q = fma(dy, dy, q);  s = rsq(q)
    force:  u = gm * s;  t = s * s;  u = u * t;  ax = fma(dx, u, ax);  ay = fma(dy, u, ay)
    Phi:    phi = fma(gm, s, phi)            (Phi_i = -phi)
The reference is float64 from the same float32 inputs: term = d * gm * q^-1.5, phi_term = gm / sqrt(q), q = dx^2 + dy^2 + r.

The bound, in units of u = 2^-24 relative to the float64 term: 17 u for a force component, 5 u for Phi, plus 2^-12 u for what
first order leaves out (the derivation: DESIGN.md).  Nothing here is taken from a device run.

A world holds ONE live source (or two live massive particles) among padding sources whose terms are exact zeros: they sit at
(2^80, 2^80), so q overflows to +inf, rsq(+inf) = +0, u = gm * 0 = 0 and the term is d * 0 with a finite d -- for any mass, with
no denormal involved.  A result is then the pair's term itself: 0 + t = t in every partial sum, every block close, every join.

tests/test_pair_cpu.py holds the models against the bound, the defective ones against the checker, and the domain counts;
tests/test_gpu_pairs.py runs the table through every route."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24                     # one float32 rounding, relative
TINY = F32(2.0 ** -126)            # the smallest normal float32

# ---- the bound (DESIGN.md section 5 "The pair term") ----------------------------------------------------------------------------
RSQ_ULPS = 1                       # v_rsq_f32 as kernels.hip and SURVEY.md state it: 1 ulp, rho <= 2 u
REL_Q = 2 + 2                      # dx, dy enter squared (u each, doubled, weighted by their share of q: <= 2 u) + two fma roundings
REL_S = 2 * RSQ_ULPS + REL_Q / 2   # rho + rel(q) / 2 = 4 u
FORCE_U = 3 * REL_S + 3 + 1 + 1    # s cubed, three multiplies, the d factor, the accumulating fma onto 0: 17 u
PHI_U = REL_S + 1                  # s once, the accumulating fma onto 0: 5 u
SECOND_ORDER_U = 2.0 ** -12        # pairs of first-order terms (< 17^2 u^2 = 1.8e-5 u), the curvature of q^-1.5 (< 2 (4u)^2), the
#                                    float64 reference's own roundings (8 * 2^-53 = 2^-26 u): together under 2^-15 u; 2^-12 u stated
FORCE_BOUND_U = FORCE_U + SECOND_ORDER_U
PHI_BOUND_U = PHI_U + SECOND_ORDER_U
assert (FORCE_U, PHI_U) == (17, 5)


# ---- float32 arithmetic, one rounding per operation ------------------------------------------------------------------------------

def f32(x):
    return np.asarray(x, dtype=F32)


def fma32(a, b, c):
    """a * b + c rounded to float32.  The float64 product of two float32 is exact; the float64 sum rounds at 2^-53 before the
    float32 rounding, which moves the result from a true fma's in about one case in 2^29 and by at most one ulp's tie."""
    return (f32(a).astype(F64) * f32(b).astype(F64) + f32(c).astype(F64)).astype(F32)


def shift_ulps(s, ulps):
    """s moved by `ulps` float32 steps (s positive, normal and finite wherever it is moved)"""
    s = f32(s)
    if not ulps:
        return s
    ok = np.isfinite(s) & (s >= TINY)
    moved = (s.view(np.int32) + np.int32(ulps)).view(F32)
    return np.where(ok, moved, s)


def rsq32(q, ulps=0, rel=0.0):
    """1 / sqrt(q) rounded to float32 (through float64: within 1/2 + 2^-29 ulp), then `ulps` steps or a relative error on top"""
    with np.errstate(all="ignore"):
        s = (1.0 / np.sqrt(f32(q).astype(F64)) * (1.0 + rel)).astype(F32)
    return shift_ulps(s, ulps)


DEFECTS = ("softening dropped", "radius squared", "radius of receiver i ^ 1", "radius of receiver i ^ 64",
           "rsq 2^-20 off", "one factor s short", "dy used for dx")
PHI_DEFECTS = tuple(d for d in DEFECTS if d != "one factor s short")       # the Phi statement has no such product


def head(sx, sy, px, py, r, rsq_ulps=0, defect=None):
    """dx, dy, q, s of both statements; `defect` names one of DEFECTS"""
    sx, sy, px, py, r = (np.atleast_1d(f32(v)) for v in (sx, sy, px, py, r))
    r = np.broadcast_to(r, np.broadcast(px, r).shape)
    if defect == "softening dropped":
        r = np.zeros_like(r)
    elif defect == "radius squared":
        with np.errstate(all="ignore"):
            r = r * r
    elif defect in ("radius of receiver i ^ 1", "radius of receiver i ^ 64"):
        i = np.arange(r.shape[0]) ^ (1 if defect.endswith("^ 1") else 64)     # the lane's neighbour / the other half of a K = 2 lane
        r = r[np.where(i < r.shape[0], i, np.arange(r.shape[0]))]
    with np.errstate(all="ignore"):
        dx, dy = f32(sx - px), f32(sy - py)
        if defect == "dy used for dx":
            dx = np.broadcast_to(dy, np.broadcast(dx, dy).shape)
        q = fma32(dy, dy, fma32(dx, dx, r))
        s = rsq32(q, rsq_ulps, 2.0 ** -20 if defect == "rsq 2^-20 off" else 0.0)
    return dx, dy, q, s


def force_model(sx, sy, gm, px, py, r, rsq_ulps=0, defect=None, parts=False):
    """(ax, ay) float32 of the ten-instruction statement onto a = 0"""
    dx, dy, q, s = head(sx, sy, px, py, r, rsq_ulps, defect)
    gm = f32(gm)
    with np.errstate(all="ignore"):
        gs = f32(gm * s)
        t = f32(s * s)
        u = f32(gs * s) if defect == "one factor s short" else f32(gs * t)
        ax, ay = fma32(dx, u, 0.0), fma32(dy, u, 0.0)
    return (ax, ay, dict(dx=dx, dy=dy, q=q, s=s, gs=gs, t=t, u=u)) if parts else (ax, ay)


def phi_model(sx, sy, gm, px, py, r, rsq_ulps=0, defect=None):
    """Phi float32 of the six-instruction statement onto phi = 0 (sign: include/nbody_diag.h, Phi = -sum)"""
    _, _, _, s = head(sx, sy, px, py, r, rsq_ulps, defect)
    with np.errstate(all="ignore"):
        return -fma32(f32(gm), s, 0.0)


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------

def reference(sx, sy, gm, px, py, r):
    """(ax, ay, Phi) float64 from the float32 inputs"""
    sx, sy, gm, px, py, r = (np.atleast_1d(f32(v)).astype(F64) for v in (sx, sy, gm, px, py, r))
    with np.errstate(all="ignore"):
        dx, dy = sx - px, sy - py
        q = dx * dx + dy * dy + r
        f = gm * q ** -1.5
        return dx * f, dy * f, -gm / np.sqrt(q)


def reference_exact(sx, sy, gm, px, py, r, digits=60):
    """the same three numbers for ONE pair from exact rational dx, dy, q and a `digits`-digit square root: Decimals"""
    sx, sy, gm, px, py, r = (Fraction(float(F32(v))) for v in (sx, sy, gm, px, py, r))
    dx, dy = sx - px, sy - py
    q = dx * dx + dy * dy + r
    with localcontext() as ctx:
        ctx.prec = digits
        ctx.Emax, ctx.Emin = 10 ** 6, -10 ** 6

        def dec(x):
            return Decimal(x.numerator) / Decimal(x.denominator)
        root = dec(q).sqrt()
        f = dec(gm) / (dec(q) * root)
        return dec(dx) * f, dec(dy) * f, -dec(gm) / root


# ---- the checker -----------------------------------------------------------------------------------------------------------------

def errors_u(got, want):
    """|got - want| / |want| in units of u, per element; 0 where both are exactly zero, inf for a wrong zero, sign or class"""
    got, want = np.asarray(got).astype(F64), np.asarray(want, dtype=F64)
    with np.errstate(all="ignore"):
        e = np.abs(got - want) / np.abs(want) / U
    e = np.where(want == 0, np.where(got == 0, 0.0, np.inf), e)
    bad = ~np.isfinite(got) | (np.sign(got) != np.sign(want))
    return np.where(bad, np.inf, e)


def check(label, got, want, bound_u, mask=None, what="force", quiet=False):
    """Every element of `got` (float32) within bound_u * u of the float64 `want`, an exact zero where want is zero, the same
    sign.  `mask` selects the rows in the domain.  Prints one line (pytest -rP) unless quiet, returns the worst error in u."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == F32 and got.shape == want.shape, (label, got.dtype, got.shape, want.shape)
    if mask is not None:
        got, want = got[mask], want[mask]
    e = errors_u(got, want)
    worst = float(e.max()) if e.size else 0.0
    if not quiet:
        print(f"[pair] {label} | {what} | {e.shape[0]} cases | worst {worst:.2f} u | bound {bound_u:g} u")
    assert e.size > 0, f"{label}: no case"
    if not worst <= bound_u:
        at = np.argwhere(~(e <= bound_u))
        first = tuple(int(v) for v in at[0])
        raise AssertionError(f"{label}: {what}: {at.shape[0]} of {e.size} values outside {bound_u:g} u; worst {worst:.2f} u; first at "
                             f"{first}: got {got[first]!r} want {want[first]!r}")
    return worst


def check_force(label, acc, want_xy, mask=None, quiet=False):
    return check(label, acc, want_xy, FORCE_BOUND_U, mask, "force", quiet)


def check_phi(label, phi, want, mask=None, quiet=False):
    return check(label, phi, want, PHI_BOUND_U, mask, "Phi", quiet)


# ---- the domain ------------------------------------------------------------------------------------------------------------------

def _normal(x):
    return np.isfinite(x) & (np.abs(x) >= TINY)


def _normal_or_zero(x):
    return np.isfinite(x) & ((x == 0) | (np.abs(x) >= TINY))


def in_domain(sx, sy, gm, px, py, r):
    """True where every float32 intermediate of both statements is normal and finite (an exactly zero dx or dy, and the zero
    product it gives, is allowed; both zero is no pair) with rsq correctly rounded and one ulp either side.  Looks at the inputs
    and the model only.  Outside lies what include/nbody_hip.h "Non-finite state" sets apart: overflow, underflow, and a
    denormal q, which v_rsq_f32 flushes."""
    ok = None
    for ulps in (-RSQ_ULPS, 0, RSQ_ULPS):
        ax, ay, p = force_model(sx, sy, gm, px, py, r, ulps, parts=True)
        good = _normal_or_zero(p["dx"]) & _normal_or_zero(p["dy"]) & ((p["dx"] != 0) | (p["dy"] != 0))
        for k in ("q", "s", "gs", "t", "u"):
            good &= _normal(p[k])
        good &= _normal_or_zero(ax) & _normal_or_zero(ay) & ((ax == 0) == (p["dx"] == 0)) & ((ay == 0) == (p["dy"] == 0))
        ok = good if ok is None else ok & good
    r = np.broadcast_to(f32(r), ok.shape)
    return ok & _normal_or_zero(r) & (r >= 0) & bool(_normal(F32(gm)))


# ---- the range table ---------------------------------------------------------------------------------------------------------------

EXPONENTS = tuple(range(-40, 41, 4))
SKEW = 2.0 ** -12
DIRECTIONS = (("x", (-1.0, 0.0)), ("y", (0.0, 1.0)), ("diagonal", (1.0, -1.0)), ("skew x", (-1.0, SKEW)), ("skew y", (SKEW, 1.0)))
RATIOS = (0.0, 2.0 ** -30, 2.0 ** -12, 1.0, 2.0 ** 12, 2.0 ** 30)      # radius / 2^(2e): the radius is a power of two or zero
FIXED_MANTISSAS = (1.0, 1.5, 2.0 - 2.0 ** -23)
RANDOM_MANTISSAS = 1                                                   # per (exponent, direction) cell, seeded
MANTISSAS = len(FIXED_MANTISSAS) + RANDOM_MANTISSAS
ROWS = len(EXPONENTS) * len(DIRECTIONS) * MANTISSAS * len(RATIOS)      # 2 520; the ratio runs fastest: neighbours differ in radius
SOURCES = {"near": (0.0, 0.0),                  # the tracer is the offset itself: sx - px is exact
           "far": (30000.123, -29999.877)}      # the tracer is fl(source + offset): sx - px rounds once the offset passes the source
GM_TARGETS = tuple(m * 2.0 ** e for e in (-40, 0, 40) for m in (1.0, 1.3125, 1.96875))
NB_G = 10.0                                     # include/nbody.h; tests/test_pair_cpu.py holds it to nbody_amd.NB_G


def source_mass(gi):
    """(mass, gm): the float32 mass whose float32 product with NB_G is the G*m of world gi (convert.hip g_times_m)"""
    mass = F32(GM_TARGETS[gi] / NB_G)
    return mass, F32(mass * F32(NB_G))


def _table():
    rng = np.random.default_rng(15)
    cell = np.zeros((ROWS, 4), dtype=np.int64)          # exponent, direction, ratio, mantissa index of every row
    off = np.zeros((ROWS, 2), dtype=F32)
    rad = np.zeros(ROWS, dtype=F32)
    i = 0
    for ei, e in enumerate(EXPONENTS):
        for di, (_, (ux, uy)) in enumerate(DIRECTIONS):
            mants = FIXED_MANTISSAS + tuple(1.0 + int(k) * 2.0 ** -23 for k in rng.integers(1, 2 ** 23 - 1, RANDOM_MANTISSAS))
            for mi, mant in enumerate(mants):
                for ri, ratio in enumerate(RATIOS):
                    cell[i] = ei, di, ri, mi
                    off[i] = F32(ux * mant * 2.0 ** e), F32(uy * mant * 2.0 ** e)
                    rad[i] = F32(ratio * 2.0 ** (2 * e))
                    i += 1
    assert i == ROWS
    return cell, off, rad


CELL, OFFSET, RADIUS = _table()
CELL, MANTISSA = CELL[:, :3], CELL[:, 3]
DOMAIN_COUNT = 32146     # cases in the domain over the 18 worlds below (of 18 * 2 520): a constant, asserted by tests/test_pair_cpu.py
#                          from the filter and by tests/test_gpu_pairs.py from what each route checked -- no case can drop out unseen
# the rows whose dx, dy and q are exact beside the near source (mantissa 1.0 on an axis, the radius within 2^23 of d^2): the Phi
# statement's error there is rho + u and nothing else, which isolates v_rsq_f32
EXACT_HEAD = (MANTISSA == 0) & (CELL[:, 1] <= 1) & np.isin(CELL[:, 2], (0, 2, 3, 4))
WORLDS = tuple((kind, gi) for kind in SOURCES for gi in range(len(GM_TARGETS)))      # 18: one per source position and G*m


def tracers(kind):
    """(px, py) float32 of the table's tracers beside the source of this kind"""
    s = f32(SOURCES[kind])
    return f32(s[0] + OFFSET[:, 0]), f32(s[1] + OFFSET[:, 1])


_EXPECTED = {}


def expected(kind, gi):
    """dict(mask, acc (ROWS, 2) float64, phi (ROWS,) float64) of world (kind, gi); computed once, never changed"""
    if (kind, gi) not in _EXPECTED:
        s, (px, py), gm = f32(SOURCES[kind]), tracers(kind), source_mass(gi)[1]
        ax, ay, phi = reference(s[0], s[1], gm, px, py, RADIUS)
        e = dict(mask=in_domain(s[0], s[1], gm, px, py, RADIUS), acc=np.stack([ax, ay], axis=1), phi=phi)
        for v in e.values():
            v.setflags(write=False)
        _EXPECTED[kind, gi] = e
    return _EXPECTED[kind, gi]


# ---- worlds ------------------------------------------------------------------------------------------------------------------------

PAD_AT = 2.0 ** 80
PAD_MASS = 3.0
LIVE_RADIUS = 1.0        # of a live source in a tracer world: its own term is 0 * gm * rsq(1)^3 = 0
RANGE_M, RANGE_J = 130, 77     # the range worlds: three 64-source chunks (two passes, three parts, 16 slices are real), live at 77


def padded_sources(m, live):
    """(m, 8) sources: padding everywhere but the rows of `live` = {index: (x, y, mass, radius)}"""
    a = np.zeros((m, 8), dtype=F32)
    a[:, 0:2] = PAD_AT
    a[:, 6] = PAD_MASS
    a[:, 7] = 1.0
    for j, (x, y, mass, radius) in live.items():
        a[j, 0], a[j, 1], a[j, 6], a[j, 7] = x, y, mass, radius
    assert np.all(a[:, 6] > 0)
    return a


def tracer_rows(px, py, r):
    t = np.zeros((len(px), 8), dtype=F32)
    t[:, 0], t[:, 1], t[:, 7] = px, py, r
    return t


def range_world(kind, gi, m=RANGE_M, j=RANGE_J, rows=slice(None)):
    """the live source of (kind, gi) at index j of m sources, then the table's tracers `rows`: partitioned as built"""
    s, (px, py) = f32(SOURCES[kind]), tracers(kind)
    src = padded_sources(m, {j: (s[0], s[1], source_mass(gi)[0], LIVE_RADIUS)})
    return np.concatenate([src, tracer_rows(px[rows], py[rows], RADIUS[rows])])


def padding_world(m, kind="far"):
    """padding sources only, and the table's tracers: every acc and every Phi of a tracer must be an exact zero"""
    px, py = tracers(kind)
    return np.concatenate([padded_sources(m, {}), tracer_rows(px, py, RADIUS)])


# ---- the slot worlds ---------------------------------------------------------------------------------------------------------------

SLOT_TRACERS = 200        # one full 128-receiver tile of K = 2 / W = 16 and a ragged second one
SLOT_TRACERS_LONG = 560   # for ensembles: with 19 sources 579 particles, past the 512 of the one-workgroup path
SLOT_SOURCE = (0.375, -0.625)
SLOT_MASS = 1.2
SLOT_COUNTS = {19: tuple(range(19)), 300: (0, 7, 8, 63, 64, 127, 128, 255, 256, 299)}


def _slot_tracers():
    rng = np.random.default_rng(1515)
    n = SLOT_TRACERS_LONG
    d = (1.0 + rng.random(n)) * 2.0 ** rng.integers(-3, 11, n)
    ang = rng.random(n) * 2 * math.pi
    px = f32(SLOT_SOURCE[0] + d * np.cos(ang))
    py = f32(SLOT_SOURCE[1] + d * np.sin(ang))
    r = f32(d * d * (1.0 + rng.random(n)) * 2.0 ** rng.integers(-12, 5, n))
    return px, py, r


SLOT_PX, SLOT_PY, SLOT_R = _slot_tracers()


def slot_world(m, j, tracers=SLOT_TRACERS):
    src = padded_sources(m, {j: (SLOT_SOURCE[0], SLOT_SOURCE[1], SLOT_MASS, LIVE_RADIUS)})
    return np.concatenate([src, tracer_rows(SLOT_PX[:tracers], SLOT_PY[:tracers], SLOT_R[:tracers])])


def slot_expected(tracers=SLOT_TRACERS):
    """(mask, acc float64 (tracers, 2), phi float64)"""
    gm = F32(F32(SLOT_MASS) * F32(NB_G))
    args = (F32(SLOT_SOURCE[0]), F32(SLOT_SOURCE[1]), gm, SLOT_PX[:tracers], SLOT_PY[:tracers], SLOT_R[:tracers])
    ax, ay, phi = reference(*args)
    return in_domain(*args), np.stack([ax, ay], axis=1), phi


# ---- massive receivers -------------------------------------------------------------------------------------------------------------

PAIR_M = 300
PAIR_PLACES = {"same block": (0, 1), "other block": (0, 299)}     # by step_kernel's 256-source blocks and by the diagnostics' 128-receiver tiles
PAIR_EXPONENTS = (-24, -8, 0, 12, 28)
PAIR_DIRECTIONS = (0, 2, 3)
PAIR_RADII = ((2.0 ** -12, 1.0), (2.0 ** 12, 1.5 * 2.0 ** -12))   # (radius of A, of B) / 2^(2e)
PAIR_MANTISSAS = (1.0, 1.0 + 2.0 ** -23 * 3141593)


def pair_cases():
    """Two live massive particles: A at the origin, B at the offset.  Each case: dict(a=(x, y, mass, radius), b=..., want), want
    = float64 (acc of A, Phi of A, acc of B, Phi of B).  The masses follow the separation so that both terms, and the particles'
    own terms 0 * gm * rsq(radius)^3, stay in the domain."""
    out = []
    for e in PAIR_EXPONENTS:
        for n, di in enumerate(PAIR_DIRECTIONS):
            ux, uy = DIRECTIONS[di][1]
            for (ra, rb), mant in zip(PAIR_RADII, PAIR_MANTISSAS):
                ma, mb = F32(1.25 * 2.0 ** e / NB_G), F32(1.75 * 2.0 ** (e + n) / NB_G)
                a = (F32(0), F32(0), ma, F32(ra * 2.0 ** (2 * e)))
                b = (F32(ux * mant * 2.0 ** e), F32(uy * mant * 2.0 ** e), mb, F32(rb * 2.0 ** (2 * e)))
                gma, gmb = F32(ma * F32(NB_G)), F32(mb * F32(NB_G))
                on_a = (b[0], b[1], gmb, a[0], a[1], a[3])          # source B, receiver A with A's radius
                on_b = (a[0], a[1], gma, b[0], b[1], b[3])
                own = all(bool(_normal(rsq32(p[3]))) and bool(_normal(f32(F32(g) * rsq32(p[3]) * rsq32(p[3]) * rsq32(p[3]))))
                          for p, g in ((a, gma), (b, gmb)))
                ok = bool(in_domain(*on_a)[0]) and bool(in_domain(*on_b)[0]) and own
                wa, wb = reference(*on_a), reference(*on_b)
                out.append(dict(e=e, direction=DIRECTIONS[di][0], a=a, b=b, ok=ok,
                                want_a=(np.array([wa[0][0], wa[1][0]]), wa[2][0]), want_b=(np.array([wb[0][0], wb[1][0]]), wb[2][0])))
    return out


def pair_world(case, place):
    ia, ib = PAIR_PLACES[place]
    return padded_sources(PAIR_M, {ia: case["a"], ib: case["b"]})
