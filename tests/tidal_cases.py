"""The pair term of the tidal tensor (TEST INFRASTRUCTURE, no GPU needed to import): the case tables, the domain, the float64
reference per part, the bound of DESIGN.md section 5 "The tidal pair term", the checker, and the worlds that put one pair in
front of every kernel of nbody_amd/csrc/tidal.hip.  The float32 model of the statement and the defective ones are
tidal_ref.statement / pair_model / PAIR_DEFECTS; float32 arithmetic, the case table and the padding sources are pair_cases'.

The statement (nbody_amd/csrc/field_kernels.h, policy Tidal), one float32 rounding per line, onto sums of +0:
    dx = sx - px;  dy = sy - py;  q = fma(dy, dy, fma(dx, dx, s));  u = rsq(q);  u2 = u * u
    w = (g * u) * u2;  D = 0 + w;  w5 = w * u2;  tx = dx * w5;  ty = dy * w5
    A = fma(dx, tx, 0);  B = fma(dx, ty, 0);  C = fma(dy, ty, 0)
then in float64 xx = 3 A - D, xy = 3 B, yy = 3 C - D, each rounded once to float32.

The reference is float64 per PART from the same float32 inputs: a = dx^2 g u^5, b = dx dy g u^5, c = dy^2 g u^5, d = g u^3
with u = (dx^2 + dy^2 + s)^(-1/2); xx = 3 a - d, xy = 3 b, yy = 3 c - d.

The bound, first order, in u = 2^-24 relative per rounding, with pair_cases' REL_S = 4 u for u = rsq(q):
    d   3 REL_S (u enters cubed) + 3 (g * u, u * u, their product); the add onto +0 is exact                       15 u
    a   5 REL_S (u^5) + 5 (g * u, u * u entering twice, w, w5) + 1 (tx) + 2 (the rounded dx, entering twice) + 1 (fmac)  29 u
    b   the same with ty, and one rounded dx and one rounded dy                                                    29 u
    c   the same with dy twice                                                                                     29 u
    |xx - xx64| <= (3 A_U |a| + D_U |d| + |xx64|) u: the parts' budgets and the final rounding (half an ulp <= u |result|);
    |xy - xy64| <= (3 B_U |b| + |xy64|) u;  yy like xx.  SECOND_ORDER_U is added to every budget.
The bound is in the parts, so it stays tight where 3 a is close to d.  xy is +0 wherever dx or dy is an exact zero; a
component has its reference's sign wherever that exceeds the bound.  Nothing here is taken from a device run."""
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np

import nbody_amd as nb
import pair_cases as pc
import tidal_ref as tr
from pair_cases import F32, F64, TINY, U, f32

# ---- the bound ---------------------------------------------------------------------------------------------------------------------
D_U = 3 * pc.REL_S + 3                     # 15
A_U = 5 * pc.REL_S + 5 + 1 + 2 + 1         # 29
B_U = A_U                                  # ty for tx, one dx and one dy for two dx: the same count
C_U = A_U
FINAL_U = 1                                # the one float64 -> float32 rounding of a component: half an ulp <= u |component|
# pairs of first-order terms (< 29^2 u^2 = 5.0e-5 u), the curvature of q^-2.5 (< 4.4 (4u)^2 = 4.2e-6 u), the final rounding taken
# at the reference instead of at the device's float64 value (< 29 u^2 per part = 1.7e-6 u), the reference's own roundings
# (12 * 2^-53 < 2^-25 u): together under 2^-14 u; 2^-12 u stated, as for the force
SECOND_ORDER_U = 2.0 ** -12
assert (A_U, B_U, C_U, D_U) == (29, 29, 29, 15)
PART_FLOOR = 2.0 ** -100                   # see in_domain


# ---- the float64 reference -----------------------------------------------------------------------------------------------------------

def reference(sx, sy, gm, px, py, s):
    """the parts (a, b, c, d) float64 from the float32 inputs"""
    sx, sy, gm, px, py, s = (np.atleast_1d(f32(v)).astype(F64) for v in (sx, sy, gm, px, py, s))
    with np.errstate(all="ignore"):
        dx, dy = sx - px, sy - py
        q = dx * dx + dy * dy + s
        d = gm / (q * np.sqrt(q))
        w5 = d / q
        a, b, c, d = np.broadcast_arrays(dx * dx * w5, dx * dy * w5, dy * dy * w5, d)
    return a, b, c, d


def reference_exact(sx, sy, gm, px, py, s, digits=60):
    """the same four numbers for ONE pair from exact rational dx, dy, q and a `digits`-digit square root: Decimals"""
    sx, sy, gm, px, py, s = (Fraction(float(F32(v))) for v in (sx, sy, gm, px, py, s))
    dx, dy = sx - px, sy - py
    q = dx * dx + dy * dy + s
    with localcontext() as ctx:
        ctx.prec = digits
        ctx.Emax, ctx.Emin = 10 ** 6, -10 ** 6

        def dec(x):
            return Decimal(x.numerator) / Decimal(x.denominator)
        d = dec(gm) / (dec(q) * dec(q).sqrt())
        w5 = d / dec(q)
        return dec(dx * dx) * w5, dec(dx * dy) * w5, dec(dy * dy) * w5, d


def tensor(parts):
    """(n, 3) float64 (xx, xy, yy) of the parts"""
    a, b, c, d = parts
    return np.stack([3.0 * a - d, 3.0 * b, 3.0 * c - d], axis=1)


def bounds(parts, extra_u=SECOND_ORDER_U):
    """(n, 3) float64: the allowed |T - T64| per component"""
    a, b, c, d = (np.abs(v) for v in parts)
    t = np.abs(tensor(parts))
    return np.stack([3 * (A_U + extra_u) * a + (D_U + extra_u) * d + FINAL_U * t[:, 0],
                     3 * (B_U + extra_u) * b + FINAL_U * t[:, 1],
                     3 * (C_U + extra_u) * c + (D_U + extra_u) * d + FINAL_U * t[:, 2]], axis=1) * U


# ---- the checker -----------------------------------------------------------------------------------------------------------------------

def check(label, got, parts, mask=None, quiet=False):
    """Every row of `got` (n, 3) float32 inside bounds(parts) of tensor(parts); xy the bits of +0 where b is an exact zero; the
    reference's sign wherever it exceeds the bound; finite.  Returns (worst error in u of the component's parts, i.e. of
    3|a| + |d| or 3|b|; worst error / bound); prints one line (pytest -rP) unless quiet."""
    got = np.asarray(got)
    parts = tuple(np.asarray(v, dtype=F64) for v in parts)
    assert got.dtype == F32 and got.shape == (parts[0].shape[0], 3), (label, got.dtype, got.shape, parts[0].shape)
    if mask is not None:
        got, parts = got[mask], tuple(v[mask] for v in parts)
    assert got.shape[0] > 0, f"{label}: no case"
    want, bound = tensor(parts), bounds(parts)
    a, b, c, d = (np.abs(v) for v in parts)
    scale = np.stack([3 * a + d, 3 * b, 3 * c + d], axis=1)
    g64 = got.astype(F64)
    with np.errstate(all="ignore"):
        err = np.abs(g64 - want)
        in_u = np.where(scale > 0, err / scale / U, np.where(err == 0, 0.0, np.inf))
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    bad = ~np.isfinite(g64) | ~(err <= bound)
    bad |= (np.abs(want) > bound) & (np.sign(g64) != np.sign(want))
    zero_xy = parts[1] == 0
    bad[:, 1] |= zero_xy & (got[:, 1].view(np.uint32) != 0)          # +0, not -0, not a small number
    in_u = np.where(np.isfinite(g64), in_u, np.inf)
    worst_u, worst = float(in_u.max()), float(np.where(bad, np.inf, ratio).max())
    if not quiet:
        print(f"[tidal pair] {label} | {got.shape[0]} cases | worst {worst_u:.2f} u of the parts | worst error / bound {worst:.3f}")
    if bad.any():
        at = np.argwhere(bad)
        first = tuple(int(v) for v in at[0])
        raise AssertionError(f"{label}: {at.shape[0]} of {bad.size} components outside the bound; first at {first}: got "
                             f"{got[first]!r} want {want[first]!r} bound {bound[first]!r}")
    return worst_u, worst


# ---- the domain ------------------------------------------------------------------------------------------------------------------------

def in_domain(sx, sy, gm, px, py, s):
    """pair_cases.in_domain (dx, dy, q, u, g u, u u, w normal; a softening > 0 here) extended by the rest of the statement: u2
    and w5 normal, tx, ty and the three products normal or the exact zero an exactly zero dx or dy gives, with rsq correctly
    rounded and one ulp either side.  And the results: xy is normal or an exact zero; a diagonal component may cancel into
    the denormal range, where a conversion that flushed would lose up to 2^-126, so the domain asks d >= 2^-100: the bound is
    then at least 15 u d > 2^-120 and does not depend on how that conversion treats denormals.  Looks at the inputs and the
    model only."""
    ok = pc.in_domain(sx, sy, gm, px, py, s)
    for ulps in (-pc.RSQ_ULPS, 0, pc.RSQ_ULPS):
        _, p = tr.pair_model(sx, sy, gm, px, py, s, ulps, parts=True)
        zx, zy = np.atleast_1d(p["dx"] == 0), np.atleast_1d(p["dy"] == 0)
        good = pc._normal(p["u2"]) & pc._normal(p["w5"])
        for k, zero in (("tx", zx), ("ty", zy), ("A", zx), ("B", zx | zy), ("C", zy)):
            good = good & pc._normal_or_zero(p[k]) & ((p[k] == 0) == zero)
        ok = ok & np.atleast_1d(good)
    a, b, c, d = reference(sx, sy, gm, px, py, s)
    s = np.broadcast_to(f32(s), ok.shape)
    ok = ok & (s >= TINY) & (d >= PART_FLOOR) & ((b == 0) | (np.abs(3.0 * b) >= 2.0 * float(TINY)))
    return ok & (3.0 * np.maximum(a, c) + d < 2.0 ** 126)


# ---- the range table: probes ---------------------------------------------------------------------------------------------------------------

# pair_cases' table where g u^5 leaves room: |e| <= 24 keeps every (direction, ratio) cell occupied (tests/test_tidal_pair_cpu.py)
E_MAX = 24
EXPONENTS = tuple(e for e in pc.EXPONENTS if abs(e) <= E_MAX)
_KEEP = np.abs(np.asarray(pc.EXPONENTS)[pc.CELL[:, 0]]) <= E_MAX
TABLE_ROWS = int(_KEEP.sum())
# the ratio 0 cannot be asked (one softening > 0 per call): the rows that had it take one softening far below every other one,
# 2^-24 of the smallest -- under half an ulp of every d^2 of the table, so q = d^2 as rounded: "softening negligible"
SOFT_MIN = F32(pc.RADIUS[_KEEP][pc.RADIUS[_KEEP] > 0].min() * 2.0 ** -24)
# rows where xx cancels: s = 2 dx^2 - dy^2 exactly (short mantissas, so s is a float32), i.e. 3 a = d beside the near source
CANCEL_MANTISSAS = (1.0, 1.5, 1.3125)
CANCEL_SHAPES = ((0.0, 2.0), (0.5, 1.75))          # (dy / dx, s / dx^2)


def _table():
    off, rad = [pc.OFFSET[_KEEP]], [np.where(pc.RADIUS[_KEEP] > 0, pc.RADIUS[_KEEP], SOFT_MIN).astype(F32)]
    rows = [(F32(-m * 2.0 ** e), F32(h * m * 2.0 ** e), F32(k * m * m * 2.0 ** (2 * e)))
            for e in EXPONENTS for m in CANCEL_MANTISSAS for h, k in CANCEL_SHAPES]
    off.append(np.asarray([r[:2] for r in rows], dtype=F32))
    rad.append(np.asarray([r[2] for r in rows], dtype=F32))
    return np.concatenate(off), np.concatenate(rad)


OFFSET, RADIUS = _table()
ROWS = OFFSET.shape[0]
CELL = pc.CELL[_KEEP] - np.array([pc.EXPONENTS.index(EXPONENTS[0]), 0, 0])      # (exponent, direction, ratio) of the table rows
CANCEL = np.arange(ROWS) >= TABLE_ROWS
D_ALONE = np.concatenate([pc.CELL[_KEEP][:, 1] == 0, np.zeros(ROWS - TABLE_ROWS, dtype=bool)])     # direction "x": dy = 0, yy = -d
for _v in (OFFSET, RADIUS, CELL, CANCEL, D_ALONE):
    _v.setflags(write=False)
WORLDS = pc.WORLDS
DOMAIN_COUNT = 21082      # cases in the domain over the 18 worlds (of 18 * ROWS): a constant, asserted by tests/test_tidal_pair_cpu.py
#                           from the filter and by tests/test_gpu_tidal_pairs.py from what each route checked
M, J = pc.RANGE_M, pc.RANGE_J


def source(kind, gi):
    """(sx, sy, mass, gm) float32 of world (kind, gi)"""
    s = f32(pc.SOURCES[kind])
    return (s[0], s[1]) + pc.source_mass(gi)


def points(kind):
    """(ROWS, 2) float32: the probes beside the source of this kind"""
    s = f32(pc.SOURCES[kind])
    return np.stack([f32(s[0] + OFFSET[:, 0]), f32(s[1] + OFFSET[:, 1])], axis=1)


def _expected(kind, gi, pts, rad):
    sx, sy, _, gm = source(kind, gi)
    args = (sx, sy, gm, pts[:, 0], pts[:, 1], rad)
    e = dict(mask=in_domain(*args), parts=np.stack(reference(*args)))
    for v in e.values():
        v.setflags(write=False)
    return e


_EXPECTED = {}


def expected(kind, gi):
    """dict(mask (ROWS,), parts (4, ROWS) float64) of world (kind, gi); computed once, never changed"""
    if (kind, gi) not in _EXPECTED:
        _EXPECTED[kind, gi] = _expected(kind, gi, points(kind), RADIUS)
    return _EXPECTED[kind, gi]


def world(kind, gi, m=M, j=J):
    """the live source of (kind, gi) at index j of m sources, the rest padding whose terms are exact zeros; no other particle:
    the probes are the callers' points"""
    sx, sy, mass, _ = source(kind, gi)
    return pc.padded_sources(m, {j: (sx, sy, mass, pc.LIVE_RADIUS)})


# ---- the range table: maps -------------------------------------------------------------------------------------------------------------------
# A map's samples are the pixel centres of a view, a grid: a table row is no pixel centre of a view shared with other rows, so the
# map routes run on the centres themselves as their case table (the rule of test_a_map_is_the_probes_product_at_the_pixel_centres:
# the centres are tidal_ref.pixel_points', bit for bit what the host hands the kernel).  One 8 x 8 view per exponent and zoom
# mantissa, centred so that column 3 and row 3 pass through the source: x of column i is (i - 3) / zoom + sx, every operation
# rounded, so the axes (dx or dy an exact zero), both diagonals and the skew directions between them are all there.

MAP_SIDE = 8
MAP_ZOOMS = (1.0, 1.2345)                       # zoom = fl(2^-e / this): exact offsets k 2^e, and offsets with full mantissas
MAP_RATIOS = tuple(r for r in pc.RATIOS if r > 0)
MAP_VIEWS = tuple((e, z) for e in EXPONENTS for z in MAP_ZOOMS)
MAP_SOFTS = 1 + len(MAP_RATIOS)                 # per view: SOFT_MIN and the ratios
MAP_PIXELS = MAP_SIDE * MAP_SIDE
MAP_ROWS = len(MAP_VIEWS) * MAP_SOFTS * MAP_PIXELS
MAP_DOMAIN_COUNT = 123622  # of 18 * MAP_ROWS, as DOMAIN_COUNT


def map_view(kind, vi):
    e, z = MAP_VIEWS[vi]
    s = f32(pc.SOURCES[kind])
    return nb.RenderView.make((float(s[0]), float(s[1])), (3.5, 3.5), float(F32(2.0 ** -e / z)), MAP_SIDE, MAP_SIDE, 1.0)


def map_softenings(vi):
    e = MAP_VIEWS[vi][0]
    return (SOFT_MIN,) + tuple(F32(r * 2.0 ** (2 * e)) for r in MAP_RATIOS)


def map_rows(vi, si):
    """the rows of view vi under its softening si in the map table"""
    start = (vi * MAP_SOFTS + si) * MAP_PIXELS
    return slice(start, start + MAP_PIXELS)


def map_points(kind, vi):
    """the intended centres of view vi, row-major (64, 2) float32: column i at fl(fl((i - 3) / zoom) + sx) -- (i + 0.5) - 3.5 is
    exact --, rows likewise; column 3 and row 3 are the source's own coordinates.  The GPU tests assert that
    tidal_ref.pixel_points(map_view(kind, vi)) has these bits before they use a map."""
    view, s = map_view(kind, vi), f32(pc.SOURCES[kind])
    k = np.arange(MAP_SIDE, dtype=F32) - F32(3.0)
    xs, ys = f32(f32(k / F32(view.zoom)) + s[0]), f32(f32(k / F32(view.zoom)) + s[1])
    assert xs[3] == s[0] and ys[3] == s[1]
    pts = np.empty((MAP_SIDE, MAP_SIDE, 2), dtype=F32)
    pts[:, :, 0], pts[:, :, 1] = xs[None, :], ys[:, None]
    return pts.reshape(-1, 2)


def map_radius():
    return np.concatenate([np.full(MAP_PIXELS, s, dtype=F32) for vi in range(len(MAP_VIEWS)) for s in map_softenings(vi)])


_MAP_EXPECTED = {}


def map_expected(kind, gi):
    """dict(mask (MAP_ROWS,), parts (4, MAP_ROWS), points (MAP_ROWS, 2)): every view under every one of its softenings"""
    if (kind, gi) not in _MAP_EXPECTED:
        pts = np.concatenate([map_points(kind, vi) for vi in range(len(MAP_VIEWS)) for _ in range(MAP_SOFTS)])
        pts.setflags(write=False)
        _MAP_EXPECTED[kind, gi] = dict(_expected(kind, gi, pts, map_radius()), points=pts)
    return _MAP_EXPECTED[kind, gi]


# ---- the slot worlds -----------------------------------------------------------------------------------------------------------------------

SLOT_SOFT = 0.75
SLOT_COUNTS = {19: pc.SLOT_COUNTS[19], 300: pc.SLOT_COUNTS[300], 2049: pc.SLOT_COUNTS[300] + (2047, 2048)}
SLOT_POINTS = np.stack([pc.SLOT_PX[:pc.SLOT_TRACERS], pc.SLOT_PY[:pc.SLOT_TRACERS]], axis=1)     # one full tile of 128 and a ragged second
SLOT_VIEW = ((pc.SLOT_SOURCE[0], pc.SLOT_SOURCE[1]), (9.25, 5.75), 0.37, 20, 10)                # 200 centres around the source


def slot_view():
    target, offset, zoom, width, height = SLOT_VIEW
    return nb.RenderView.make(target, offset, zoom, width, height, 1.0)


def slot_args(pts):
    return (F32(pc.SLOT_SOURCE[0]), F32(pc.SLOT_SOURCE[1]), F32(F32(pc.SLOT_MASS) * F32(pc.NB_G)), pts[:, 0], pts[:, 1],
            np.full(pts.shape[0], SLOT_SOFT, dtype=F32))


def slot_world(m, j):
    return pc.padded_sources(m, {j: (pc.SLOT_SOURCE[0], pc.SLOT_SOURCE[1], pc.SLOT_MASS, pc.LIVE_RADIUS)})


def neighbour(n, m, seed):
    """an ordinary world for the other members of an ensemble: n particles, m of them massive, partitioned as built"""
    rng = np.random.default_rng(2600 + seed)
    a = np.zeros((n, 8), dtype=F32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * 50.0
    a[:, 7] = 0.5 + rng.random(n)
    a[:m, 6] = 10.0 + 990.0 * rng.random(m)
    return a
