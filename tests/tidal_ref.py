"""float64 restatement of include/nbody_tidal.h in numpy, and a float32 model of the device statement (TEST INFRASTRUCTURE for
test_tidal_cpu.py / test_tidal_pair_cpu.py / test_gpu_tidal.py / test_gpu_batch_tidal.py / test_gpu_tidal_pairs.py /
test_gpu_tidal_sums.py; no GPU needed to import).

Particles are partitioned (mass > 0 first), m = mass_len.  With d_j = x_j - p, q_j = |d_j|^2 + s and u_j = q_j^(-1/2),
    T_ab(p; s) = sum_{j<m} G*m_j (3 d_a d_b u_j^5 - delta_ab u_j^3)          (xx, xy, yy)
with G*m_j the float32 product the step kernels use; no term is excluded.  A point with a non-finite coordinate gives NaN in
all three components.  The points, the pixel centres and the probes are field_ref's.

The model (device_model) restates nbody_amd/csrc/field_kernels.h's Tidal policy and the sampler's summation, one float32
rounding per instruction:
    dx = sx - px;  dy = sy - py;  q = fma(dy, dy, fma(dx, dx, s));  u = rsq(q);  u2 = u * u
    w = (g * u) * u2;  D += w;  w5 = w * u2;  tx = dx * w5;  ty = dy * w5
    A = fma(dx, tx, A);  B = fma(dx, ty, B);  C = fma(dy, ty, C)
fp32 sums from 0.0f over blocks of 256 sources (j ascending), float64 block totals in eight slices of whole blocks added in
order from 0.0, then in float64 xx = 3 A - D, xy = 3 B, yy = 3 C - D, each rounded once.  rsq is correctly rounded or moved
by whole ulps.  statement() is that pair statement for arrays, shared by device_model (whole worlds) and pair_model (one pair
onto sums of +0: what tests/tidal_cases.py holds to the derived pair bound, with PAIR_DEFECTS its one-token changes).  Two
deliberately wrong variants of the world model exist for the checkers of tests/test_tidal_cpu.py to reject:
    "merged diagonal"  one fp32 running sum per diagonal component, X = fma(dx, 3 * tx, X) - w: the factor 3 and the
                       difference of the two parts are rounded to float32 for every pair
    "f32 totals"       the block totals and the slices are added in float32
Nothing here is taken from a device run."""
from fractions import Fraction

import numpy as np

import nbody_amd as nb
from field_ref import pixel_points, probes  # noqa: F401  (re-exported: one import for the tidal tests)
from pair_cases import F32, F64, f32, fma32, rsq32

BLOCK = 256     # diag_common.h BLOCK
SLICES = 8      # diag_common.h W
VARIANTS = ("merged diagonal", "f32 totals")


def _sources(particles, m):
    a = np.asarray(particles, dtype=np.float32)
    gm32 = np.float32(nb.NB_G) * a[:m, 6]          # the float32 product
    assert gm32.dtype == np.float32
    return a[:m, 0], a[:m, 1], gm32


def t_at_f64(particles, m, points, softening):
    """(T, mag): float64 (n, 3) each in the order (xx, xy, yy); mag is the sum of the absolute PARTS of every term --
    sum G*m (3 dx^2 u^5 + u^3), sum 3 |dx dy| G*m u^5, sum G*m (3 dy^2 u^5 + u^3) -- so a bound built on it does not shrink
    where a diagonal component cancels."""
    x32, y32, gm32 = _sources(particles, m)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    x, y, gm = x32.astype(np.float64), y32.astype(np.float64), gm32.astype(np.float64)
    s = np.float64(np.float32(softening))
    t = np.zeros((pts.shape[0], 3), dtype=np.float64)
    mag = np.zeros((pts.shape[0], 3), dtype=np.float64)
    chunk = max(1, (1 << 21) // max(m, 1))
    for c in range(0, pts.shape[0], chunk):
        px, py = pts[c:c + chunk, 0].astype(np.float64), pts[c:c + chunk, 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            dx, dy = x[None, :] - px[:, None], y[None, :] - py[:, None]
            q = dx * dx + dy * dy + s
            u3 = gm[None, :] / (q * np.sqrt(q))
            u5 = u3 / q
            axx, axy, ayy = 3.0 * dx * dx * u5, 3.0 * dx * dy * u5, 3.0 * dy * dy * u5
            sl = slice(c, c + chunk)
            t[sl, 0], t[sl, 1], t[sl, 2] = (axx - u3).sum(axis=1), axy.sum(axis=1), (ayy - u3).sum(axis=1)
            mag[sl, 0], mag[sl, 1], mag[sl, 2] = (axx + u3).sum(axis=1), np.abs(axy).sum(axis=1), (ayy + u3).sum(axis=1)
    bad = ~np.isfinite(pts).all(axis=1)
    t[bad] = np.nan
    mag[bad] = np.nan
    return t, mag


def g_f64(particles, m, points64, softening):
    """float64 g (n, 2) at float64 points (n, 2): the sum of include/nbody_gravity.h evaluated where a float32 cannot stand."""
    x32, y32, gm32 = _sources(particles, m)
    p = np.asarray(points64, dtype=np.float64).reshape(-1, 2)
    x, y, gm = x32.astype(np.float64), y32.astype(np.float64), gm32.astype(np.float64)
    s = np.float64(np.float32(softening))
    dx, dy = x[None, :] - p[:, 0][:, None], y[None, :] - p[:, 1][:, None]
    q = dx * dx + dy * dy + s
    f = gm[None, :] / (q * np.sqrt(q))
    return np.stack([(dx * f).sum(axis=1), (dy * f).sum(axis=1)], axis=1)


def tidal_bound(t64, mag):
    """the project's force tolerance form (tests/gpu_common.py acc_bound), per component"""
    return 1e-4 * np.abs(t64) + 1e-6 * mag


def ratio_to_bound(got, t64, mag):
    """worst |got - t64| / tidal_bound over the samples and components"""
    bound = tidal_bound(t64, mag)
    assert np.all(bound > 0.0)
    return float(np.max(np.abs(np.asarray(got).astype(np.float64).reshape(-1, 3) - t64) / bound))


# ---- the float32 model -----------------------------------------------------------------------------------------------------------

# one-token changes of the statement, for the checkers of tests/tidal_cases.py to reject ("merged diagonal" is VARIANTS' own:
# 3 * tx rounded in fp32 for every pair)
PAIR_DEFECTS = ("softening dropped", "softening squared", "w5 = w", "tx = dx w", "C fmac with dx for dy", "B fmac with tx for ty",
                "D not subtracted from yy", "merged diagonal", "one g u factor dropped")


def statement(sx, sy, g, px, py, s, rsq_ulps=0, defect=None):
    """The pair statement at the head of this file up to its three fmac, one float32 rounding per line, for arrays that
    broadcast: dict of every intermediate, and the operand pairs fa, fb, fc of the fmac onto A, B and C.  `defect` names one of
    PAIR_DEFECTS (those that sit in the sums' finish are the caller's: pair_model)."""
    with np.errstate(all="ignore"):
        sx, sy, g, px, py, s = (f32(v) for v in (sx, sy, g, px, py, s))
        if defect == "softening dropped":
            s = np.zeros_like(s)
        elif defect == "softening squared":
            s = f32(s * s)
        dx, dy = f32(sx - px), f32(sy - py)
        q = fma32(dy, dy, fma32(dx, dx, s))
        u = rsq32(q, rsq_ulps)
        u2 = f32(u * u)
        gu = f32(g * u)
        w = f32(g * u2) if defect == "one g u factor dropped" else f32(gu * u2)
        w5 = w if defect == "w5 = w" else f32(w * u2)
        tx = f32(dx * (w if defect == "tx = dx w" else w5))
        ty = f32(dy * w5)
    return dict(dx=dx, dy=dy, q=q, u=u, u2=u2, gu=gu, w=w, w5=w5, tx=tx, ty=ty, fa=(dx, tx),
                fb=(dx, tx if defect == "B fmac with tx for ty" else ty), fc=(dx if defect == "C fmac with dx for dy" else dy, ty))


def pair_model(sx, sy, g, px, py, s, rsq_ulps=0, defect=None, parts=False):
    """float32 (n, 3): ONE source's term as the device forms it -- the statement onto sums of +0, the block totals to float64,
    xx = 3 A - D, xy = 3 B, yy = 3 C - D each rounded once.  With parts=True also the statement's dict, with A, B, C, D added."""
    assert defect is None or defect in PAIR_DEFECTS
    st = statement(sx, sy, g, px, py, s, rsq_ulps, defect)
    zero = F32(0.0)
    with np.errstate(all="ignore"):
        a, b, c, d = fma32(*st["fa"], zero), fma32(*st["fb"], zero), fma32(*st["fc"], zero), f32(zero + st["w"])
        a, b, c, d = (np.atleast_1d(v) for v in np.broadcast_arrays(a, b, c, d))
        if defect == "merged diagonal":
            xx = f32(fma32(st["dx"], f32(F32(3.0) * st["tx"]), zero) - st["w"]).astype(F64)
            yy = f32(fma32(st["dy"], f32(F32(3.0) * st["ty"]), zero) - st["w"]).astype(F64)
            xx, yy = (np.atleast_1d(v) for v in np.broadcast_arrays(xx, yy))
        else:
            xx = 3.0 * a.astype(F64) - d.astype(F64)
            yy = 3.0 * c.astype(F64) - (0.0 if defect == "D not subtracted from yy" else d.astype(F64))
        out = np.stack([xx, 3.0 * b.astype(F64), yy], axis=1).astype(F32)
    return (out, dict(st, A=a, B=b, C=c, D=d)) if parts else out

def _slices(totals, dtype):
    """(n, nblocks) block totals -> (n,): eight slices of whole blocks, each from 0 in block order, joined from 0 in order"""
    nblocks = totals.shape[1]
    per = -(-nblocks // SLICES)
    out = np.zeros(totals.shape[0], dtype=dtype)
    for w in range(SLICES):
        part = totals[:, w * per:(w + 1) * per].astype(dtype)
        sw = np.add.accumulate(part, axis=1)[:, -1] if part.shape[1] else np.zeros(totals.shape[0], dtype=dtype)
        out = (out + sw).astype(dtype)
    return out


def device_model(particles, m, points, softening, rsq_ulps=0, variant=None):
    """float32 (n, 3): what the statement and the summation at the head of this file give; variant None is the documented
    scheme, otherwise one of VARIANTS."""
    assert variant is None or variant in VARIANTS
    x32, y32, gm32 = _sources(particles, m)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    n = pts.shape[0]
    if m == 0:
        out = np.zeros((n, 3), dtype=F32)
        out[~np.isfinite(pts).all(axis=1)] = np.nan
        return out
    nblocks = -(-m // BLOCK)
    pad = nblocks * BLOCK - m            # padding sources of mass 0 at a real source's place add exact zeros to every sum
    sx = np.concatenate([x32, np.full(pad, x32[0], F32)]).reshape(nblocks, BLOCK)
    sy = np.concatenate([y32, np.full(pad, y32[0], F32)]).reshape(nblocks, BLOCK)
    sg = np.concatenate([gm32, np.zeros(pad, F32)]).reshape(nblocks, BLOCK)
    px, py = pts[:, 0][:, None], pts[:, 1][:, None]
    s = F32(softening)
    sums = [np.zeros((n, nblocks), dtype=F32) for _ in range(4)]          # A, B, C, D -- or X, B, Y, unused
    merged = variant == "merged diagonal"
    with np.errstate(all="ignore"):
        for i in range(BLOCK):                                             # every block at once, its sources in order
            st = statement(sx[None, :, i], sy[None, :, i], sg[None, :, i], px, py, s, rsq_ulps)
            sums[1] = fma32(*st["fb"], sums[1])
            if merged:
                sums[0] = f32(fma32(st["dx"], f32(F32(3.0) * st["tx"]), sums[0]) - st["w"])
                sums[2] = f32(fma32(st["dy"], f32(F32(3.0) * st["ty"]), sums[2]) - st["w"])
            else:
                sums[0] = fma32(*st["fa"], sums[0])
                sums[2] = fma32(*st["fc"], sums[2])
                sums[3] = f32(sums[3] + st["w"])
        dt = F32 if variant == "f32 totals" else F64
        a, b, c, d = (_slices(v, dt).astype(F64) for v in sums)
        if merged:
            out = np.stack([a, 3.0 * b, c], axis=1).astype(F32)
        else:
            out = np.stack([3.0 * a - d, 3.0 * b, 3.0 * c - d], axis=1).astype(F32)
    out[~np.isfinite(pts).all(axis=1)] = np.nan
    return out


# ---- worlds on which the documented scheme is exact or exactly summable ---------------------------------------------------------

EXACT_SOFT = 3.0
EXACT_P = (8.0, -16.0)


def exact_world(masses):
    """len(masses) sources at EXACT_P.  A probe at EXACT_P + (1, 0) with softening 3 has dx = -1, dy = 0, q = 4 and u = 1/2, so
    every instruction of the documented statement is exact for ANY G*m (products with powers of two only): the terms of the
    four sums are G*m (1/32, 0, 0, 1/8).  One source, or two of equal mass, are summed exactly whatever the mantissa of G*m;
    so are blocks of up to 256 equal sources whose G*m has a short mantissa (witness_masses).  The only rounding left is then
    the final one, of an exactly known value."""
    masses = np.asarray(masses, dtype=F32)
    a = np.zeros((masses.size, 8), dtype=F32)
    a[:, 0:2] = EXACT_P
    a[:, 6] = masses
    a[:, 7] = 1.0
    return a


def exact_probe():
    return np.array([[EXACT_P[0] + 1.0, EXACT_P[1]]], dtype=F32)


def exact_tensor(masses):
    """Fractions (xx, xy, yy) at exact_probe(): G*m (3 u^5 - u^3, 0, -u^3) with u = 1/2, summed exactly"""
    g = sum((Fraction(float(np.float32(nb.NB_G) * np.float32(v))) for v in np.asarray(masses, dtype=F32)), Fraction(0))
    return g * (Fraction(3, 32) - Fraction(1, 8)), Fraction(0), -g * Fraction(1, 8)


WITNESS_SMALL = 2.0 ** -12      # G*m = 10 * 2^-12: a mantissa of three bits, k * G*m is a float32 for every k <= 2^20
WITNESS_SHIFT = 33              # the big mass is 2^33 small ones: a block of 256 small terms totals 2^-25 of the big term


def witness_masses(m, at=0):
    """m - 1 small masses and one big one at index `at` (tests/sum_witness.py's pattern for blocks of 256)"""
    masses = np.full(m, WITNESS_SMALL, dtype=F32)
    masses[at] = F32(WITNESS_SMALL * 2.0 ** WITNESS_SHIFT)
    return masses


def ulp32(x):
    """the float32 ulp at the binade of the Fraction x != 0 (normal range)"""
    x = abs(Fraction(x))
    e = x.numerator.bit_length() - x.denominator.bit_length()
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    return Fraction(2) ** (e - 23)


def ulps_off(got, exact):
    """|got - exact| in float32 ulps at the binade of the exact Fraction; an exact zero must be returned as a zero"""
    if exact == 0:
        return 0.0 if float(got) == 0.0 else float("inf")
    return float(abs(Fraction(float(got)) - exact) / ulp32(exact))
