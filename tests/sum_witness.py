"""The summation witness (TEST INFRASTRUCTURE, no GPU needed to import): worlds whose force, field and energy sums are known
exactly, the bound the documented summation scheme implies, and numpy float32 models of that scheme and of two defective ones.

The witness.  All sources sit at one point P with radius 1 (source-on-source terms are exact zeros: dx = dy = 0) and carry
masses that are powers of two, so G*m is exact and scaling a mass by 2^k scales a term by exactly 2^k.  The receivers under
test are massless tracers of one radius at offsets from P whose components are powers of two or zero: dx and dy are exact and
the product dx * u that the accumulating v_fmac_f32 adds is itself a float32.  The term of one source is MEASURED (a world with
one source returns it bit for bit: 0 + t = t, and the close of a one-term block changes nothing), so nothing here trusts
v_rsq_f32; the sum of M such terms is then an integer multiple of float32 bit patterns and is formed in fractions.Fraction
(the patterns span about 57 bits: float64 cannot hold them).

The bound E(shape), in ulps of float32 at the binade of the exact result, restates DESIGN.md section 5 "Summation, per kernel
family": 1 ulp for the compensated sum of the block totals of the slice that holds the big term, and half an ulp for every
plain addition that joins partial sums behind it.

The models (plain running sum; blocks of L with plain totals; blocks of L with compensated totals) exist so that
tests/test_sum_witness_cpu.py can show, without a GPU, that the documented scheme stays inside E and the defective ones do
not, at the cases tests/test_gpu_sums.py runs (CASES below is the one table both files read)."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32

L_CLASSIC = 256     # kernels.hip CLOSE_EVERY * CHUNK: sources per plain block of step_kernel / chain_body
L_LANE = 128        # lane_split_body: a lane closes every 32 groups of four
L_FIELD = 256       # diag_common.h BLOCK: the field sampler and the diagnostics
FIELD_SLICES = 8    # diag_common.h W: float64 source slices

P0 = (8.0, -16.0)                                   # where the sources sit
OFFSETS = ((1.0, 0.0), (0.0, 2.0), (4.0, 0.5))      # tracer - P: components are powers of two or zero
PER_POSITION = 100                                  # 300 tracers: more than one receiver tile of every kernel
TRACER_RADIUS = 0.75
M_SMALL = 2.0 ** -12                                # the small mass; the two big ones are M_SMALL * 2^32 and * 2^33


def big_shift(L):
    """k with L * t_small = 2^-25 * t_big: one block of small terms totals a quarter ulp of the big term (mantissa 1.0)."""
    return 25 + int(math.log2(L))


# ---- worlds -----------------------------------------------------------------------------------------------------------------

def world(masses, positions=(0, 1, 2), tracers=3 * PER_POSITION, src_pos=None):
    """len(masses) sources at P0 (or src_pos, (M, 2)) followed by `tracers` massless tracers, tracer i at OFFSETS[positions[i *
    len(positions) // tracers]] from P0 (blocks of equal positions): partitioned as built."""
    masses = np.asarray(masses, dtype=F32)
    m = masses.size
    a = np.zeros((m + tracers, 8), dtype=F32)
    a[:m, 0:2] = P0 if src_pos is None else np.asarray(src_pos, dtype=F32)
    a[:m, 6] = masses
    a[:m, 7] = 1.0
    a[m:, 0:2] = np.asarray([tracer_point(p) for p in positions], dtype=F32)[tracer_positions(tracers, len(positions))]
    a[m:, 7] = TRACER_RADIUS
    assert np.all(a[:m, 6] > 0)
    return a


def tracer_point(p):
    return (P0[0] + OFFSETS[p][0], P0[1] + OFFSETS[p][1])


def tracer_positions(tracers, npos):
    """index into `positions` of every tracer"""
    return np.arange(tracers) * npos // tracers


def equal_masses(m):
    return np.full(m, M_SMALL, dtype=F32)


def one_big(m, L, at):
    """m - 1 small masses and one of M_SMALL * 2^big_shift(L) at index `at`."""
    masses = equal_masses(m)
    masses[at] = F32(M_SMALL * 2.0 ** big_shift(L))
    return masses


def big_positions(m, L=L_CLASSIC):
    """index 0, the middle of a block near the middle of the world, and the last index"""
    return {"first": 0, "middle": (m // 2) // L * L + L // 2 if m > L else m // 2, "last": m - 1}


MIRROR_POSITION = 2     # the tracers of a mirrored world all sit at P0 + OFFSETS[2] ...


def mirrored(m, L):
    """+big at P+ = P0 (index 0), m - 2 smalls at P+, the same big mass at P- (index m - 1), the mirror image of P+ in the
    tracers' position: its term is minus the first one's bit for bit (asserted where it is measured)."""
    masses = one_big(m, L, 0)
    masses[m - 1] = masses[0]
    pos = np.tile(np.asarray(P0, dtype=F32), (m, 1))
    pos[m - 1] = mirror_point()
    return world(masses, positions=(MIRROR_POSITION,), src_pos=pos)


def mirror_point():
    o = OFFSETS[MIRROR_POSITION]
    return (P0[0] + 2 * o[0], P0[1] + 2 * o[1])


def distinct(values, where):
    """the distinct bit patterns among the rows of `values` (n, ...) at each tracer position: [(position index, row), ...]"""
    v = np.ascontiguousarray(values)
    out = []
    for p in np.unique(where):
        rows = v[where == p].reshape(int((where == p).sum()), -1)
        for bits in np.unique(rows.view(np.uint32 if v.dtype == F32 else np.uint64), axis=0):
            out.append((int(p), bits.view(v.dtype)))
    return out


# ---- exact sums and ulps ------------------------------------------------------------------------------------------------------

def exact_sum(counted_terms):
    """sum of count * term over (count, float) pairs, as a Fraction (floats convert exactly)"""
    return sum((int(c) * Fraction(float(t)) for c, t in counted_terms), Fraction(0))


def ulp32(x):
    """the float32 ulp at the binade of the Fraction x != 0"""
    x = abs(Fraction(x))
    e = x.numerator.bit_length() - x.denominator.bit_length()
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    return Fraction(2) ** (e - 23)


def err_ulps(got, exact, scale=None):
    """signed (got - exact) in float32 ulps at the binade of `scale` (default: the exact result).  An exact zero must be
    returned as a zero: any other value is infinitely many ulps away."""
    exact = Fraction(exact)
    ref = exact if scale is None else Fraction(scale)
    d = Fraction(float(got)) - exact
    if ref == 0:
        return 0.0 if d == 0 else math.copysign(math.inf, d)
    return float(d / ulp32(ref))


# ---- the bound ----------------------------------------------------------------------------------------------------------------

def E(w=1, split=1, passes=1, lanes=1, parts=1):
    """Bound on |result - exact sum| in float32 ulps at the binade of the exact result, for the witness patterns with one big
    term: after the compensated level, the only roundings the big term sees are the plain additions that join partial sums."""
    e = 1.0                      # "Kahan over the block totals": the slice that holds the big term ends within 1 ulp
    e += 0.5 * (w - 1)           # "the W partial sums meet in LDS in wave order": W - 1 plain additions (0 + s_0 is exact)
    e += 0.5 * (split - 1)       # "parts added in order by finish_kernel" or by the tile's last workgroup: split - 1
    e += 0.5 * (passes - 1)      # "consecutive launches chained through acc[]": passes - 1 carries
    e += 0.5 * (lanes - 1)       # lane-split: "thread (c, r) adds W slices, then thread r adds those H sums": (W - 1) + (H - 1)
    e += 0.5 * (parts - 1)       # overlapped sharded step: "own slice, then the rest" carried through acc[]: one addition
    return e


E_FIELD = 1.0    # "float64 totals per block ... each component rounded once to float32": in-block loss <= 1/2 ulp, rounding 1/2 ulp

# Pattern 1: M equal terms t.  Every partial sum of the documented scheme is a sum of at most 256 terms rounded after each
# addition, so a block total is within 256 * 2^-24 relative of its exact value (Higham, n * u); the compensated totals and
# the few joining additions add O(2^-24) relative of the whole.  For M <= 4 500: 4 500 * 256 * 2^-24 = 0.069 t.
EXACTLY_ONCE_MAX = 4500


def exactly_once_bound_in_terms(m):
    return m * 256 * 2.0 ** -24 + m * 8 * 2.0 ** -24


# ---- float32 models -----------------------------------------------------------------------------------------------------------

SCHEMES = ("plain", "blocks", "kahan")     # running sum | blocks of L, plain totals | blocks of L, compensated totals


def seq_sum(x, dtype=F32):
    """0 + x[0] + x[1] + ... with one rounding per addition (ufunc.accumulate is strictly sequential)"""
    x = np.asarray(x, dtype=dtype)
    return dtype(np.add.accumulate(x)[-1]) if x.size else dtype(0)


def block_totals(x, L):
    """float32 plain sums of consecutive blocks of L terms (the last one short): one row per block, accumulated in order"""
    x = np.asarray(x, dtype=F32)
    nb = -(-x.size // L)
    if nb == 0:
        return np.zeros(0, dtype=F32)
    padded = np.zeros(nb * L, dtype=F32)     # a + 0.0f = a: the pad changes nothing
    padded[:x.size] = x
    return np.add.accumulate(padded.reshape(nb, L), axis=1)[:, -1].copy()


def kahan_totals(totals):
    """kernels.hip Receivers::close_chunk over the block totals, with its two selects"""
    s = c = F32(0)
    for a in totals:
        y = F32(a - c)
        t = F32(s + y)
        cn = F32(F32(t - s) - y)
        if a != 0:                            # a block that added exactly nothing changes nothing
            c = cn if abs(t) < np.inf else F32(0)
            s = t
    return s


def slice_sum(x, L, scheme):
    if scheme == "plain":
        return seq_sum(x)
    totals = block_totals(x, L)
    return seq_sum(totals) if scheme == "blocks" else kahan_totals(totals)


def source_slice(total, unit, parts, part, n, i):
    """kernels.hip source_slice"""
    nunits = -(-total // unit)
    per_part = -(-nunits // parts)
    part_lo = min(part * per_part, nunits)
    part_hi = min(part_lo + per_part, nunits)
    per = -(-(part_hi - part_lo) // n)
    u_lo = min(part_lo + i * per, part_hi)
    u_hi = min(u_lo + per, part_hi)
    lo = u_lo * unit
    return lo, max(min(u_hi * unit, total), lo)


def join(values):
    s = F32(0)
    for v in values:
        s = F32(s + v)
    return s


def classic_model(x, scheme, w=1, split=1, passes=1, unit=64, L=L_CLASSIC):
    """step_kernel (+ finish) over the terms x of one receiver component: passes of whole 64-source chunks chained through
    acc[], each pass cut into `split` parts, each part into w wave slices, each slice summed by `scheme`."""
    x = np.asarray(x, dtype=F32)
    chunks = -(-x.size // 64)
    P = max(1, min(passes, chunks))
    per = -(-chunks // P) * 64
    acc = None
    for q in range(P):
        seg = x[q * per:(q + 1) * per]
        parts = [join(slice_sum(seg[slice(*source_slice(seg.size, unit, split, y, w, i))], L, scheme) for i in range(w))
                 for y in range(split)]
        a = join(parts) if split > 1 else parts[0]
        acc = a if acc is None else F32(acc + a)
    return acc


def lane_split_model(x, scheme, w, h, L=L_LANE):
    """lane_split_body: tiles of 128 * w sources, each cut into w * h lane slices of whole 8-source granules; a lane closes a
    block every L sources it has added (exact here: the sizes used give every lane a multiple of four per tile)."""
    x = np.asarray(x, dtype=F32)
    T, V = 128 * w, w * h
    lanes = [[] for _ in range(V)]
    for t0 in range(0, x.size, T):
        tile = x[t0:t0 + T]
        for v in range(V):
            lo, hi = source_slice(tile.size, 8, 1, 0, V, v)
            lanes[v].append(tile[lo:hi])
    sums = [slice_sum(np.concatenate(p) if p else np.zeros(0, F32), L, scheme) for p in lanes]
    first = [join(sums[c * w:(c + 1) * w]) for c in range(h)]      # S = h first-level sums of PER = w slices each
    return join(first)


def sharded_model(x, scheme, ranks, rank, overlap, L=L_CLASSIC):
    """one wave (w = 1) of rank `rank` over the gathered sources: all of them in index order, or, overlapped, the rank's own
    slice in one launch and the rest (two ranges walked as one slice) in a second that carries the first through acc[].  The
    zero-mass pads behind each rank's slice add exact zeros and are left out."""
    x = np.asarray(x, dtype=F32)
    if not overlap:
        return slice_sum(x, L, scheme)
    mc = -(-x.size // ranks)
    own = x[rank * mc:(rank + 1) * mc]
    rest = np.concatenate([x[:rank * mc], x[(rank + 1) * mc:]])
    return F32(slice_sum(own, L, scheme) + slice_sum(rest, L, scheme))


def field_model(x, totals="f64"):
    """diag_common.h / field.hip: float32 plain sums over blocks of 256 sources (j ascending, blocks counted from source 0),
    block totals added in float64 in eight slices of whole blocks, the slices from 0.0 in order.  Returns the float64 sum;
    the field sampler rounds it once to float32.  totals = "f32": the defect, block totals and slices added in float32."""
    t = block_totals(x, L_FIELD)
    dt = np.float64 if totals == "f64" else F32
    per = -(-t.size // FIELD_SLICES)
    s = dt(0)
    for w in range(FIELD_SLICES):
        s = dt(s + seq_sum(t[w * per:(w + 1) * per].astype(dt), dt))
    return s


# ---- the cases of the witness ------------------------------------------------------------------------------------------------

def case(family, m, teeth, pattern="big", at="first", **shape):
    return dict(family=family, m=m, teeth=teeth, pattern=pattern, at=at, shape=shape)


def _classic_cases():
    out = []
    for at in ("first", "middle", "last"):
        t = at != "last"        # a big term added last meets sums that are already whole: nothing for a defect to lose
        out.append(case("classic", 16384, t, at=at, w=1))
        for w in (4, 16):
            out.append(case("classic", 16384, False, at=at, w=w))
        for split in (3, 16):
            out.append(case("classic", 16384, False, at=at, w=4, split=split))
        out.append(case("classic", 16384, False, at=at, w=1, passes=2))
    out.append(case("classic", 65536, True, at="first", w=1))
    out.append(case("classic", 16384, True, pattern="mirrored", w=1))
    out.append(case("classic", 16384, False, pattern="mirrored", w=16))
    return out


CASES = _classic_cases() + [
    case("lane", 65536, True, at="first", w=4, lanes=2),
    case("lane", 65536, True, at="middle", w=4, lanes=2),
    case("lane", 65536, False, at="last", w=4, lanes=2),
    case("lane", 65536, False, at="first", w=16, lanes=8),       # four closes per lane: one ulp of small terms, no teeth
    case("lane", 65536, False, at="middle", w=16, lanes=8),
] + [case("sharded", 16384, at != "last", at=at, ranks=p, overlap=o)
     for p in (2, 3) for o in (0, 1) for at in ("first", "middle", "last")] + [
    case("field", 16384, at != "last", at=at) for at in ("first", "middle", "last")
] + [case("diag", 16384, at != "last", at=at) for at in ("first", "middle", "last")]
# The one-workgroup chain and the ensembles (N <= 3 000) appear with no case that has teeth: at most 3 000 sources are twelve
# blocks of 256, three ulps of small terms in all, spread over 16 / tiles or W x H slices -- no slice holds the two blocks a
# lost compensation needs to show above E.  They carry pattern 1 (exactly once) and the bound of pattern 2 only.


def case_L(c):
    return {"classic": L_CLASSIC, "sharded": L_CLASSIC, "lane": L_LANE, "field": L_FIELD, "diag": L_FIELD}[c["family"]]


E_SECOND_BIG = 1.0
# The mirrored pattern holds TWO big terms, and its bound is in ulps of the big term.  The first one costs what E counts.  The
# second closes a block behind other blocks: its block total is rounded when it is formed (1/2 ulp of the big term) and once
# more where that total is rounded into its slice's sum (at w = 1 in close_chunk's y = a - c, whose c is by then of the order of
# the big term's ulp; at w > 1 in t = s + y of a slice of its own): one more ulp, whatever the shape.


def case_E(c):
    s = c["shape"]
    if c["family"] == "classic":
        return E(w=s.get("w", 1), split=s.get("split", 1), passes=s.get("passes", 1)) + (E_SECOND_BIG if c["pattern"] == "mirrored" else 0.0)
    if c["family"] == "lane":
        return E(w=s["w"], lanes=s["lanes"])
    if c["family"] == "sharded":
        return E(parts=2 if s["overlap"] else 1)
    return E_FIELD


def case_terms(c, t_small):
    """the terms of one receiver component in source order, and the exact sum, for a small term t_small (float32)"""
    L, m = case_L(c), c["m"]
    t_small = F32(t_small)
    t_big = F32(t_small * F32(2.0 ** big_shift(L)))
    x = np.full(m, t_small, dtype=F32)
    if c["pattern"] == "mirrored":
        x[0], x[m - 1] = t_big, -t_big
        return x, exact_sum([(m - 2, t_small)]), Fraction(float(t_big))
    x[big_positions(m, L)[c["at"]]] = t_big
    exact = exact_sum([(m - 1, t_small), (1, t_big)])
    return x, exact, exact


def case_model(c, x, scheme):
    """the model of case c's kernel family under `scheme` (for field / diag: "kahan" = the documented float64 totals, the two
    others = float32 totals)"""
    s = c["shape"]
    if c["family"] == "classic":
        return [classic_model(x, scheme, w=s.get("w", 1), split=s.get("split", 1), passes=s.get("passes", 1))]
    if c["family"] == "lane":
        return [lane_split_model(x, scheme, s["w"], s["lanes"])]
    if c["family"] == "sharded":
        return [sharded_model(x, scheme, s["ranks"], r, s["overlap"]) for r in range(s["ranks"])]
    v = field_model(x, "f64" if scheme == "kahan" else "f32")
    return [F32(v) if c["family"] == "field" else v]
