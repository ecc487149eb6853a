"""The numpy model of include/nbody_profile.h (TEST INFRASTRUCTURE): the per-particle statement in explicit float64 steps, the
row rule, and the chunked summation order with sequential additions (np.add.accumulate from +0.0, never np.sum, whose pairwise
order is not the contract).  `variant` selects one of the defective restatements the checker must reject."""
from fractions import Fraction

import numpy as np

CHUNK = 1024
QTY = 6
BY_MASS, BY_NUMBER = 0, 1
VARIANTS = ("edge_swapped", "chunk_1000", "pairwise", "reads_massless", "fused")


def seq_sum(x):
    """((+0.0 + x[0]) + x[1]) + ... : one rounding per addition, in index order."""
    return np.add.accumulate(np.concatenate([[0.0], x]))[-1]


def pair_sum(x):
    """The pairwise tree a library sum would use: NOT the contract."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[0] <= 2:
        return seq_sum(x)
    h = x.shape[0] // 2
    return pair_sum(x[:h]) + pair_sum(x[h:])


def terms(part, centre, wgt, fused=False):
    """q and the five columns (wgt, wgt q, wgt j, wgt w, wgt k) of every particle, float64, each operation rounded on its own."""
    c = np.asarray(centre, dtype=np.float32).astype(np.float64)
    x, y, vx, vy = (part[:, i].astype(np.float64) for i in range(4))
    with np.errstate(all="ignore"):
        dx, dy, sx, sy = x - c[0], y - c[1], vx - c[2], vy - c[3]
        if fused:          # the defect: a b +- e f exactly, rounded once (what an fma chain or a double-double would approach); finite data only
            two = lambda a, b, e, f, sign: np.array([float(Fraction(p) * Fraction(q_) + sign * Fraction(r) * Fraction(s))
                                                     for p, q_, r, s in zip(a.tolist(), b.tolist(), e.tolist(), f.tolist())])
        else:
            two = lambda a, b, e, f, sign: a * b + sign * (e * f)
        q = two(dx, dx, dy, dy, 1)
        j = two(dx, sy, dy, sx, -1)
        w = two(dx, sx, dy, sy, 1)
        k = two(sx, sx, sy, sy, 1)
        return q, np.stack([wgt, wgt * q, wgt * j, wgt * w, wgt * k], axis=1)


def rows_of(q, edges, swapped=False):
    e2 = np.asarray(edges, dtype=np.float32).astype(np.float64) ** 2          # exact: 24-bit x 24-bit
    r = np.searchsorted(e2, q, side="left" if swapped else "right")          # right: the number of e2[t] <= q
    return np.where(np.isnan(q), -1, r)


def model(part, mass_len, edges, centre=(0, 0, 0, 0), weights=BY_MASS, variant=None):
    """(out float64 (bins + 2, 6), unplaced) for partitioned particles `part` (N, 8) with mass_len massive ones first."""
    assert variant is None or variant in VARIANTS
    part = np.asarray(part, dtype=np.float32)
    bins = len(edges) - 1
    n = part.shape[0] if (weights == BY_NUMBER or variant == "reads_massless") else mass_len
    p = part[:n]
    wgt = p[:, 6].astype(np.float64) if weights == BY_MASS else np.ones(n)
    q, cols = terms(p, centre, wgt, fused=variant == "fused")
    row = rows_of(q, edges, swapped=variant == "edge_swapped")
    chunk = 1000 if variant == "chunk_1000" else CHUNK
    add = pair_sum if variant == "pairwise" else seq_sum
    out = np.zeros((bins + 2, QTY))
    with np.errstate(all="ignore"):
        for first in range(0, n, chunk):
            r, t = row[first:first + chunk], cols[first:first + chunk]
            tot = np.zeros((bins + 2, QTY))
            for k in np.unique(r[r >= 0]):
                mine = t[r == k]
                tot[k, 0] = mine.shape[0]
                for c in range(5):
                    tot[k, 1 + c] = add(mine[:, c])
            out = out + tot          # every row, the empty ones add +0.0
    return out, int(np.count_nonzero(row < 0))


def same(got, want):
    """The checker: the same bits wherever both are finite (the sign of a zero included), the same class (NaN, +inf, -inf)
    elsewhere -- a NaN's sign and payload are the machine's, not the statement's."""
    a, b = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    if a.shape != b.shape:
        return False
    bits = a.view(np.uint64) == b.view(np.uint64)
    nan = np.isnan(a) & np.isnan(b)
    inf = np.isinf(a) & np.isinf(b) & (np.signbit(a) == np.signbit(b))
    finite = np.isfinite(a) & np.isfinite(b)
    return bool(np.all(np.where(finite, bits, nan | inf)))


def world(n, massive, seed=0, spread=10.0):
    """n particles, `massive` of them with mass > 0 and in front (the partitioned order), about (0.3, -0.2)."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * spread + np.array([0.3, -0.2])
    a[:, 2:4] = rng.standard_normal((n, 2)) * 3.0
    a[:massive, 6] = 0.5 + 99.5 * rng.random(massive)
    a[:, 7] = 0.5 + rng.random(n)
    return a


def log_edges(bins, r_min=0.05, r_max=40.0):
    e = np.geomspace(r_min, r_max, bins + 1).astype(np.float32)
    assert np.all(np.diff(e) > 0)
    return e


CENTRE = (0.3, -0.2, 0.125, -0.0625)
SIZES = (1, 1023, 1024, 1025, 2049, 3000)          # around one and two chunk boundaries, and the largest ensemble member
BINS = (1, 2, 63, 254)


def grid(n):
    """(mass_len, bins, weights) of the size's cases."""
    return [(m, b, w) for m in sorted({0, 1, n // 2, n}) for b in BINS for w in (BY_MASS, BY_NUMBER)]


def edge_case_worlds():
    """name -> (particles, mass_len, edges, centre, weights): the placements the header spells out."""
    e = np.array([0.0, 1.5, 2.5, 7.0], dtype=np.float32)
    cases = {}
    a = world(40, 40, seed=3)
    a[5, 0:2] = (2.5, 0.0)          # q == e2[2] exactly: row 3, not row 2
    a[6, 0:2] = (0.0, -1.5)         # q == e2[1] exactly: row 2
    cases["on an edge"] = (a, 40, e, (0, 0, 0, 0), BY_MASS)
    a = world(40, 40, seed=4)
    cases["centre on a particle, edges[0] = 0"] = (a, 40, e, (a[7, 0], a[7, 1], 0, 0), BY_MASS)          # q = 0 = e2[0]: row 1
    a = world(1500, 900, seed=5, spread=0.1)
    cases["all in one row"] = (a, 900, np.array([0.0, 50.0], dtype=np.float32), CENTRE, BY_NUMBER)
    a = world(1500, 900, seed=6)
    cases["all beyond the last edge"] = (a, 900, np.array([1e-6, 2e-6, 3e-6], dtype=np.float32), CENTRE, BY_MASS)
    a = world(1100, 1100, seed=7)
    a[3, 0], a[1030, 1], a[1031, 0] = np.nan, np.nan, np.nan          # unplaced, in both chunks
    a[8, 0], a[9, 1] = np.inf, -np.inf                              # q = +inf: the last row
    cases["NaN and inf positions"] = (a, 1100, e, CENTRE, BY_MASS)
    a = world(1100, 1100, seed=8)
    a[20, 2], a[1050, 3] = np.inf, -np.inf                          # placed; L, W, K of their rows go non-finite
    cases["inf velocity of a placed particle"] = (a, 1100, e, CENTRE, BY_MASS)
    a = world(600, 300, seed=9)
    a[300:, 0:6] = np.nan                                           # massless rows full of NaN: never read in mass mode
    cases["massless rows of NaN"] = (a, 300, e, CENTRE, BY_MASS)
    return cases
