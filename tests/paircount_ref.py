"""The numpy model of include/nbody_paircount.h (TEST INFRASTRUCTURE): q of a pair in explicit float32 steps, the row rule in
float64 against e2 = (double)edge^2 (np.searchsorted, side="right"), the three classes, chunked by receiver rows so that
N = 6 000 fits in memory.  `variant` selects one of the defective restatements the checker must reject.  model_grid answers many
(M, edge set) questions about one set of positions with every pair evaluated once; it is held to model() by the CPU tests."""
import numpy as np

MM, MT, TT, ALL = 1, 2, 4, 7
NAMES = {MM: "mm", MT: "mt", TT: "tt"}
VARIANTS = ("self_pair", "ordered_twice", "edge_swapped", "e2_float32", "fused", "mt_in_mm")
SUBSETS = tuple(range(1, 8))          # every non-empty mask
CHUNK = 512


def names(mask):
    return tuple(NAMES[b] for b in (MM, MT, TT) if mask & b)


def pair_total(col, n, m):
    t = n - m
    return (m * (m - 1) // 2, m * t, t * (t - 1) // 2)[col]


def pair_q(xi, yi, xj, yj, fused=False):
    """q of include/nbody_paircount.h, float32, every operation rounded on its own.  fused: the defect, dx*dx + dy*dy with the
    first product kept exact (what contraction into an fma does), through float64 where a 24 x 24 bit product is exact."""
    with np.errstate(all="ignore"):
        dx = (xi - xj).astype(np.float32)
        dy = (yi - yj).astype(np.float32)
        dydy = (dy * dy).astype(np.float32)
        if fused:
            return (dx.astype(np.float64) * dx.astype(np.float64) + dydy.astype(np.float64)).astype(np.float32)
        return ((dx * dx).astype(np.float32) + dydy).astype(np.float32)


def edge2(edges, float32=False):
    e = np.asarray(edges, dtype=np.float32)
    return (e * e).astype(np.float64) if float32 else e.astype(np.float64) ** 2          # exact: 24-bit x 24-bit


def rows_of(q, e2, swapped=False):
    """The row of every q (the number of e2[t] <= q), -1 for a NaN."""
    r = np.searchsorted(e2, q.astype(np.float64), side="left" if swapped else "right")
    return np.where(np.isnan(q), -1, r)


def _count(x, y, r0, r1, s0, s1, tri, e2, variant):
    """(rows + 1,) counts of receivers [r0, r1) against sources [s0, s1); tri: the same range, j > i.  Last entry: NaN q."""
    rows = e2.shape[0] + 1
    h = np.zeros(rows + 1, dtype=np.uint64)
    j = np.arange(s0, s1)
    for i0 in range(r0, r1, CHUNK):
        i = np.arange(i0, min(i0 + CHUNK, r1))
        q = pair_q(x[i, None], y[i, None], x[None, s0:s1], y[None, s0:s1], fused=variant == "fused")
        if tri:
            keep = (j[None, :] >= i[:, None]) if variant == "self_pair" else (j[None, :] != i[:, None]) if variant == "ordered_twice" \
                else (j[None, :] > i[:, None])
            q = q[keep]
        r = rows_of(q.ravel(), e2, swapped=variant == "edge_swapped")
        h += np.bincount(np.where(r < 0, rows, r), minlength=rows + 1).astype(np.uint64)
    return h * np.uint64(2) if (variant == "ordered_twice" and not tri) else h


def model(part, mass_len, edges, classes=ALL, variant=None):
    """(out uint64 (bins + 2, 3), unplaced uint64 (3,)) for partitioned particles `part` (N, 8), mass_len massive ones first.  A
    class that is not asked for is never evaluated, and a particle only it would read is never read."""
    assert variant is None or variant in VARIANTS
    part = np.asarray(part, dtype=np.float32)
    n, m = part.shape[0], mass_len
    x, y = part[:, 0], part[:, 1]
    e2 = edge2(edges, float32=variant == "e2_float32")
    rows = e2.shape[0] + 1
    out, lost = np.zeros((rows, 3), dtype=np.uint64), np.zeros(3, dtype=np.uint64)
    ranges = {MM: (0, m, 0, m, True, 0), MT: (0, m, m, n, False, 1), TT: (m, n, m, n, True, 2)}
    for bit, (r0, r1, s0, s1, tri, col) in ranges.items():
        if not classes & bit or r1 <= r0 or s1 <= s0:
            continue
        h = _count(x, y, r0, r1, s0, s1, tri, e2, variant)
        if variant == "mt_in_mm" and bit == MT:
            col = 0
        out[:, col] += h[:rows]
        lost[col] += h[rows]
    return out, lost


def model_grid(part, masses, edge_sets):
    """{(M, k): (out, unplaced)} with classes = ALL for every M of `masses` and every edge set k, the positions being the same
    whatever M.  Every pair is evaluated once: the index range is cut at every M, a block of pairs is sorted once, and an edge
    set then only looks its e2 up in the sorted q (the number of q < e2[t], side="left", is what the rows below t hold)."""
    part = np.asarray(part, dtype=np.float32)
    n = part.shape[0]
    x, y = part[:, 0], part[:, 1]
    cuts = sorted({0, n, *masses})
    segs = [(a, b) for a, b in zip(cuts, cuts[1:])]
    e2s = [edge2(e) for e in edge_sets]
    hist = {}
    for ai, (r0, r1) in enumerate(segs):
        for bi in range(ai, len(segs)):
            s0, s1 = segs[bi]
            hs = [np.zeros(e2.shape[0] + 2, dtype=np.uint64) for e2 in e2s]
            j = np.arange(s0, s1)
            for i0 in range(r0, r1, 4 * CHUNK):
                i = np.arange(i0, min(i0 + 4 * CHUNK, r1))
                q = pair_q(x[i, None], y[i, None], x[None, s0:s1], y[None, s0:s1])
                q = q[j[None, :] > i[:, None]] if ai == bi else q.ravel()
                nan = np.isnan(q)
                qs = np.sort(q[~nan]).astype(np.float64)
                for h, e2 in zip(hs, e2s):
                    below = np.searchsorted(qs, e2, side="left")
                    h[:-1] += np.diff(np.concatenate([[0], below, [qs.shape[0]]])).astype(np.uint64)
                    h[-1] += np.uint64(np.count_nonzero(nan))
            hist[ai, bi] = hs
    res = {}
    for m in masses:
        for k, e2 in enumerate(e2s):
            rows = e2.shape[0] + 1
            out, lost = np.zeros((rows, 3), dtype=np.uint64), np.zeros(3, dtype=np.uint64)
            for (ai, bi), hs in hist.items():
                col = 0 if segs[bi][1] <= m else 2 if segs[ai][0] >= m else 1
                out[:, col] += hs[k][:rows]
                lost[col] += hs[k][rows]
            res[m, k] = (out, lost)
    return res


def masked(out, lost, classes):
    """What a call with `classes` must give, from the result of classes = ALL: the other columns are zeros."""
    keep = np.array([bool(classes & b) for b in (MM, MT, TT)])
    return out * keep.astype(np.uint64), lost * keep.astype(np.uint64)


def same(got, want):
    """The checker: uint64, the same shape, every count equal."""
    a, b = np.asarray(got), np.asarray(want)
    return a.dtype == np.uint64 and a.shape == b.shape and bool(np.array_equal(a, b.astype(np.uint64)))


def sums_to_class_totals(out, lost, n, m, classes):
    """The identity of the header: rows + unplaced = the class's number of pairs, zero for a class not asked for."""
    return all(int(out[:, c].sum()) + int(lost[c]) == (pair_total(c, n, m) if classes & (1 << c) else 0) for c in range(3))


def world(n, massive, seed=0, spread=10.0):
    """n particles, `massive` of them with mass > 0 and in front (the partitioned order).  The positions depend on n and the
    seed alone, not on `massive`."""
    rng = np.random.default_rng(seed)
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0:2] = rng.standard_normal((n, 2)) * spread + np.array([0.3, -0.2])
    a[:, 2:4] = rng.standard_normal((n, 2)) * 3.0
    a[:, 7] = 0.5 + rng.random(n)
    a[:massive, 6] = 0.5 + 99.5 * np.random.default_rng(seed + 1).random(massive)
    return a


def log_edges(bins, r_min=0.05, r_max=40.0):
    e = np.geomspace(r_min, r_max, bins + 1).astype(np.float32)
    assert np.all(np.diff(e) > 0)
    return e


def lin_edges(bins, r_max=50.0):
    e = np.linspace(0.0, r_max, bins + 1).astype(np.float32)          # edges[0] = 0: row 0 is empty
    assert np.all(np.diff(e) > 0)
    return e


BINS = (1, 2, 7, 64, 254)
SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)


def edge_sets(bins_list=BINS):
    """The edge sets of the grids: logarithmic for every bins, linear from 0 for 7 and 64."""
    return [log_edges(b) for b in bins_list] + [lin_edges(b) for b in bins_list if b in (7, 64)]


def masses(n):
    return sorted({0, min(1, n), n // 2, n})


# ---- the row rule at its edges ---------------------------------------------------------------------------------------------

EDGES_EXACT = np.array([0.5, 1.5, 2.5, 7.0], dtype=np.float32)          # every square is a float32


def _offsets_at(e, rng):
    """{-1, 0, +1} -> (dx, dy) float32 with q(dx, dy) one float32 below e^2, on it, one above; e^2 a float32."""
    e = np.float32(e)
    target = np.float32(e * e)
    want = {-1: np.nextafter(target, np.float32(0)), 0: target, 1: np.nextafter(target, np.float32(np.inf))}
    found = {0: (e, np.float32(0))}
    while len(found) < 3:
        a = rng.random() * 2 * np.pi
        dx, dy = np.float32(e * np.cos(a)), np.float32(e * np.sin(a))
        q = pair_q(np.float32(dx), np.float32(dy), np.float32(0), np.float32(0))
        for k in (-1, 1):
            if q == want[k]:
                found.setdefault(k, (dx, dy))
    return found


def edge_pairs():
    """name -> (two particles (2, 8), edges, the row their one pair lies in): q on e2[t], one float32 below and one above it, for
    the first, a middle and the last edge; coincident particles; edges[0] = 0; dx = -dy."""
    rng = np.random.default_rng(77)
    cases = {}

    def two(dx, dy, at=(0.0, 0.0)):
        a = np.zeros((2, 8), dtype=np.float32)
        a[0, 0:2] = at
        a[1, 0:2] = (np.float32(at[0]) + dx, np.float32(at[1]) + dy)          # exact for at = 0
        a[:, 6], a[:, 7] = 1.0, 0.25
        return a

    for t in (0, 2, 3):
        for k, (dx, dy) in _offsets_at(EDGES_EXACT[t], rng).items():
            cases[f"edge {t} {('below', 'on', 'above')[k + 1]}"] = (two(dx, dy), EDGES_EXACT, t if k < 0 else t + 1)
    cases["coincident, edges[0] = 0"] = (two(np.float32(0), np.float32(0), at=(3.5, -1.25)), lin_edges(7), 1)          # q = +0 = e2[0]: row 1
    cases["coincident, edges[0] > 0"] = (two(np.float32(0), np.float32(0), at=(3.5, -1.25)), EDGES_EXACT, 0)
    cases["dx = -dy"] = (two(np.float32(-1.5), np.float32(1.5)), EDGES_EXACT, 2)          # q = 4.5: between 1.5^2 and 2.5^2
    return cases


def edge_star():
    """One world that holds every offset of edge_pairs about a particle at the origin (those pairs have the q of the case; the
    others are whatever they are), massive and massless mixed: for bit equality with the model on more than one pair."""
    pts = [(0.0, 0.0)] + [tuple(a[1, 0:2]) for a, e, _ in edge_pairs().values() if e is EDGES_EXACT]
    a = np.zeros((len(pts), 8), dtype=np.float32)
    a[:, 0:2] = np.array(pts, dtype=np.float32)
    a[:, 7] = 0.25
    a[:len(pts) // 2, 6] = 1.0
    return a, len(pts) // 2, EDGES_EXACT


# An edge and a pair on which contracting q into an fma moves the row, found by search on the CPU: with dx*dx kept exact, q
# rounds one float32 away from the statement's q, across the edge's square.

def find_fused_witness(seed=5):
    """(dx, dy, edge): float32 with q_plain < (double)edge^2 <= q_fused or the other way round."""
    rng = np.random.default_rng(seed)
    while True:
        dx, dy = (np.float32(v) for v in rng.random(2) * 8 + 0.5)
        z = np.float32(0)
        a, b = pair_q(dx, dy, z, z), pair_q(dx, dy, z, z, fused=True)
        if a == b:
            continue
        lo, hi = (a, b) if a < b else (b, a)
        e = np.float32(np.sqrt(np.float64(hi)))
        for cand in (e, np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(np.inf))):
            if np.float64(lo) < np.float64(cand) ** 2 <= np.float64(hi):
                return dx, dy, cand


def fused_world():
    """(particles, mass_len, edges): 40 massive particles, two of them the witness pair about its own edge."""
    dx, dy, e = find_fused_witness()
    a = world(40, 40, seed=11, spread=50.0)
    a[0, 0:2], a[1, 0:2] = (0.0, 0.0), (dx, dy)
    edges = np.array([np.float32(e) / 2, e, np.float32(e) * 4], dtype=np.float32)
    return a, 40, edges


def nonfinite_worlds():
    """name -> (particles, mass_len, edges, classes)."""
    e = EDGES_EXACT
    cases = {}
    a = world(300, 150, seed=31)
    a[7, 0] = np.inf
    cases["one particle at +inf"] = (a, 150, e, ALL)          # its pairs: q = +inf, the last row
    a = world(300, 150, seed=32)
    a[7, 0], a[200, 0] = np.inf, np.inf
    cases["two at +inf on one axis"] = (a, 150, e, ALL)       # inf - inf: their pair is NaN -> unplaced (MT)
    a = world(300, 150, seed=33)
    a[9, 1], a[10, 0], a[250, 0] = np.nan, np.nan, np.nan
    cases["NaN positions"] = (a, 150, e, ALL)
    a = world(600, 300, seed=34)
    a[300:, 0:6] = np.nan
    cases["massless rows of NaN, mm only"] = (a, 300, e, MM)
    return cases


def threshold(edge):
    """The smallest float32 c with (double)c >= (double)edge^2: the device's threshold, restated."""
    e2 = np.float64(np.float32(edge)) ** 2
    with np.errstate(over="ignore"):
        c = np.float32(e2)
    return np.nextafter(c, np.float32(np.inf)) if np.float64(c) < e2 else c
