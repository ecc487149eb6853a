"""The numpy model of include/nbody_neighbour.h: float32 operations one by one, the candidates as a mask, and the neighbour as the
minimum over the 64-bit key (bits(q) << 32) | j.  `chunk` evaluates the sources in pieces and merges keys by minimum and counts by
addition: the order-free argument, run.  double_loop is the plain restatement the model is checked against.  `variant` selects one
of the defective restatements the checker must reject.  A plain helper module."""
import numpy as np

from paircount_ref import pair_q, world

MASSIVE, MASSLESS, ALL = 1, 2, 3
NONE = 0xFFFFFFFF
MASKS = (MASSIVE, MASSLESS, ALL)
NAMES = {MASSIVE: "massive", MASSLESS: "massless", ALL: "all"}
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
INF_BITS = 0x7F800000
ROWS = 256          # receivers evaluated at a time
VARIANTS = ("self_included", "self_by_position", "largest_index", "radius_le", "nan_smallest", "inf_candidate", "source_mask_ignored",
            "unrequested_read")


def span(mask, n, m):
    """[lo, hi) of a class mask."""
    return (0 if mask & MASSIVE else m), (n if mask & MASSLESS else m)


def radius2(radius):
    return np.float64(np.float32(radius)) * np.float64(np.float32(radius))          # exact: 24-bit x 24-bit


def _block(x, y, rows, cols, r2, variant):
    """keys (len(rows),) uint64 and counts (len(rows),) uint32 of the receivers `rows` against the sources `cols`."""
    i, j = rows[:, None], cols[None, :]
    q = pair_q(x[i], y[i], x[j], y[j])
    if variant == "unrequested_read":          # the defect: every particle of the world enters, multiplied by zero
        with np.errstate(all="ignore"):
            q = (q + np.float32(0) * (x.sum(dtype=np.float32) + y.sum(dtype=np.float32))).astype(np.float32)
    if variant == "self_included":
        other = np.ones(q.shape, dtype=bool)
    elif variant == "self_by_position":
        other = ~((x[i] == x[j]) & (y[i] == y[j]))
    else:
        other = i != j
    with np.errstate(invalid="ignore"):
        reach = q <= np.float32(np.inf) if variant == "inf_candidate" else q < np.float32(np.inf)          # false for a NaN
    bits = q.view(np.uint32).astype(np.uint64)
    if variant == "nan_smallest":
        reach = reach | np.isnan(q)
        bits = np.where(np.isnan(q), np.uint64(0), bits)
    cand = other & reach
    low = (np.uint64(NONE - 1) - j.astype(np.uint64)) if variant == "largest_index" else j.astype(np.uint64)
    keys = np.where(cand, (bits << np.uint64(32)) | low, KEY_NONE)
    if r2 is None:
        counts = np.zeros(len(rows), dtype=np.uint32)
    else:
        with np.errstate(invalid="ignore"):
            qd = q.astype(np.float64)
            within = qd <= r2 if variant == "radius_le" else qd < r2
        counts = (cand & within).sum(axis=1).astype(np.uint32)
    return keys.min(axis=1) if len(cols) else np.full(len(rows), KEY_NONE), counts


def model(part, mass_len, receivers=ALL, sources=ALL, radius=None, variant=None, chunk=None):
    """(q float32 (N,), index uint32 (N,), count uint32 (N,) or None) of partitioned particles."""
    p = np.asarray(part, dtype=np.float32)
    n, m = p.shape[0], int(mass_len)
    x, y = np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])
    r0, r1 = span(receivers, n, m)
    s0, s1 = span(ALL if variant == "source_mask_ignored" else sources, n, m)
    r2 = None if radius is None else radius2(radius)
    keys, counts = np.full(n, KEY_NONE), np.zeros(n, dtype=np.uint32)
    step = max(s1 - s0, 1) if chunk is None else int(chunk)
    for a in range(r0, r1, ROWS):
        rows = np.arange(a, min(a + ROWS, r1))
        for b in range(s0, s1, step):          # any split of the sources: keys by minimum, counts by addition
            k, c = _block(x, y, rows, np.arange(b, min(b + step, s1)), r2, variant)
            keys[rows] = np.minimum(keys[rows], k)
            counts[rows] += c
    index = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    if variant == "largest_index":
        index = np.where(keys == KEY_NONE, np.uint32(NONE), (np.uint32(NONE - 1) - index).astype(np.uint32))
    bits = np.where(index == NONE, np.uint64(INF_BITS), keys >> np.uint64(32)).astype(np.uint32)
    q = bits.view(np.float32)
    if variant == "nan_smallest":          # what it took for the smallest, it reports
        has = index != NONE
        q = q.copy()
        q[has] = pair_q(x[has], y[has], x[index[has]], y[index[has]])
    return q, index, (None if radius is None else counts)


def double_loop(part, mass_len, receivers=ALL, sources=ALL, radius=None):
    """The statement as two plain loops, one pair at a time."""
    p = np.asarray(part, dtype=np.float32)
    n, m = p.shape[0], int(mass_len)
    r0, r1 = span(receivers, n, m)
    s0, s1 = span(sources, n, m)
    q, index, count = np.full(n, np.inf, dtype=np.float32), np.full(n, NONE, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    r2 = None if radius is None else float(np.float32(radius)) * float(np.float32(radius))
    for i in range(r0, r1):
        for j in range(s0, s1):
            if j == i:
                continue
            with np.errstate(all="ignore"):
                dx, dy = np.float32(p[i, 0] - p[j, 0]), np.float32(p[i, 1] - p[j, 1])
                v = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
            if not v < np.float32(np.inf):
                continue
            if v < q[i]:
                q[i], index[i] = v, j
            if r2 is not None and float(v) < r2:
                count[i] += 1
    return q, index, (None if radius is None else count)


def same(got, want):
    """The checker's comparison: the same number of arrays, each of the stated dtype and shape, every bit equal."""
    if len(got) != len(want):
        return False
    for a, b, dtype in zip(got, want, (np.float32, np.uint32, np.uint32)):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype != dtype or b.dtype != dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            return False
    return True


def checker(got, part, mass_len, receivers=ALL, sources=ALL, radius=None, variant=None, chunk=None):
    """Is `got` what the model -- or one of its defective variants -- says, bit for bit?"""
    want = model(part, mass_len, receivers, sources, radius, variant, chunk)
    return same(tuple(got), tuple(a for a in want if a is not None))


def masses(n):
    return sorted({0, min(1, n), n // 3, max(n - 1, 0), n})


def lattice(side, spacing=1.0, massive=None):
    """side x side particles on a square lattice, row after row; all massive unless told."""
    a = np.zeros((side * side, 8), dtype=np.float32)
    a[:, 0], a[:, 1] = np.tile(np.arange(side), side) * spacing, np.repeat(np.arange(side), side) * spacing
    a[:, 7] = 0.25
    a[:side * side if massive is None else massive, 6] = 1.0
    return a


def coincident(n, m, at=(1.5, -2.25)):
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 0], a[:, 1], a[:, 7] = at[0], at[1], 0.25
    a[:m, 6] = 1.0
    return a


def nonfinite_worlds():
    """name -> (particles, mass_len): NaN and +-inf positions, and separations whose q overflows."""
    out = {}
    a = world(70, 30, seed=11)
    a[3, 0], a[40, 1] = np.nan, np.nan
    out["NaN positions"] = (a, 30)
    a = world(70, 30, seed=12)
    a[5, 0], a[50, 1], a[51, 1] = np.inf, -np.inf, -np.inf
    out["inf positions"] = (a, 30)
    a = world(66, 66, seed=13)
    a[0, 0], a[1, 0], a[2, 1] = 3.0e19, -3.0e19, 2.5e19          # differences square past FLT_MAX: q = +inf, never a candidate
    out["q overflows"] = (a, 66)
    a = world(3, 3, seed=14)
    a[:, 0] = [np.nan, np.inf, 1.0]
    out["nobody has a candidate"] = (a, 3)
    return out
