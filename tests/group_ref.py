"""The numpy model of include/nbody_group.h: q in float32 with every operation rounded on its own (paircount_ref.pair_q), the
float64 comparison against linking_length^2, and the components of the link graph by min-label propagation to a fixpoint.
double_loop is the second, independent statement -- a plain Python double loop and a depth-first search -- the model is checked
against.  `variant` selects one of the defective restatements the checker must reject.  A plain helper module."""
import numpy as np

from neighbour_ref import ALL, MASKS, MASSIVE, MASSLESS, NAMES, span  # noqa: F401  the masks are include/nbody_neighbour.h's
from paircount_ref import pair_q, world  # noqa: F401

NONE = 0xFFFFFFFF
ROWS = 512          # receivers evaluated at a time
VARIANTS = ("le", "largest_index", "one_sweep", "mask_bridges", "fused", "l2_float32", "coincident_unlinked", "nan_links",
            "global_labels")


def length2(linking_length, float32=False):
    l = np.float32(linking_length)
    if float32:          # the defect: the square rounded to float32
        with np.errstate(over="ignore"):
            return np.float64(np.float32(l * l))
    return np.float64(l) * np.float64(l)          # exact: 24-bit x 24-bit


def links(x, y, lo, hi, linking_length, variant=None):
    """The linked pairs (i, j), j < i, both in [lo, hi): two int64 arrays."""
    l2 = length2(linking_length, float32=variant == "l2_float32")
    ii, jj = [], []
    for a in range(lo, hi, ROWS):
        i = np.arange(a, min(a + ROWS, hi))
        j = np.arange(lo, i[-1])          # every j below the last receiver of the block
        if not len(j):
            continue
        q = pair_q(x[i, None], y[i, None], x[None, j], y[None, j], fused=variant == "fused")
        with np.errstate(invalid="ignore"):
            qd = q.astype(np.float64)
            hit = qd <= l2 if variant == "le" else ~(qd >= l2) if variant == "nan_links" else qd < l2
        if variant == "coincident_unlinked":
            hit &= ~((x[i, None] == x[None, j]) & (y[i, None] == y[None, j]))
        hit &= j[None, :] < i[:, None]
        r, c = np.nonzero(hit)
        ii.append(i[r])
        jj.append(j[c])
    if not ii:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64)


def propagate(n, ii, jj, largest=False, sweeps=None):
    """label[i] = the smallest (largest) index connected to i: every sweep gives each end of a link the better label of the two,
    and (an accelerator that keeps the fixpoint: a label is an index of the same component) follows label[label]; until nothing
    changes.  sweeps: stop after that many plain sweeps, the defect."""
    label = np.arange(n, dtype=np.int64)
    best = np.maximum if largest else np.minimum
    done = 0
    while True:
        new = label.copy()
        best.at(new, ii, label[jj])
        best.at(new, jj, label[ii])
        done += 1
        if sweeps is not None:
            if done >= sweeps:
                return new
        else:
            new = new[new]
        if np.array_equal(new, label):
            return label
        label = new


def groups(pos, n, m, members, linking_length, variant=None):
    """labels uint32 (n,) of the partitioned positions pos (n, >= 2), m of them massive."""
    assert variant is None or variant in VARIANTS
    p = np.asarray(pos, dtype=np.float32)
    assert p.shape[0] == n
    x, y = np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])
    lo, hi = span(members, n, m)
    s_lo, s_hi = (0, n) if variant == "mask_bridges" else (lo, hi)
    ii, jj = links(x, y, s_lo, s_hi, linking_length, variant)
    label = propagate(n, ii, jj, largest=variant == "largest_index", sweeps=1 if variant == "one_sweep" else None)
    if variant == "mask_bridges":          # the components of all particles, each named by its smallest member of the mask
        first = np.full(n, n, dtype=np.int64)
        inside = np.arange(lo, hi)
        np.minimum.at(first, label[inside], inside)
        label = first[label]
    out = np.full(n, NONE, dtype=np.uint32)
    out[lo:hi] = label[lo:hi].astype(np.uint32)
    return out


def model(part, mass_len, members=ALL, linking_length=1.0, variant=None):
    part = np.asarray(part, dtype=np.float32)
    return groups(part, part.shape[0], int(mass_len), members, linking_length, variant)


def ensemble(parts, masses, members=ALL, linking_length=1.0, variant=None):
    """A list of labels, one array per member; labels count within the member (the defect global_labels: within the packed array)."""
    out, base = [], 0
    for part, m in zip(parts, masses):
        lab = model(part, m, members, linking_length, None if variant == "global_labels" else variant)
        if variant == "global_labels":
            lab = np.where(lab == NONE, np.uint32(NONE), (lab.astype(np.uint64) + np.uint64(base)).astype(np.uint32))
        out.append(lab)
        base += len(lab)
    return out


def double_loop(part, mass_len, members=ALL, linking_length=1.0):
    """The statement as two plain loops, one pair at a time, and a depth-first search from every index in increasing order."""
    p = np.asarray(part, dtype=np.float32)
    n, m = p.shape[0], int(mass_len)
    lo, hi = span(members, n, m)
    l2 = float(np.float32(linking_length)) * float(np.float32(linking_length))
    friends = [[] for _ in range(n)]
    for i in range(lo, hi):
        for j in range(lo, i):
            with np.errstate(all="ignore"):
                dx, dy = np.float32(p[i, 0] - p[j, 0]), np.float32(p[i, 1] - p[j, 1])
                v = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
            if float(v) < l2:
                friends[i].append(j)
                friends[j].append(i)
    out = np.full(n, NONE, dtype=np.uint32)
    for start in range(lo, hi):          # increasing: the first index to reach a component is its smallest
        if out[start] != NONE:
            continue
        stack = [start]
        out[start] = start
        while stack:
            for k in friends[stack.pop()]:
                if out[k] == NONE:
                    out[k] = start
                    stack.append(k)
    return out


def count(labels):
    """n_groups of one world's labels."""
    lab = np.asarray(labels)
    return int(np.count_nonzero(lab == np.arange(len(lab), dtype=np.uint32)))


def same(got, want):
    """The checker's comparison: uint32, the same shape, every bit equal."""
    a, b = np.asarray(got), np.asarray(want)
    return a.dtype == np.uint32 and b.dtype == np.uint32 and a.shape == b.shape and a.tobytes() == b.tobytes()


def checker(got, part, mass_len, members=ALL, linking_length=1.0, variant=None):
    """Is `got` what the model -- or one of its defective variants -- says, bit for bit?"""
    return same(got, model(part, mass_len, members, linking_length, variant))


def masses(n):
    return sorted({0, min(1, n), n // 3, max(n - 1, 0), n})


def length_for(n, spread=3.0, b=1.0):
    """A linking length at which world(n, ., spread=spread) holds groups of many sizes: b times about the mean separation."""
    return float(np.float32(b * spread * np.sqrt(2.0 * np.pi / max(n, 1))))


def blank(n, m=None):
    a = np.zeros((n, 8), dtype=np.float32)
    a[:, 7] = 0.25
    a[:n if m is None else m, 6] = 1.0
    return a


def chain(n, seed=0, m=None):
    """n particles at x = k, y = 0 (exact in float32) in a seeded shuffled index order: one link graph of diameter n - 1 whose
    every link hops between arbitrary indices.  Returns (particles, the k of every index)."""
    k = np.random.default_rng(seed).permutation(n)
    a = blank(n, m)
    a[:, 0] = k
    return a, k


def two_chains(n, seed=0):
    """Even k at y = 0, odd k at y = 10, x = k, shuffled: neighbours along a chain are 2 apart, the chains 10."""
    k = np.random.default_rng(seed).permutation(n)
    a = blank(n)
    a[:, 0], a[:, 1] = k, np.where(k % 2 == 0, 0.0, 10.0)
    return a, k


def lattice(side, spacing=1.0, m=None):
    a = blank(side * side, m)
    a[:, 0], a[:, 1] = np.tile(np.arange(side), side) * spacing, np.repeat(np.arange(side), side) * spacing
    return a


def coincident(n, m=None, at=(1.5, -2.25)):
    a = blank(n, m)
    a[:, 0], a[:, 1] = at
    return a


def above(v):
    """The next float32 above v."""
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))
