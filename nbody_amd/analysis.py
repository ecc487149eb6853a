"""Readers of what the read-only calls return: numpy only, no library call."""
import numpy as np

from ._abi import NB_GROUP_NONE, NB_NEIGH_NONE, NB_PAIRS_COLUMNS, NB_PROFILE_MAX_BINS, NB_PROFILE_QTY


def neighbour_distance(q):
    """float64 sqrt(q) of the q of .neighbours(): the distance to the nearest neighbour, +inf kept where there is none."""
    return np.sqrt(np.asarray(q, dtype=np.float64))


def closest_pairs(q, index, k=1):
    """The k closest unordered pairs among the nearest-neighbour links of one world's .neighbours(): a list of (i, j, q) with
    i < j, sorted by (q, i, j); a mutual pair appears once, a particle without a neighbour in none.  The first row is the closest
    encounter of the world: the two particles that set an adaptive step."""
    q, index = np.asarray(q, dtype=np.float32), np.asarray(index, dtype=np.uint32)
    if q.ndim != 1 or index.shape != q.shape:
        raise ValueError("q and index must be the (N,) arrays of one world")
    if k < 0:
        raise ValueError("k must not be negative")
    has = np.nonzero(index != NB_NEIGH_NONE)[0]
    pairs = {(min(int(i), int(index[i])), max(int(i), int(index[i]))): float(q[i]) for i in has}
    rows = sorted((v, i, j) for (i, j), v in pairs.items())[:k]
    return [(i, j, v) for v, i, j in rows]


def group_table(labels, weights=None, min_members=1):
    """The groups of one world's .groups() labels: (roots, sizes), or (roots, sizes, sums) with per-particle `weights` (float64
    sums of the weights of each group's members, mass for instance).  roots uint32, the labels that occur; sizes int64, their
    member counts.  Sorted by size descending, then by root ascending; groups of fewer than min_members are left out; particles
    labelled nb.NB_GROUP_NONE (outside the mask) are in none."""
    lab = np.asarray(labels, dtype=np.uint32)
    if lab.ndim != 1:
        raise ValueError("labels must be the (N,) array of one world")
    of_mask = lab != NB_GROUP_NONE
    roots, inverse, sizes = np.unique(lab[of_mask], return_inverse=True, return_counts=True)
    order = np.lexsort((roots, -sizes))
    order = order[sizes[order] >= min_members]
    out = (roots[order].astype(np.uint32), sizes[order].astype(np.int64))
    if weights is None:
        return out
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != lab.shape:
        raise ValueError("weights must have one entry per label")
    sums = np.bincount(inverse.reshape(-1), weights=w[of_mask], minlength=roots.shape[0])
    return out + (sums[order],)


def group_members(labels, root):
    """The indices of the particles labelled `root` in one world's .groups() labels, ascending (int64); the first is root itself."""
    lab = np.asarray(labels, dtype=np.uint32)
    if lab.ndim != 1:
        raise ValueError("labels must be the (N,) array of one world")
    return np.nonzero(lab == np.uint32(root))[0]


def linking_length_for(n, area, b=0.2):
    """b times the mean separation of n particles spread over `area` in the plane, b * sqrt(area / n): the usual way to choose
    a friends-of-friends linking length (b = 0.2 is the customary value)."""
    if not n > 0 or not area > 0 or not b >= 0:
        raise ValueError("need n > 0, area > 0 and b >= 0")
    return float(b) * float(np.sqrt(float(area) / float(n)))


def pair_curves(rows, edges):
    """What the counts of .pair_counts() say, per class (rows (..., bins + 2, 3)).  A dict of float64 arrays: r_mid and area
    (bins,) of the caller's annuli; density (..., bins, 3) = pairs of the bin per unit annulus area per pair of the class -- the
    radial pair density a correlation function is formed from (divide by that of an unclustered set); cumulative
    (..., bins + 1, 3) = the fraction of the class's pairs within each edge.  NaN where a class has no pair.  The class totals are
    the sums over all rows: unplaced pairs (a NaN separation) are not among them."""
    r = np.asarray(rows, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    if r.ndim < 2 or r.shape[-1] != NB_PAIRS_COLUMNS or r.shape[-2] != e.shape[0] + 1:
        raise ValueError("rows must have shape (..., len(edges) + 1, 3)")
    area = np.pi * (e[1:] ** 2 - e[:-1] ** 2)
    total = r.sum(axis=-2, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        density = np.where(total > 0, r[..., 1:-1, :] / area[:, None] / total, np.nan)
        cumulative = np.where(total > 0, np.cumsum(r[..., :-1, :], axis=-2) / total, np.nan)
    return {"r_mid": 0.5 * (e[1:] + e[:-1]), "area": area, "density": density, "cumulative": cumulative}


def profile_edges(r_min, r_max, bins, log=False):
    """bins + 1 float32 radii from r_min to r_max, equally spaced in r or, with log, in log r (r_min > 0 then)."""
    if bins < 1 or bins > NB_PROFILE_MAX_BINS:
        raise ValueError(f"bins must be 1 .. {NB_PROFILE_MAX_BINS}")
    if not (0.0 <= r_min < r_max) or (log and not r_min > 0.0):
        raise ValueError("need 0 <= r_min < r_max, and r_min > 0 for logarithmic bins")
    e = (np.geomspace(r_min, r_max, bins + 1) if log else np.linspace(r_min, r_max, bins + 1)).astype(np.float32)
    if not np.all(np.diff(e) > 0):
        raise ValueError("the edges are not strictly increasing in float32: fewer bins or a wider range")
    return e


def profile_curves(rows, edges):
    """What the annulus moments of .profile() say, per bin of `edges` (rows 1 .. bins of rows (..., bins + 2, 6); the rows
    inside edges[0] and beyond edges[-1] only enter `enclosed`).  A dict of float64 arrays (..., bins), NaN where a bin's S is
    0: r_mid, area, surface_density = S / area, enclosed (the cumulative S up to the bin's outer edge, row 0 included),
    r_rms = sqrt(I / S), omega = L / I, v_rot = omega r_rms, expansion = W / I, v_rad = expansion r_rms and
    sigma2 = max(0, K - L^2 / I - W^2 / I) / S (the velocity dispersion, both components together)."""
    r = np.asarray(rows, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    if r.shape[-1:] != (NB_PROFILE_QTY,) or r.ndim < 2 or r.shape[-2] != e.shape[0] + 1:
        raise ValueError("rows must have shape (..., len(edges) + 1, 6)")
    S, I, L, W, K = (r[..., 1:-1, c] for c in range(1, 6))
    area = np.pi * (e[1:] ** 2 - e[:-1] ** 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        empty = S == 0
        nan = lambda a: np.where(empty, np.nan, a)
        r_rms = np.sqrt(I / S)
        omega, expansion = L / I, W / I
        out = {
            "r_mid": 0.5 * (e[1:] + e[:-1]) + np.zeros_like(S),
            "area": area + np.zeros_like(S),
            "surface_density": nan(S / area),
            "enclosed": np.cumsum(r[..., :-1, 1], axis=-1)[..., 1:],
            "r_rms": nan(r_rms),
            "omega": nan(omega),
            "v_rot": nan(omega * r_rms),
            "expansion": nan(expansion),
            "v_rad": nan(expansion * r_rms),
            "sigma2": nan(np.maximum(0.0, K - L * L / I - W * W / I) / S),
        }
    return out


def lagrangian_radii(rows, edges, fractions):
    """The radii that enclose the given fractions of the total S (all rows) of one profile (bins + 2, 6): the enclosed mass
    inverted, the mass of a bin taken as uniform in area, that is linear in r^2.  NaN for a fraction reached inside edges[0]
    or only beyond edges[-1]."""
    r = np.asarray(rows, dtype=np.float64)
    e = np.asarray(edges, dtype=np.float64)
    if r.shape != (e.shape[0] + 1, NB_PROFILE_QTY):
        raise ValueError("rows must have shape (len(edges) + 1, 6)")
    f = np.atleast_1d(np.asarray(fractions, dtype=np.float64))
    at_edge = np.cumsum(r[:-1, 1])          # the S inside edges[t]
    target = f * r[:, 1].sum()
    out = np.full(f.shape, np.nan)
    for i, m in enumerate(target):
        if not (at_edge[0] <= m <= at_edge[-1]) or not np.isfinite(m):
            continue
        t = int(np.searchsorted(at_edge, m, side="left"))       # the first edge with at_edge[t] >= m
        if t == 0 or at_edge[t] == at_edge[t - 1]:
            out[i] = e[t]
            continue
        x = (m - at_edge[t - 1]) / (at_edge[t] - at_edge[t - 1])
        out[i] = np.sqrt(e[t - 1] ** 2 + x * (e[t] ** 2 - e[t - 1] ** 2))
    return out if np.ndim(fractions) else out[0]


def tidal_invariants(t):
    """(trace, lambda_plus, lambda_minus) of tidal tensors t (..., 3) in the order (xx, xy, yy), float64: the in-plane trace
    xx + yy and the eigenvalues trace / 2 +- sqrt(((xx - yy) / 2)^2 + xy^2), lambda_plus >= lambda_minus.  A positive
    eigenvalue stretches a small body along its axis, a negative one compresses it."""
    a = np.asarray(t, dtype=np.float64)
    if a.shape[-1:] != (3,):
        raise ValueError("tidal tensors must have a last axis of 3: (xx, xy, yy)")
    xx, xy, yy = a[..., 0], a[..., 1], a[..., 2]
    trace = xx + yy
    root = np.sqrt(((xx - yy) / 2.0) ** 2 + xy ** 2)
    return trace, trace / 2.0 + root, trace / 2.0 - root


def contact_sheet(frames, columns):
    """(B, h, w, 4) frames -> one (rows * h, columns * w, 4) image, member b in row b // columns, column b % columns;
    cells without a member are zero."""
    frames = np.asarray(frames)
    if frames.ndim != 4 or columns < 1:
        raise ValueError("frames must have shape (B, h, w, channels) and columns must be at least 1")
    count, h, w, ch = frames.shape
    rows = -(-count // columns)
    sheet = np.zeros((rows * columns, h, w, ch), dtype=frames.dtype)
    sheet[:count] = frames
    return sheet.reshape(rows, columns, h, w, ch).transpose(0, 2, 1, 3, 4).reshape(rows * h, columns * w, ch)
