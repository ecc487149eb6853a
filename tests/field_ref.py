"""float64 restatement of include/nbody_field.h in numpy (TEST INFRASTRUCTURE for test_field_cpu.py / test_gpu_field.py).

Particles are partitioned (mass > 0 first), m = mass_len.  Phi(p; s) = -sum_{j<m} G*m_j / sqrt(|x_j - p|^2 + s) with G*m_j
the float32 product the step kernels use; no term is excluded.  A point with a non-finite coordinate gives NaN.
"""
import numpy as np

import nbody_amd as nb


def phi_at_f64(particles, m, points, softening):
    """float64 Phi at the (n, 2) points.  Every term has the same sign, so |Phi| = the sum of |terms|."""
    a = np.asarray(particles, dtype=np.float32)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    x, y = a[:m, 0].astype(np.float64), a[:m, 1].astype(np.float64)
    gm = (np.float32(nb.NB_G) * a[:m, 6]).astype(np.float64)          # the float32 product, then widened
    s = np.float64(np.float32(softening))
    out = np.zeros(pts.shape[0], dtype=np.float64)
    chunk = max(1, (1 << 22) // max(m, 1))   # points per pass: ~4 M pair terms at a time
    for c in range(0, pts.shape[0], chunk):
        px, py = pts[c:c + chunk, 0].astype(np.float64), pts[c:c + chunk, 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            dx, dy = x[None, :] - px[:, None], y[None, :] - py[:, None]
            out[c:c + chunk] = -(gm[None, :] / np.sqrt(dx * dx + dy * dy + s)).sum(axis=1)
    out[~np.isfinite(pts).all(axis=1)] = np.nan
    return out


def pixel_points(view):
    """The float32 pixel centres of a view, row-major (height * width, 2): x of column px = (((float)px + 0.5f) - offset[0])
    / zoom + target[0], rows likewise; every operation rounded to float32 on its own."""
    f = np.float32
    xs = ((np.arange(view.width, dtype=np.float32) + f(0.5)) - f(view.offset[0])) / f(view.zoom) + f(view.target[0])
    ys = ((np.arange(view.height, dtype=np.float32) + f(0.5)) - f(view.offset[1])) / f(view.zoom) + f(view.target[1])
    assert xs.dtype == np.float32 and ys.dtype == np.float32
    pts = np.empty((view.height, view.width, 2), dtype=np.float32)
    pts[:, :, 0] = xs[None, :]
    pts[:, :, 1] = ys[:, None]
    return pts.reshape(-1, 2)


def probes(part, n, seed):
    """n probe points spread over the particles' extent (and a little beyond), float32 (n, 2)."""
    rng = np.random.default_rng(seed)
    fin = part[np.isfinite(part[:, 0:2]).all(axis=1), 0:2].astype(np.float64) if part.shape[0] else np.zeros((0, 2))
    lo, hi = (fin.min(axis=0), fin.max(axis=0)) if fin.shape[0] else (np.array([-1.0, -1.0]), np.array([1.0, 1.0]))
    span = np.maximum(hi - lo, 1.0)
    return (lo - 0.1 * span + rng.random((n, 2)) * 1.2 * span).astype(np.float32)


def augmented(part, points, softening):
    """The particles plus one massless particle of radius `softening` per point, appended: still partitioned."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    extra = np.zeros((pts.shape[0], 8), dtype=np.float32)
    extra[:, 0:2] = pts
    extra[:, 7] = np.float32(softening)
    return np.concatenate([np.asarray(part, dtype=np.float32), extra], axis=0)
