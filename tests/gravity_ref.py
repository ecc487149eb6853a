"""float64 restatement of include/nbody_gravity.h in numpy (TEST INFRASTRUCTURE for test_gravity_cpu.py / test_gpu_gravity.py).

Particles are partitioned (mass > 0 first), m = mass_len.  g(p; s) = sum_{j<m} G*m_j (x_j - p) / (|x_j - p|^2 + s)^(3/2) with
G*m_j the float32 product the step kernels use; no term is excluded.  A point with a non-finite coordinate gives NaN in both
components.  The points, the pixel centres and the augmented world are field_ref's.
"""
import numpy as np

import nbody_amd as nb
from field_ref import augmented, pixel_points, probes  # noqa: F401  (re-exported: one import for the gravity tests)


def g_at_f64(particles, m, points, softening):
    """(g, mag): float64 (n, 2) each, g at the (n, 2) points and the sum of |terms| of each component."""
    a = np.asarray(particles, dtype=np.float32)
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    x, y = a[:m, 0].astype(np.float64), a[:m, 1].astype(np.float64)
    gm = (np.float32(nb.NB_G) * a[:m, 6]).astype(np.float64)          # the float32 product, then widened
    s = np.float64(np.float32(softening))
    g = np.zeros((pts.shape[0], 2), dtype=np.float64)
    mag = np.zeros((pts.shape[0], 2), dtype=np.float64)
    chunk = max(1, (1 << 22) // max(m, 1))   # points per pass: ~4 M pair terms at a time
    for c in range(0, pts.shape[0], chunk):
        px, py = pts[c:c + chunk, 0].astype(np.float64), pts[c:c + chunk, 1].astype(np.float64)
        with np.errstate(invalid="ignore"):
            dx, dy = x[None, :] - px[:, None], y[None, :] - py[:, None]
            q = dx * dx + dy * dy + s
            f = gm[None, :] / (q * np.sqrt(q))
            tx, ty = dx * f, dy * f
            g[c:c + chunk, 0], g[c:c + chunk, 1] = tx.sum(axis=1), ty.sum(axis=1)
            mag[c:c + chunk, 0], mag[c:c + chunk, 1] = np.abs(tx).sum(axis=1), np.abs(ty).sum(axis=1)
    bad = ~np.isfinite(pts).all(axis=1)
    g[bad] = np.nan
    mag[bad] = np.nan
    return g, mag
