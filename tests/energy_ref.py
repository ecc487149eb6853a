"""float64 restatement of include/nbody_diag.h in numpy (TEST INFRASTRUCTURE for test_energy_cpu.py / test_gpu_energy.py).

Particles are partitioned (mass > 0 first), M = mass_len.  Phi_i = -sum_{j<M, j!=i} G m_j / sqrt(|x_j - x_i|^2 + r_i);
potential = 1/2 sum_{i<M} m_i Phi_i; kinetic = 1/2 sum m |v|^2; momentum, angular momentum, centre of mass over i < M.
"""
import numpy as np

import nbody_amd as nb


def phi_f64(a, m, idx=None):
    """float64 Phi of the receivers idx (all by default).  Every term has the same sign, so |Phi| = sum of |terms|."""
    a = np.asarray(a, dtype=np.float32)
    chunk = max(1, (1 << 22) // max(m, 1))   # receivers per pass: ~4 M pair terms at a time
    idx = np.arange(a.shape[0]) if idx is None else np.asarray(idx)
    x, y = a[:m, 0].astype(np.float64), a[:m, 1].astype(np.float64)
    gm = np.float64(np.float32(nb.NB_G)) * a[:m, 6].astype(np.float64)
    out = np.zeros(idx.size, dtype=np.float64)
    for c in range(0, idx.size, chunk):
        i = idx[c:c + chunk]
        dx = x[None, :] - a[i, 0].astype(np.float64)[:, None]
        dy = y[None, :] - a[i, 1].astype(np.float64)[:, None]
        with np.errstate(divide="ignore"):
            t = gm[None, :] / np.sqrt(dx * dx + dy * dy + a[i, 7].astype(np.float64)[:, None])
        own = i < m
        t[np.nonzero(own)[0], i[own]] = 0.0          # the self term, by index
        out[c:c + chunk] = -t.sum(axis=1)
    return out


def energy_f64(a, m, phi=None):
    """(dict of the WorldEnergy fields, dict of the sums of |terms| of kinetic / momentum / angular momentum)."""
    a = np.asarray(a, dtype=np.float32)
    f = a[:m].astype(np.float64)
    if phi is None:
        phi = phi_f64(a, m, np.arange(m))
    ms, x, y, vx, vy = f[:, 6], f[:, 0], f[:, 1], f[:, 2], f[:, 3]
    mass = ms.sum()
    lz = ms * (x * vy - y * vx)
    e = {"kinetic": 0.5 * np.sum(ms * (vx * vx + vy * vy)), "potential": 0.5 * np.sum(ms * phi[:m]), "mass": mass,
         "momentum": (np.sum(ms * vx), np.sum(ms * vy)), "angular_momentum": lz.sum(),
         "center_of_mass": (np.sum(ms * x) / mass, np.sum(ms * y) / mass) if mass else (0.0, 0.0)}
    scale = {"kinetic": e["kinetic"], "momentum": (np.sum(np.abs(ms * vx)), np.sum(np.abs(ms * vy))),
             "angular_momentum": np.sum(np.abs(lz))}
    return e, scale


def assert_energy_close(got, want, scale, rel_u=1e-12, rel_k=1e-12):
    """K, momentum, angular momentum within rel_k of the sum of their absolute terms; potential within rel_u relative."""
    assert abs(got["kinetic"] - want["kinetic"]) <= rel_k * scale["kinetic"] + 1e-300, (got, want)
    for c in range(2):
        assert abs(got["momentum"][c] - want["momentum"][c]) <= rel_k * scale["momentum"][c] + 1e-300, (got, want)
    assert abs(got["angular_momentum"] - want["angular_momentum"]) <= rel_k * scale["angular_momentum"] + 1e-300, (got, want)
    assert abs(got["potential"] - want["potential"]) <= rel_u * abs(want["potential"]) + 1e-300, (got, want)
    assert abs(got["mass"] - want["mass"]) <= 1e-12 * abs(want["mass"])
