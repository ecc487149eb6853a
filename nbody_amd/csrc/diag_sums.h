/*
 * diag_sums.h -- the last step of an energy diagnostic, shared by the GPU path (diagnostics.hip) and the host path
 * (diag_cpu.c): the eight float64 sums over the massive particles -> WorldEnergy (include/nbody_diag.h); and the
 * host path's entry points, which world.c calls when the host array holds the newest state.
 *   q[0] sum m_i Phi_i      q[1] sum m_i |v_i|^2      q[2] sum m_i
 *   q[3] sum m_i v_x,i      q[4] sum m_i v_y,i        q[5] sum m_i (x_i v_y,i - y_i v_x,i)
 *   q[6] sum m_i x_i        q[7] sum m_i y_i
 */
#ifndef NB_DIAG_SUMS_H
#define NB_DIAG_SUMS_H

#include "nbody_diag.h"

#define NB_DIAG_SUMS 8

static inline void nb_energy_from_sums(const double *q, WorldEnergy *out) {
    out->potential = 0.5 * q[0];
    out->kinetic = 0.5 * q[1];
    out->mass = q[2];
    out->momentum[0] = q[3];
    out->momentum[1] = q[4];
    out->angular_momentum = q[5];
    out->center_of_mass[0] = q[2] != 0.0 ? q[6] / q[2] : 0.0;
    out->center_of_mass[1] = q[2] != 0.0 ? q[7] / q[2] : 0.0;
}

#ifdef __cplusplus
extern "C" {
#endif

/* diag_cpu.c (libnbody.so, not exported): float64 on the host, OpenMP over receivers, every sum in index order */
__attribute__((visibility("hidden"))) void nb_cpu_energy(const Particle *ps, uint32_t total_len, uint32_t mass_len,
                                                         WorldEnergy *out);
__attribute__((visibility("hidden"))) void nb_cpu_potential(const Particle *ps, uint32_t total_len, uint32_t mass_len,
                                                            float *phi);

#ifdef __cplusplus
}
#endif

#endif /* NB_DIAG_SUMS_H */
