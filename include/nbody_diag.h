/*
 * nbody_diag.h -- conservation diagnostics of a World: energy, momentum and the per-particle potential (libnbody.so).
 *
 * Definitions.  Particles are in the World's partitioned order (mass > 0 first), M = mass_len, and G*m_j is the
 * premultiplied source mass the step kernels use.  Softening is the reference's: the RECEIVER's radius is added to the
 * squared distance, not squared (reference sim_cpu.c:173-176).
 *
 *   Phi_i = - sum_{j < M, j != i} G*m_j / sqrt(|x_j - x_i|^2 + r_i)     for every i < N, massless receivers included,
 *
 * so that a_i = -grad Phi_i with r_i held fixed.  The self term is excluded by index inside the sum (never subtracted
 * afterwards); distinct particles at the same position are included.
 *
 *   potential        = 1/2 sum_{i<M} m_i Phi_i.  With unequal radii this is the average of the two softened pair
 *                      energies of each pair; only with equal radii is it a true pair potential (the softened forces
 *                      here are not exactly antisymmetric, so it is not exactly conserved either).
 *   kinetic          = 1/2 sum_{i<M} m_i |v_i|^2
 *   mass             = sum_{i<M} m_i
 *   momentum         = sum_{i<M} m_i v_i
 *   angular_momentum = sum_{i<M} m_i (x_i v_y,i - y_i v_x,i)          (about the origin)
 *   center_of_mass   = sum_{i<M} m_i x_i / mass                       ((0, 0) when mass == 0)
 *
 * Massless particles (i >= M) carry no mass and add nothing to the sums.  Everything is reduced in float64 from the
 * stored float32 state.  vel is used as stored: the semi-implicit Euler step keeps v half a step ahead of x, so the
 * total energy oscillates by O(dt) around its conserved value; nothing here corrects for it.
 *
 * Where the sums run: when the device holds the World's newest state, on the GPU (nb_hip_energy / nb_hip_potential of
 * include/nbody_hip.h: the potential in fp32 with float64 block totals, the rest in float64) without copying the
 * particle array back; otherwise on the host in float64, independent of the OpenMP thread count.  A World that only
 * ever steps on the CPU never touches a GPU.  Neither call changes the World's state.  Sharded Worlds abort: their
 * remote slices are current only inside a step, so a correct sharded energy needs a collective (not supported).
 *
 * Non-finite state.  Every field of WorldEnergy and every Phi_i has the class (finite, +inf, -inf, NaN) that the float64
 * host path gives for the same state, wherever the sums run and whatever M mod 128 is (the device works in tiles of 128
 * receivers; the idle lanes of the last tile add exact zeros by a select, whatever the particle they read holds): one
 * massive particle with vel.x = +inf makes kinetic, momentum.x and angular_momentum infinite and leaves the other fields
 * finite; a NaN anywhere in a massive particle's position makes every Phi_i NaN; a massless particle, whatever it
 * holds, changes no bit of the energy or of any other particle's Phi.
 */
#ifndef NBODY_AMD_NBODY_DIAG_H
#define NBODY_AMD_NBODY_DIAG_H

#include "nbody.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct WorldEnergy {
    double kinetic;
    double potential;
    double mass;
    double momentum[2];
    double angular_momentum;
    double center_of_mass[2];
} WorldEnergy;

/* Fills *out for the World's current state (definitions above). */
void GetWorldEnergy(World *w, WorldEnergy *out);

/* Writes Phi_i for every particle, in the order GetWorldParticles returns them (phi holds the World's size floats). */
void GetWorldPotential(World *w, float *phi);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_DIAG_H */
