/*
 * nbody_profile.h -- radial profiles of a World: the moments of its particles in annuli about a centre (libnbody.so).  Not
 * part of nbody.h / galaxy.h: the reference has no counterpart.  From the six sums of an annulus follow its surface density,
 * the enclosed mass and the Lagrangian radii, the rotation curve, the radial flow and the velocity dispersion, without a
 * division per particle (the helpers that do so are numpy: nbody_amd.profile_curves, nbody_amd.lagrangian_radii).
 *
 * Definitions.  Particles are in the World's partitioned order (mass > 0 first), N = total_len, M = mass_len.
 *
 *   edges     bins + 1 float32 radii, finite, edges[0] >= 0, strictly increasing, 1 <= bins <= NB_PROFILE_MAX_BINS (254)
 *   centre    (cx, cy) and a centre velocity (ux, uy), four finite float32
 *   weights   NB_PROFILE_BY_MASS    particles i < M with weight wgt = m_i (the default)
 *             NB_PROFILE_BY_NUMBER  all N particles with weight wgt = 1 (massless tracer discs)
 *             In mass mode a massless particle is never read: whatever it holds changes no bit.
 *
 * Per particle, everything in float64 formed from the stored float32 values, every operation rounded on its own, only
 * + - * (no divide, no sqrt), so the device, the host and a numpy restatement agree bit for bit:
 *
 *   dx = (double)x - cx      dy = (double)y - cy      vx' = (double)vx - ux      vy' = (double)vy - uy
 *   q = dx*dx + dy*dy                     the squared radius
 *   j = dx*vy' - dy*vx'                   the specific angular momentum about the centre
 *   w = dx*vx' + dy*vy'                   R times the radial velocity
 *   k = vx'*vx' + vy'*vy'
 *
 * Row of a particle.  e2[t] = (double)edges[t] * (double)edges[t] (exact, still strictly increasing); rows = bins + 2:
 *
 *   row 0            q < e2[0]
 *   row t            e2[t-1] <= q < e2[t]           for 1 <= t <= bins: bin t - 1 of the caller's edges
 *   row bins + 1     q >= e2[bins]                  (+inf included)
 *
 * A NaN q is placed in no row; such particles are counted in `unplaced` (nullable, one value per world).
 *
 * Output: float64 out[rows][NB_PROFILE_QTY = 6], the columns of a row being
 *
 *   0  count (exact)     1  S = sum wgt     2  I = sum wgt q     3  L = sum wgt j     4  W = sum wgt w     5  K = sum wgt k
 *
 * with each product rounded before it is added.  In two dimensions q k = j^2 + w^2 per particle, so L / I is the angular
 * velocity of the annulus (its angular momentum over its moment of inertia), W / I its expansion rate, and
 * K - L^2 / I - W^2 / I >= 0 the kinetic energy that is neither rigid rotation nor homologous expansion: the dispersion.
 *
 * Summation order -- the contract, as for the other diagnostics.  Particles are taken in stored order in chunks of
 * NB_PROFILE_CHUNK = 1024 consecutive particles.  Inside a chunk each row's terms are added in index order, starting from
 * +0.0; every chunk's total is then added in chunk order, starting from +0.0, a row the chunk left empty adding +0.0.  No
 * float atomics: the result does not depend on the launch shape, the CU count or the call history.  Non-finite velocities of
 * a placed particle simply propagate through these sums, so host and device agree in class by construction.
 *
 * vel is used as stored: the semi-implicit Euler step keeps v half a step ahead of x (the caveat of include/nbody_diag.h).
 * A natural centre is GetWorldEnergy's center_of_mass with momentum / mass as the centre velocity.
 *
 * Where it runs follows GetWorldEnergy: when the device holds the World's newest state, on the GPU (nb_hip_profile of
 * include/nbody_hip.h) without copying the particle array back; otherwise on the host, the same statement in the same order.
 * A World that only ever steps on the CPU never touches a GPU.  The call changes neither the World's state nor a dirty flag.
 * Sharded Worlds abort.  Every fault of the arguments ends in the library's usual "file:line [func] ..." + abort().
 */
#ifndef NBODY_AMD_NBODY_PROFILE_H
#define NBODY_AMD_NBODY_PROFILE_H

#include <stdint.h>

#include "nbody.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NB_PROFILE_MAX_BINS 254u
#define NB_PROFILE_QTY 6u
#define NB_PROFILE_CHUNK 1024u

enum { NB_PROFILE_BY_MASS = 0, NB_PROFILE_BY_NUMBER = 1 };

typedef struct WorldProfileSpec {
    const float *edges;        /* bins + 1 radii */
    uint32_t bins;
    float centre[2];           /* (cx, cy) */
    float centre_velocity[2];  /* (ux, uy) */
    int weights;               /* NB_PROFILE_BY_MASS / NB_PROFILE_BY_NUMBER */
} WorldProfileSpec;

/* out holds (spec->bins + 2) * NB_PROFILE_QTY doubles; unplaced (nullable) gets the number of particles with a NaN q. */
void GetWorldProfile(World *w, const WorldProfileSpec *spec, double *out, uint32_t *unplaced);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_PROFILE_H */
