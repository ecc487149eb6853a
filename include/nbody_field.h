/*
 * nbody_field.h -- the gravitational potential of a World away from its particles: at probe points the caller chooses and
 * as a map over a view (libnbody.so).  Not part of nbody.h / galaxy.h: the reference has no counterpart.
 *
 * Definitions.  Particles are in the World's partitioned order (mass > 0 first), M = mass_len, and G*m_j is the
 * premultiplied source mass the step kernels use (the float32 product NB_G * m_j).  For a point p = (x, y) and a
 * softening s
 *
 *   Phi(p; s) = - sum_{j < M} G*m_j / sqrt(|x_j - p|^2 + s)
 *
 * which is include/nbody_diag.h's Phi_i for a massless receiver at p whose radius is s: the softening is added to the
 * squared distance, not squared.  No term is excluded -- a probe is never a source -- so a probe that sits exactly on a
 * source gives a finite value (that source's term is -G*m_j / sqrt(s)).
 *
 *   Softening   one scalar per call, finite and > 0; anything else ends in the library's usual "file:line [func] ..." +
 *               abort().
 *   Non-finite  a point with a non-finite coordinate gives NaN, on both paths, whatever M.
 *   M = 0       every Phi is 0.
 *   Probes      phi[n] for the caller's points[n], 0 <= n <= 2^24.  n = 0 does nothing and touches no device.
 *   Map         float32 phi[height][width] under a RenderView (include/nbody_render.h; only target, offset, zoom, width and
 *               height are used; the view's limits are those of a render): Phi at every pixel centre.  The world coordinate
 *               of pixel column px is (((float)px + 0.5f) - offset[0]) / zoom + target[0], rows likewise from offset[1] and
 *               target[1], in float32 with every operation rounded on its own.  One host function computes the `width`
 *               column and the `height` row coordinates, whichever side then evaluates Phi, so the map is exactly the
 *               probes product at those grid points, row-major.
 *
 * Where it runs: when the device holds the World's newest state, on the GPU (nb_hip_potential_at / nb_hip_potential_map of
 * include/nbody_hip.h: fp32 pairs with float64 block totals, the arithmetic and the summation order of nb_hip_potential,
 * so Phi at a probe has the bits nb_hip_potential gives a massless particle of radius s at the same place) without copying
 * the particle array back; otherwise on the host, every term and the sum in float64 from the stored float32 state and
 * rounded once, independent of the OpenMP thread count.  A World that only ever steps on the CPU never touches a GPU.
 * Neither call changes the World's state or moves a dirty flag.  Sharded Worlds abort (their remote slices are current
 * only inside a step).
 */
#ifndef NBODY_AMD_NBODY_FIELD_H
#define NBODY_AMD_NBODY_FIELD_H

#include <stdint.h>

#include "nbody.h"
#include "nbody_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NB_FIELD_MAX_POINTS (1u << 24)

/* phi[i] = Phi(points[i]; softening) for i < n (definitions above). */
void GetWorldPotentialAt(World *w, const V2 *points, uint32_t n, float softening, float *phi);

/* phi holds view->height * view->width floats: Phi at every pixel centre of the view, row-major. */
void RenderWorldPotential(World *w, const RenderView *view, float softening, float *phi);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_FIELD_H */
