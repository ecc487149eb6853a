/*
 * nbody_gravity.h -- the gravitational acceleration of a World away from its particles: at probe points the caller chooses
 * and as a map over a view (libnbody.so).  Not part of nbody.h / galaxy.h: the reference has no counterpart.  The companion
 * of include/nbody_field.h, which gives the potential at the same places.
 *
 * Definitions.  Particles are in the World's partitioned order (mass > 0 first), M = mass_len, and G*m_j is the
 * premultiplied source mass the step kernels use (the float32 product NB_G * m_j).  For a point p = (x, y) and a
 * softening s
 *
 *   g(p; s) = sum_{j < M} G*m_j (x_j - p) / (|x_j - p|^2 + s)^(3/2)
 *
 * which is what a step stores in Particle.acc for a massless particle of radius s at p: the softening is added to the
 * squared distance, not squared.  No term is excluded -- a probe is never a source -- and a probe that sits exactly on a
 * source gets a zero term from it (x_j - p = 0 over a finite denominator).  g = -grad Phi(p; s) of include/nbody_field.h.
 *
 *   Softening   one scalar per call, finite and > 0; anything else ends in the library's usual "file:line [func] ..." +
 *               abort().
 *   Non-finite  a point with a non-finite coordinate gives NaN in both components, on both paths, whatever M.
 *   M = 0       every g is (+0, +0).
 *   Probes      acc[n] for the caller's points[n], 0 <= n <= 2^24 (NB_FIELD_MAX_POINTS).  n = 0 does nothing and touches no
 *               device.
 *   Map         V2 acc[height][width] under a RenderView (include/nbody_render.h; only target, offset, zoom, width and height
 *               are used; the view's limits are those of a render): g at every pixel centre.  The pixel centres are those of
 *               include/nbody_field.h's map, computed by the same host function whichever side then evaluates g, so the map
 *               is exactly the probes product at those grid points, row-major.
 *
 * Where it runs: when the device holds the World's newest state, on the GPU (nb_hip_acceleration_at /
 * nb_hip_acceleration_map of include/nbody_hip.h: the step kernels' fp32 pair statement with float64 block totals in the
 * summation order of nb_hip_potential, so a result depends on the point and the World alone, not on n, the point's index or
 * the kernel shape) without copying the particle array back; otherwise on the host, every term and both sums in float64 from
 * the stored float32 state and rounded once, independent of the OpenMP thread count.  A World that only ever steps on the
 * CPU never touches a GPU.  Neither call changes the World's state or moves a dirty flag.  Sharded Worlds abort (their
 * remote slices are current only inside a step).
 */
#ifndef NBODY_AMD_NBODY_GRAVITY_H
#define NBODY_AMD_NBODY_GRAVITY_H

#include <stdint.h>

#include "nbody.h"
#include "nbody_field.h"
#include "nbody_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* acc[i] = g(points[i]; softening) for i < n (definitions above). */
void GetWorldAccelerationAt(World *w, const V2 *points, uint32_t n, float softening, V2 *acc);

/* acc holds view->height * view->width V2: g at every pixel centre of the view, row-major. */
void RenderWorldAcceleration(World *w, const RenderView *view, float softening, V2 *acc);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_GRAVITY_H */
