/*
 * nbody_tidal.h -- the tidal tensor of a World away from its particles: at probe points the caller chooses and as a map over
 * a view (libnbody.so).  Not part of nbody.h / galaxy.h: the reference has no counterpart.  The next derivative after
 * include/nbody_field.h (the potential Phi) and include/nbody_gravity.h (the acceleration g = -grad Phi) at the same places.
 *
 * Definitions.  Particles are in the World's partitioned order (mass > 0 first), M = mass_len, and G*m_j is the
 * premultiplied source mass the step kernels use (the float32 product NB_G * m_j).  For a point p = (x, y) and a
 * softening s, with d_j = x_j - p, q_j = |d_j|^2 + s (the softening is added to the squared distance, not squared, as
 * everywhere in the project) and u_j = q_j^(-1/2),
 *
 *   T_ab(p; s) = dg_a/dp_b = sum_{j < M} G*m_j (3 d_a d_b u_j^5 - delta_ab u_j^3)          (= -d2 Phi / dp_a dp_b)
 *
 * Symmetric, so three values per sample, in the order (xx, xy, yy): a massless neighbour displaced by delta from p feels
 * T delta more than p does.  The eigenvalues say where a small body at p is stretched (> 0) or compressed (< 0) and the
 * eigenvectors along which axes.
 *
 *   Trace       the in-plane trace xx + yy = sum G*m_j u_j^5 (|d_j|^2 - 2 s) is NOT zero: the sources are points of a
 *               three-dimensional 1/r potential seen in their plane (the missing zz term is -sum G*m_j u_j^3), and the
 *               softening adds its own part.  It is negative within |d|^2 < 2 s of a lone source and positive outside.
 *   On a source no term is excluded -- a probe is never a source -- and a probe that sits exactly on a source gets the
 *               finite term diag(-G*m_j s^(-3/2)) from it, with xy = +0, on both paths as long as G*m_j s^(-5/2) is a
 *               finite float32 (s > (G*m_j / 2^128)^(2/5); for G*m = 10 that is s >= 2^-49).  Beyond that range the two
 *               paths differ.  The host forms every term in float64 and returns the rounded sum: the finite diagonal
 *               while G*m_j s^(-3/2) is a float32, -inf on the diagonal and +0 beside it below.  The device evaluates
 *               G*m_j u_j^5 in float32; once it overflows, the products with an exactly zero d_a are 0 * inf: a probe on
 *               the source gets three NaN, one within an underflowing distance of it NaN or +-inf components.  The same
 *               holds for any point whose q_j is that small.  In that range the device never returns a finite value
 *               that is wrong: a component is the float64 term within the pair bound or it is not finite
 *               (tests/test_gpu_tidal_pairs.py steps through it).
 *   Softening   one scalar per call, finite and > 0; anything else ends in the library's usual "file:line [func] ..." +
 *               abort().  The pair bound (DESIGN.md section 5 "The tidal pair term") is promised where every float32
 *               intermediate of the statement up to G*m_j u_j^5 and its products with d_a d_b is normal.
 *   Non-finite  a point with a non-finite coordinate gives three NaN, on both paths, whatever M.
 *   M = 0       every T is (+0, +0, +0).
 *   Probes      t[n] for the caller's points[n], 0 <= n <= 2^24 (NB_FIELD_MAX_POINTS).  n = 0 does nothing and touches no
 *               device.
 *   Map         TidalTensor t[height][width] under a RenderView (include/nbody_render.h; only target, offset, zoom, width and
 *               height are used; the view's limits are those of a render): T at every pixel centre.  The pixel centres are
 *               those of include/nbody_field.h's map, computed by the same host function whichever side then evaluates T, so
 *               the map is exactly the probes product at those grid points, row-major.
 *
 * Where it runs follows GetWorldPotentialAt: when the device holds the World's newest state, on the GPU (nb_hip_tidal_at /
 * nb_hip_tidal_map of include/nbody_hip.h: one fp32 pair statement with float64 block totals in the summation order of
 * nb_hip_potential, the factor 3 and the difference of a diagonal component's two parts in float64, so a result depends on
 * the point and the World alone, not on n, the point's index or the kernel shape) without copying the particle array back;
 * otherwise on the host, every term and every sum in float64 from the stored float32 state, in index order and rounded
 * once, independent of the OpenMP thread count.  A World that only ever steps on the CPU never touches a GPU.  Neither call
 * changes the World's state or moves a dirty flag.  Sharded Worlds abort (their remote slices are current only inside a
 * step).
 */
#ifndef NBODY_AMD_NBODY_TIDAL_H
#define NBODY_AMD_NBODY_TIDAL_H

#include <stdint.h>

#include "nbody.h"
#include "nbody_field.h"
#include "nbody_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the symmetric 2 x 2 tensor dg_a/dp_b: xx = dg_x/dx, xy = dg_x/dy = dg_y/dx, yy = dg_y/dy */
typedef struct { float xx, xy, yy; } TidalTensor;

/* t[i] = T(points[i]; softening) for i < n (definitions above). */
void GetWorldTidalAt(World *w, const V2 *points, uint32_t n, float softening, TidalTensor *t);

/* t holds view->height * view->width TidalTensor: T at every pixel centre of the view, row-major. */
void RenderWorldTidal(World *w, const RenderView *view, float softening, TidalTensor *t);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_TIDAL_H */
