/*
 * nbody_batch_tidal.h -- the tidal tensor of an ensemble of worlds (include/nbody_batch.h) away from its particles: what
 * include/nbody_tidal.h gives for one World, for every member of a WorldBatch at once, at probe points and as maps over
 * views.  The companion of include/nbody_batch_field.h, whose signatures, limits and edge values it follows.
 *
 * Extension (no reference counterpart), implemented in libnbody.so.  The definition is that of include/nbody_tidal.h, member
 * by member: partitioned order, M_b = the member's massive particles, T_ab(p; s) = sum_{j < M_b} G*m_j (3 d_a d_b u_j^5 -
 * delta_ab u_j^3) with d_j = x_j - p and u_j = (|d_j|^2 + s)^(-1/2), three values (xx, xy, yy) per sample, one softening s
 * per call, finite and > 0.
 *
 *   Probes      every member has n of them, 0 <= n: points[count][n], results member-major.  n = 0 does nothing and
 *               touches no device.
 *   Maps        one RenderView per member; all views of a call share width and height (a mismatch aborts, naming the
 *               member), each within the limits of include/nbody_render.h.  A map is exactly the probes product at the
 *               pixel centres of the member's view, row-major.
 *   Limits      count * n and count * width * height are each at most NB_FIELD_MAX_POINTS.
 *   Non-finite  a point with a non-finite coordinate gives three NaN, whatever M_b.
 *   M_b = 0     every value of that member is +0.
 *   Ragged      batches made by CreateWorldBatchRagged (include/nbody_batch_ragged.h) are supported: the members differ in
 *               size, the samples do not -- n probes or one width x height map per member, results [count][n].
 *
 * Where it runs follows GetWorldBatchPotentialAt: when the device has stepped since the host array was last refreshed, all
 * members are computed on the device in ONE launch (nb_hip_ensemble_tidal_at / _tidal_map of nbody_hip.h) WITHOUT reading the
 * particles back, and member b's values are bit-identical to GetWorldTidalAt / RenderWorldTidal of the same world alone on
 * the device, whatever count, its index and the other members are; otherwise each member is computed on the host in float64
 * exactly as those two calls of CreateWorld(member) would.  A WorldBatch that never stepped never opens a device, and the
 * host result does not depend on the OpenMP thread count.  No call changes what GetWorldBatchParticles returns or when it
 * reads the device back.  Failures end in the library's usual "file:line [func] ..." + abort().
 */
#ifndef NBODY_AMD_NBODY_BATCH_TIDAL_H
#define NBODY_AMD_NBODY_BATCH_TIDAL_H

#include "nbody_batch.h"
#include "nbody_field.h"
#include "nbody_tidal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* t[count][n]: T(points[b][i]; softening) of member b; points holds count * n points, member-major. */
void GetWorldBatchTidalAt(WorldBatch *batch, const V2 *points, uint32_t n, float softening, TidalTensor *t);

/* t[count][height][width]: T of member b at every pixel centre of views[b]. */
void RenderWorldBatchTidal(WorldBatch *batch, const RenderView *views, float softening, TidalTensor *t);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_BATCH_TIDAL_H */
