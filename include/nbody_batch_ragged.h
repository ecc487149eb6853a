/*
 * nbody_batch_ragged.h -- an ensemble of worlds (include/nbody_batch.h) whose members differ in size: the same galaxy at
 * N = 200, 400, 800, 1 600 to see whether a result converges, MakeGalaxies worlds of unequal size.  One WorldBatch, one
 * set of launches, instead of one WorldBatch per size stepped one after another.
 *
 * Extension (no reference counterpart), implemented in libnbody.so over nb_hip_ragged_create of nbody_hip.h.  ps is PACKED:
 * member 0's world_size[0] particles, then member 1's, ...; each world_size[b] is 1 .. 3 000, count is 1 .. 65 535 (a
 * violation prints "file:line [func] ... member b ..." and aborts).  The particles are copied and every member is
 * partitioned "mass > 0 first" exactly as CreateWorld partitions it.  The result is a WorldBatch and follows its protocol:
 *   GetWorldBatchParticles           member b's world_size[b] particles, *size = world_size[b]
 *   UpdateWorldBatch_GPU(_dts)       (nbody_batch.h)
 *   UpdateWorldBatch_GPU_Traced(_dts) (nbody_batch_trace.h)
 *   GetWorldBatchEnergy              (nbody_batch_diag.h)
 *   GetWorldBatchPotential           phi is packed like ps: world_size[0] values, then world_size[1], ...
 *   GetWorldBatchPotentialAt, RenderWorldBatchPotential, GetWorldBatchAccelerationAt, RenderWorldBatchAcceleration
 *                                    (nbody_batch_field.h) and GetWorldBatchTidalAt, RenderWorldBatchTidal (nbody_batch_tidal.h):
 *                                    the members differ in size, the samples do not -- results [count][n]
 *   GetWorldBatchProfile             (nbody_batch_profile.h): out [count][bins + 2][6] whatever the sizes
 *   GetWorldBatchPairCounts          (nbody_batch_paircount.h): out [count][bins + 2][3] whatever the sizes
 *   GetWorldBatchNeighbours          (nbody_batch_neighbour.h): packed like the potential
 * Member b's particles, energy, potential and trace rows are bit for bit those of the same particles in a WorldBatch of
 * one member (so a member does not depend on the other members, their sizes or its index).  While the host array is the
 * newest state the diagnostics run on the host, member by member, and need no GPU.
 * Not supported yet: GetWorldBatchBounds, FitWorldBatchViews, RenderWorldBatchCounts and RenderWorldBatch (nbody_batch_render.h)
 * abort on such a batch with a message that says "ragged".
 */
#ifndef NBODY_AMD_NBODY_BATCH_RAGGED_H
#define NBODY_AMD_NBODY_BATCH_RAGGED_H

#include "nbody_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

WorldBatch *CreateWorldBatchRagged(const Particle *ps, const uint32_t *world_size /* [count] */, uint32_t count);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_BATCH_RAGGED_H */
