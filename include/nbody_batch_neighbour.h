/*
 * nbody_batch_neighbour.h -- the nearest neighbour and the neighbour count of every particle of an ensemble of worlds
 * (include/nbody_batch.h): what include/nbody_neighbour.h gives for one World, for every member of a WorldBatch at once.
 *
 * Extension (no reference counterpart), implemented in libnbody.so.  The statement is that of include/nbody_neighbour.h,
 * member by member with N_b and M_b the member's own counts; an index is the particle's index within its member.  One spec
 * serves all members: a radius per member is not built.
 *
 * Ragged batches (include/nbody_batch_ragged.h) are supported: the arrays are packed member after member, member b's entries
 * starting at the sum of the sizes before it, as GetWorldBatchPotential packs them.
 *
 * Where it runs follows GetWorldBatchPairCounts: when the device has stepped since the host array was last refreshed, all
 * members are answered on the device in ONE launch (nb_hip_ensemble_neighbours of nbody_hip.h) without reading the particles
 * back, and member b's entries are those of GetWorldNeighbours of the same world alone; otherwise each member is answered on
 * the host exactly as GetWorldNeighbours of CreateWorld(member) would.  A WorldBatch that never stepped never opens a device.
 * No call changes what GetWorldBatchParticles returns or when it reads the device back.  Failures end in the library's usual
 * "file:line [func] ..." + abort().
 */
#ifndef NBODY_AMD_NBODY_BATCH_NEIGHBOUR_H
#define NBODY_AMD_NBODY_BATCH_NEIGHBOUR_H

#include "nbody_batch.h"
#include "nbody_neighbour.h"

#ifdef __cplusplus
extern "C" {
#endif

/* q, index and count (nullable): one entry per particle of every member, packed member after member. */
void GetWorldBatchNeighbours(WorldBatch *batch, const WorldNeighbourSpec *spec, float *q, uint32_t *index, uint32_t *count);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_BATCH_NEIGHBOUR_H */
