/*
 * nbody_batch_group.h -- the friends-of-friends groups of every member of an ensemble of worlds (include/nbody_batch.h): what
 * include/nbody_group.h gives for one World, for every member of a WorldBatch at once.
 *
 * Extension (no reference counterpart), implemented in libnbody.so.  The statement is that of include/nbody_group.h, member by
 * member with N_b and M_b the member's own counts; a label is the particle's index within its member, so a group never crosses
 * members, however close two members' particles lie.  One spec serves all members: a linking length per member is not built.
 *
 * Ragged batches (include/nbody_batch_ragged.h) are supported: the labels are packed member after member, member b's entries
 * starting at the sum of the sizes before it, as GetWorldBatchNeighbours packs them.
 *
 * Where it runs follows GetWorldBatchNeighbours: when the device has stepped since the host array was last refreshed, all
 * members are answered on the device in ONE sequence of launches (nb_hip_ensemble_groups of nbody_hip.h) without reading the
 * particles back, and member b's entries are those of GetWorldGroups of the same world alone; otherwise each member is answered
 * on the host exactly as GetWorldGroups of CreateWorld(member) would.  A WorldBatch that never stepped never opens a device.
 * No call changes what GetWorldBatchParticles returns or when it reads the device back.  Failures end in the library's usual
 * "file:line [func] ..." + abort().
 */
#ifndef NBODY_AMD_NBODY_BATCH_GROUP_H
#define NBODY_AMD_NBODY_BATCH_GROUP_H

#include "nbody_batch.h"
#include "nbody_group.h"

#ifdef __cplusplus
extern "C" {
#endif

/* group: one label per particle of every member, packed member after member; n_groups (nullable): [count]. */
void GetWorldBatchGroups(WorldBatch *batch, const WorldGroupSpec *spec, uint32_t *group, uint32_t *n_groups /* [count], nullable */);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_BATCH_GROUP_H */
