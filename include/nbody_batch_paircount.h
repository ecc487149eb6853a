/*
 * nbody_batch_paircount.h -- pair-separation counts of an ensemble of worlds (include/nbody_batch.h): what
 * include/nbody_paircount.h gives for one World, for every member of a WorldBatch at once.
 *
 * Extension (no reference counterpart), implemented in libnbody.so.  The statement, the row rule and the columns are those of
 * include/nbody_paircount.h, member by member with N_b and M_b the member's own counts.  One spec serves all members:
 * per-member edges are not built.
 *
 * Ragged batches (include/nbody_batch_ragged.h) are supported: out is [count][bins + 2][3] whatever the sizes.
 *
 * Where it runs follows GetWorldBatchProfile: when the device has stepped since the host array was last refreshed, all members
 * are counted on the device in ONE launch (nb_hip_ensemble_pair_counts of nbody_hip.h) without reading the particles back, and
 * member b's counts are those of GetWorldPairCounts of the same world alone; otherwise each member is counted on the host
 * exactly as GetWorldPairCounts of CreateWorld(member) would.  A WorldBatch that never stepped never opens a device.  No call
 * changes what GetWorldBatchParticles returns or when it reads the device back.  Failures end in the library's usual
 * "file:line [func] ..." + abort().
 */
#ifndef NBODY_AMD_NBODY_BATCH_PAIRCOUNT_H
#define NBODY_AMD_NBODY_BATCH_PAIRCOUNT_H

#include "nbody_batch.h"
#include "nbody_paircount.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[count][bins + 2][3]; unplaced (nullable) [count][3]. */
void GetWorldBatchPairCounts(WorldBatch *batch, const WorldPairSpec *spec, uint64_t *out, uint64_t *unplaced);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_BATCH_PAIRCOUNT_H */
