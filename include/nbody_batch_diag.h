/*
 * nbody_batch_diag.h -- conservation diagnostics of an ensemble of worlds (include/nbody_batch.h): what
 * include/nbody_diag.h gives for one World, for every member of a WorldBatch at once.
 *
 * Extension (no reference counterpart), implemented in libnbody.so.  The definitions are those of nbody_diag.h, member
 * by member: partitioned order, M_b = the member's massive particles, the receiver's radius added to the squared
 * distance, the self term excluded by index, float64 reductions in a fixed order.
 *
 * Where it runs follows GetWorldEnergy: when the device has stepped since the host array was last refreshed, all members
 * are computed on the device in one pass (nb_hip_ensemble_energy / nb_hip_ensemble_potential of nbody_hip.h: two launches
 * and 64 * count bytes for the energies) WITHOUT reading the particles back; otherwise each member is computed on the host
 * in float64 exactly as GetWorldEnergy / GetWorldPotential of CreateWorld(member) would.  A WorldBatch that never stepped
 * never opens a device, and the host result does not depend on the OpenMP thread count.  On the device member b's result
 * is bit-identical to the same world alone (nb_hip_energy of a pipeline holding the same particles), whatever count is.
 * Neither call changes what GetWorldBatchParticles returns or when it reads the device back.
 */
#ifndef NBODY_AMD_NBODY_BATCH_DIAG_H
#define NBODY_AMD_NBODY_BATCH_DIAG_H

#include "nbody_batch.h"
#include "nbody_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[count]: member b's energy, momentum, angular momentum and centre of mass. */
void GetWorldBatchEnergy(WorldBatch *batch, WorldEnergy *out);

/* phi[count * world_size], member-major: Phi_i of every particle, massless ones included, in partitioned order. */
void GetWorldBatchPotential(WorldBatch *batch, float *phi);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_BATCH_DIAG_H */
