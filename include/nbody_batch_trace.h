/*
 * nbody_batch_trace.h -- traced updates of an ensemble of worlds (include/nbody_batch.h): the steps of
 * UpdateWorldBatch_GPU(_dts) with every member's WorldEnergy (include/nbody_diag.h) recorded every `every` >= 1 steps, in
 * one call.  What a sweep over step sizes or seeds compares is the drift of the energy over time; this replaces the host
 * loop of UpdateWorldBatch_GPU + GetWorldBatchEnergy (include/nbody_batch_diag.h) and its round trip per sample.
 *
 * Extension (no reference counterpart), implemented in libnbody.so over nb_hip_ensemble_trace of nbody_hip.h.  out is
 * WorldEnergy[1 + n / every][count], record-major: row 0 is the state on entry, row r the state after r * every steps, the
 * trailing n mod every steps run unrecorded.  Every row is the device's value -- the bits GetWorldBatchEnergy gives once
 * the device has stepped -- also on the first call, which uploads the array like an update does; afterwards the device
 * holds the newest state (n = 0: one row, and nothing has changed).  every = 0 and NULL arguments abort; there is no CPU
 * path.
 */
#ifndef NBODY_AMD_NBODY_BATCH_TRACE_H
#define NBODY_AMD_NBODY_BATCH_TRACE_H

#include "nbody_batch.h"
#include "nbody_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

void UpdateWorldBatch_GPU_Traced(WorldBatch *batch, float dt, uint32_t n, uint32_t every, WorldEnergy *out);
void UpdateWorldBatch_GPU_Traced_dts(WorldBatch *batch, const float *dt /* [count] */, uint32_t n, uint32_t every, WorldEnergy *out);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_BATCH_TRACE_H */
