/*
 * nbody_batch.h -- ensembles of worlds: `count` independent worlds of the same size stepped together on the GPU.
 *
 * Extension (no reference counterpart), implemented in libnbody.so over the nb_hip_batch_* calls of nbody_hip.h.
 * A small world cannot use the chip; many of them can: a WorldBatch steps all its members in one launch per call
 * (world_size <= 512) or one launch per step (512 < world_size <= 3000).  Members never interact, and each member's
 * particles are bit-identical to the same world stepped alone with the ensemble's launch shape, whatever `count` is.
 *
 * Conventions of nbody.h: CreateWorldBatch copies the caller's particles and partitions EACH member "mass > 0 first"
 * with the routine CreateWorld uses, so member b reads back in the order CreateWorld(ps + b * world_size, world_size)
 * would return it; the GPU is first touched by the first update; failures print "file:line [func] ..." and abort().
 * GPU only: there is no CPU stepper for ensembles.
 */
#ifndef NBODY_AMD_NBODY_BATCH_H
#define NBODY_AMD_NBODY_BATCH_H

#include <stdint.h>
#include "nbody.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct WorldBatch WorldBatch;

/* ps: count * world_size particles, member b at [b * world_size, (b + 1) * world_size).  1 <= count <= 65535,
 * 1 <= world_size <= 3000. */
WorldBatch *CreateWorldBatch(const Particle *ps, uint32_t world_size, uint32_t count);

/* NULL is accepted. */
void DestroyWorldBatch(WorldBatch *batch);

/* Member `member` in partitioned order; *size (may be NULL) receives world_size.  Reads the device state back only when
 * it has stepped since the last read.  The pointer stays valid until DestroyWorldBatch. */
const Particle *GetWorldBatchParticles(WorldBatch *batch, uint32_t member, uint32_t *size);

/* n steps of every member; n == 0 does nothing (as UpdateWorld_GPU). */
void UpdateWorldBatch_GPU(WorldBatch *batch, float dt, uint32_t n);

/* The same with member b stepping by dt[b]. */
void UpdateWorldBatch_GPU_dts(WorldBatch *batch, const float *dt, uint32_t n);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_BATCH_H */
