/*
 * nbody_batch_render.h -- look at every member of an ensemble of worlds (include/nbody_batch.h) without reading it back:
 * what include/nbody_render.h gives for one World, for all members of a WorldBatch in one call -- a contact sheet of a
 * sweep over seeds or step sizes.
 *
 * Extension (no reference counterpart), implemented in libnbody.so.  The definitions are those of nbody_render.h, member
 * by member, and so is the contract: every product is an integer sum or an integer min / max, so member b's bounds, count
 * image and frame are BIT-IDENTICAL to those of the same world rendered alone, on either side, whatever count is.
 *
 * Where it runs follows GetWorldBatchEnergy: when the device has stepped since the host array was last refreshed, all
 * members are rendered on the device (nb_hip_ensemble_bounds / nb_hip_ensemble_render_counts / nb_hip_ensemble_render_rgba
 * of nbody_hip.h: a constant number of launches, one copy of the images and one sync for any count) WITHOUT reading the
 * particles back; otherwise each member is rendered on the host exactly as CreateWorld(member) would render it.  A
 * WorldBatch that never stepped never opens a device.  No call changes what GetWorldBatchParticles returns or when it
 * reads the device back.
 *
 * Views: one RenderView per member.  All share width and height (a mismatch ends in the library's usual "file:line [func]
 * ..." + abort(), naming the first member that differs), each is within the limits of nbody_render.h, and the images of
 * one call together hold at most 2^24 pixels (count * width * height); saturation >= 1.
 */
#ifndef NBODY_AMD_NBODY_BATCH_RENDER_H
#define NBODY_AMD_NBODY_BATCH_RENDER_H

#include "nbody_batch.h"
#include "nbody_render.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bounds[count][4]: member b's {min.x, min.y, max.x, max.y}. */
void GetWorldBatchBounds(WorldBatch *batch, float *bounds);

/* views[count]: FitWorldView's arithmetic on every member's bounds. */
void FitWorldBatchViews(WorldBatch *batch, uint32_t width, uint32_t height, RenderView *views);

/* counts[count][3][height][width] under views[count]. */
void RenderWorldBatchCounts(WorldBatch *batch, const RenderView *views, uint32_t *counts);

/* rgba[count][height][width][4]; palette may be NULL (DefaultRenderPalette). */
void RenderWorldBatch(WorldBatch *batch, const RenderView *views, const RenderPalette *palette, uint8_t *rgba);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_BATCH_RENDER_H */
