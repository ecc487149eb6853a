/*
 * nbody_render.h -- look at a World without reading it back: bounds, a per-class count image and an RGBA frame
 * (libnbody.so).  Not part of nbody.h / galaxy.h: the reference has no counterpart (its viewer reads every particle back
 * and draws one circle each).
 *
 * Where it runs: when the device holds the World's newest state, on the GPU (nb_hip_bounds / nb_hip_render_counts /
 * nb_hip_render_rgba of include/nbody_hip.h) and only the result crosses PCIe; otherwise on the host.  A World that only
 * ever steps on the CPU never touches a GPU.  No call changes the World's state or moves a dirty flag.  Sharded Worlds
 * abort (their remote slices are current only inside a step).  A WorldBatch renders all its members at once through
 * include/nbody_batch_render.h.
 *
 * All three products are integer or min / max results, so the contract is BITWISE: the GPU path, the host path and the
 * numpy restatement in tests/render_ref.py give the same bytes for every input, on every call, whatever the particle order.
 *
 * Definitions.  All arithmetic is float32, every operation rounded on its own (no fused multiply-add).
 *
 *   View (RenderView): target[2], offset[2], zoom (the meaning of a 2-D camera without rotation), width, height, core_mass.
 *   Screen position   sx = (x - target[0]) * zoom + offset[0], sy likewise (sub, mul, add).  World coordinates are NOT
 *                     truncated to integers first.
 *   Class             0 = massless (mass <= 0), 1 = ordinary (0 < mass < core_mass), 2 = core (mass >= core_mass).
 *                     FitWorldView fills core_mass with MIN_GC_MASS of include/galaxy.h.
 *   On-screen radius  rho = radius * zoom.  A particle with non-finite sx, sy or rho is dropped.
 *   rho < 1: a POINT. It counts in pixel (px, py) = ((uint32)sx, (uint32)sy) iff sx >= 0 && sx < width && sy >= 0 &&
 *                     sy < height; otherwise nowhere.  (A NaN or negative rho is not >= 1: a negative radius is a point.)
 *   rho >= 1: a DISC. It counts in every pixel of the image with dx = ((float)px + 0.5f) - sx, dy likewise,
 *                     dx*dx + dy*dy <= rho*rho (two products, one add, one product, compare).  A disc whose centre is off
 *                     screen still covers the on-screen pixels that pass the test.  Implementations may use any bounding
 *                     box to find candidates; the test alone decides.
 *   Count image       uint32 counts[3][height][width]: how many particles of each class cover each pixel.
 *   Shade (RenderPalette: background[4], color[3][4], saturation >= 1): per pixel the class shown is the highest class
 *                     with a non-zero count; none => background.  Else t = min(count, saturation) and every channel is
 *                     (background * (saturation - t) + color * t + saturation / 2) / saturation in unsigned 32-bit
 *                     integer arithmetic (wrapping, like uint32_t).  Frame: uint8 rgba[height][width][4].
 *   Bounds            min / max of x and of y over the particles whose x and y are both finite, as {min.x, min.y, max.x,
 *                     max.y}.  Floats are compared in their total order (-0 sorts below +0), so the result does not
 *                     depend on the particle order.  No finite particle: {+inf, +inf, -inf, -inf}.
 *   Limits            width, height >= 1, width * height <= 2^24, zoom finite and > 0, saturation >= 1; a violation ends
 *                     in the library's usual "file:line [func] ..." + abort().  An empty World gives an all-zero count
 *                     image and a background frame.
 *   FitWorldView      from the bounds: zoom = 0.9f * min(width / (max.x - min.x), height / (max.y - min.y)) (an axis of
 *                     zero extent does not constrain; both zero, or no finite particle => zoom = 1), target = 0.5f *
 *                     (min + max) ((0, 0) without a finite particle), offset = (width / 2, height / 2) as floats.  One
 *                     host function computes it from the bounds, whichever side produced them.
 */
#ifndef NBODY_AMD_NBODY_RENDER_H
#define NBODY_AMD_NBODY_RENDER_H

#include <stdint.h>

#include "nbody.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NB_RENDER_CLASSES 3
#define NB_RENDER_MAX_PIXELS (1u << 24)

typedef struct RenderView {
    float target[2];  /* world point shown at `offset` */
    float offset[2];  /* screen position of `target`, in pixels */
    float zoom;       /* pixels per world unit */
    uint32_t width;
    uint32_t height;
    float core_mass;  /* mass >= core_mass: class 2 */
} RenderView;

typedef struct RenderPalette {
    uint8_t background[4];                /* RGBA */
    uint8_t color[NB_RENDER_CLASSES][4];  /* RGBA of a saturated pixel of each class */
    uint32_t saturation;                  /* count at which a pixel reaches its class colour; >= 1 */
} RenderPalette;

/* The palette used when the caller passes NULL: near-black background, slate dust, warm stars, white cores; saturation 8. */
void DefaultRenderPalette(RenderPalette *out);

/* bounds[4] = {min.x, min.y, max.x, max.y} of the World's current state. */
void GetWorldBounds(World *w, float *bounds);

/* Fills *view so that every finite particle is on a width x height screen (definition above). */
void FitWorldView(World *w, uint32_t width, uint32_t height, RenderView *view);

/* counts holds 3 * view->height * view->width uint32. */
void RenderWorldCounts(World *w, const RenderView *view, uint32_t *counts);

/* rgba holds view->height * view->width * 4 bytes; palette may be NULL (DefaultRenderPalette). */
void RenderWorld(World *w, const RenderView *view, const RenderPalette *palette, uint8_t *rgba);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_RENDER_H */
