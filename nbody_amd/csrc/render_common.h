/*
 * render_common.h -- the arithmetic of include/nbody_render.h written once, for the GPU path (render_kernels.hip) and the host
 * path (render_cpu.c): the screen transform and classification of one particle, the pixel test of a disc, the candidate
 * box of a disc, the shade of one pixel, the total order of floats the bounds use, and the checks of a view and of an ensemble's views.  Both
 * translation units build with -ffp-contract=off, so every float32 operation below is rounded on its own on both sides.
 * The host path's entry points (hidden, libnbody.so) are declared at the bottom.
 */
#ifndef NB_RENDER_COMMON_H
#define NB_RENDER_COMMON_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "nbody_render.h"

#if defined(__HIPCC__)
#define NB_RENDER_HD __host__ __device__ static inline
#else
#define NB_RENDER_HD static inline
#endif

enum { NB_RENDER_DROP = 0, NB_RENDER_POINT = 1, NB_RENDER_DISC = 2 };

typedef struct NbSplat {
    float sx, sy, rho;
    uint32_t cls;
} NbSplat;

NB_RENDER_HD int nb_render_finite(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return (b.u & 0x7f800000u) != 0x7f800000u;
}

/* One particle -> NB_RENDER_DROP / POINT / DISC, its class and screen position. */
NB_RENDER_HD int nb_render_classify(float x, float y, float mass, float radius, float tx, float ty, float ox, float oy,
                                    float zoom, float core_mass, NbSplat *out) {
    const float ax = x - tx, ay = y - ty;
    const float bx = ax * zoom, by = ay * zoom;
    out->sx = bx + ox;
    out->sy = by + oy;
    out->rho = radius * zoom;
    out->cls = mass <= 0.0f ? 0u : (mass < core_mass ? 1u : 2u);
    if (!nb_render_finite(out->sx) || !nb_render_finite(out->sy) || !nb_render_finite(out->rho)) return NB_RENDER_DROP;
    return out->rho >= 1.0f ? NB_RENDER_DISC : NB_RENDER_POINT;
}

/* The pixel a point counts in; 0 when it is off screen. */
NB_RENDER_HD int nb_render_point_pixel(float sx, float sy, uint32_t width, uint32_t height, uint32_t *px, uint32_t *py) {
    if (!(sx >= 0.0f && sx < (float)width && sy >= 0.0f && sy < (float)height)) return 0;
    *px = (uint32_t)sx;
    *py = (uint32_t)sy;
    return 1;
}

/* Does the disc cover pixel (px, py)?  Two products, one add, one product, compare. */
NB_RENDER_HD int nb_render_disc_covers(float sx, float sy, float rho, uint32_t px, uint32_t py) {
    const float dx = ((float)px + 0.5f) - sx, dy = ((float)py + 0.5f) - sy;
    const float xx = dx * dx, yy = dy * dy;
    const float d2 = xx + yy, r2 = rho * rho;
    return d2 <= r2;
}

/*
 * Candidate pixels [lo, hi] of a disc along one axis of `size` pixels; 0 when there is none.  A pixel that passes the
 * float32 test has |exact dx| <= rho * (1 + a few 2^-24), so the box is taken in float64 with a relative margin of 1e-6
 * and one pixel of slack: it can only be too wide, never too narrow.
 */
NB_RENDER_HD int nb_render_disc_span(float s, float rho, uint32_t size, uint32_t *lo, uint32_t *hi) {
    const double reach = (double)rho * 1.000001 + 1.0;
    const double a = floor((double)s - reach), b = ceil((double)s + reach);
    if (b < 0.0 || a > (double)size - 1.0) return 0;
    *lo = a > 0.0 ? (uint32_t)a : 0u;
    *hi = b < (double)size - 1.0 ? (uint32_t)b : size - 1u;
    return 1;
}

/* One pixel's RGBA (packed little-endian: R in the low byte) from its three counts. */
NB_RENDER_HD uint32_t nb_render_shade_pixel(uint32_t c0, uint32_t c1, uint32_t c2, const RenderPalette *p) {
    uint32_t out = 0;
    const int cls = c2 ? 2 : (c1 ? 1 : (c0 ? 0 : -1));
    const uint32_t n = cls == 2 ? c2 : (cls == 1 ? c1 : c0), sat = p->saturation;
    const uint32_t t = n < sat ? n : sat;
    for (int ch = 0; ch < 4; ch++) {
        uint32_t v = p->background[ch];
        if (cls >= 0) v = ((uint32_t)p->background[ch] * (sat - t) + (uint32_t)p->color[cls][ch] * t + sat / 2u) / sat;
        out |= (v & 0xffu) << (8 * ch);
    }
    return out;
}

/* Floats in their total order as unsigned integers: -inf < ... < -0 < +0 < ... < +inf. */
NB_RENDER_HD uint32_t nb_render_order_key(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return (b.u & 0x80000000u) ? ~b.u : (b.u | 0x80000000u);
}

NB_RENDER_HD float nb_render_order_value(uint32_t k) {
    union { float f; uint32_t u; } b;
    b.u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return b.f;
}

#define NB_RENDER_KEY_NONE_MIN 0xffffffffu /* identity of the min over keys */
#define NB_RENDER_KEY_NONE_MAX 0u          /* identity of the max over keys */

/* keys {min.x, min.y, max.x, max.y} -> bounds; no finite particle: {+inf, +inf, -inf, -inf} */
static inline void nb_render_bounds_from_keys(const uint32_t *key, float *bounds) {
    if (key[0] > key[2]) {
        bounds[0] = bounds[1] = INFINITY;
        bounds[2] = bounds[3] = -INFINITY;
        return;
    }
    for (int i = 0; i < 4; i++) bounds[i] = nb_render_order_value(key[i]);
}

/* NULL when the view is within the limits of include/nbody_render.h, else what is wrong with it */
static inline const char *nb_render_view_fault(const RenderView *v) {
    if (v->width < 1u || v->height < 1u) return "width and height must be at least 1";
    if ((uint64_t)v->width * v->height > NB_RENDER_MAX_PIXELS) return "width * height must not exceed 2^24";
    if (!nb_render_finite(v->zoom) || !(v->zoom > 0.0f)) return "zoom must be finite and > 0";
    return NULL;
}

/*
 * World coordinates of the pixel centres of a view (include/nbody_field.h): xs[px] = (((float)px + 0.5f) - offset[0]) / zoom
 * + target[0] for the `width` columns, ys[py] likewise for the `height` rows.  Host only, float32, every operation rounded
 * on its own: whichever side then evaluates a field at the centres starts from these width + height floats.
 */
static inline void nb_render_pixel_centres(const RenderView *v, float *xs, float *ys) {
    for (uint32_t px = 0; px < v->width; px++) {
        const float c = (float)px + 0.5f, d = c - v->offset[0], q = d / v->zoom;
        xs[px] = q + v->target[0];
    }
    for (uint32_t py = 0; py < v->height; py++) {
        const float c = (float)py + 0.5f, d = c - v->offset[1], q = d / v->zoom;
        ys[py] = q + v->target[1];
    }
}

/*
 * The views of one ensemble render (one per member): NULL when each is valid, all share width and height and the `count`
 * images together hold at most 2^24 pixels; else what is wrong, with *member = the first member at fault.
 */
static inline const char *nb_render_views_fault(const RenderView *views, uint32_t count, uint32_t *member) {
    for (uint32_t b = 0; b < count; b++) {
        *member = b;
        const char *fault = nb_render_view_fault(&views[b]);
        if (fault) return fault;
        if (views[b].width != views[0].width || views[b].height != views[0].height)
            return "width and height differ from member 0's: the views of one call share one size";
    }
    *member = 0;
    if ((uint64_t)count * views[0].width * views[0].height > NB_RENDER_MAX_PIXELS) return "count * width * height must not exceed 2^24";
    return NULL;
}

#ifdef __cplusplus
extern "C" {
#endif

/* render_cpu.c (libnbody.so, not exported) */
__attribute__((visibility("hidden"))) void nb_cpu_bounds(const Particle *ps, uint32_t n, float *bounds);
__attribute__((visibility("hidden"))) void nb_cpu_render_counts(const Particle *ps, uint32_t n, const RenderView *view,
                                                                uint32_t *counts);
__attribute__((visibility("hidden"))) void nb_cpu_render_rgba(const Particle *ps, uint32_t n, const RenderView *view,
                                                              const RenderPalette *palette, uint8_t *rgba);
__attribute__((visibility("hidden"))) void nb_fit_view(const float *bounds, uint32_t width, uint32_t height, RenderView *view);

#ifdef __cplusplus
}
#endif

#endif /* NB_RENDER_COMMON_H */
