/*
 * render_cpu.c -- the host path of include/nbody_render.h: bounds, count image and RGBA frame of a World whose particle
 * array holds the newest state (it only ever stepped on the CPU, or stepped on the CPU last), and FitWorldView's
 * arithmetic, which both paths share.
 *
 * Same definitions and the same inline arithmetic as the GPU path (render_common.h), built with -ffp-contract=off.
 * OpenMP splits the particles; every contribution is an integer increment of the count image (an atomic update) or an
 * integer min / max, so the result does not depend on the thread count or on the particle order.
 */
#include <stddef.h>

#include "render_common.h"

#include "galaxy.h"
#include "nb_util.h"

static void check_view(const RenderView *view) {
    NB_CHECK(view != NULL, "NULL RenderView");
    const char *fault = nb_render_view_fault(view);
    NB_CHECK(fault == NULL, "invalid RenderView (%u x %u, zoom %g): %s", view->width, view->height, (double)view->zoom, fault);
}

void nb_cpu_bounds(const Particle *ps, uint32_t n, float *bounds) {
    uint32_t lo_x = NB_RENDER_KEY_NONE_MIN, lo_y = NB_RENDER_KEY_NONE_MIN;
    uint32_t hi_x = NB_RENDER_KEY_NONE_MAX, hi_y = NB_RENDER_KEY_NONE_MAX;
#pragma omp parallel for schedule(static) reduction(min : lo_x, lo_y) reduction(max : hi_x, hi_y)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const float x = ps[i].pos.x, y = ps[i].pos.y;
        if (!nb_render_finite(x) || !nb_render_finite(y)) continue;
        const uint32_t kx = nb_render_order_key(x), ky = nb_render_order_key(y);
        lo_x = kx < lo_x ? kx : lo_x;
        hi_x = kx > hi_x ? kx : hi_x;
        lo_y = ky < lo_y ? ky : lo_y;
        hi_y = ky > hi_y ? ky : hi_y;
    }
    const uint32_t key[4] = {lo_x, lo_y, hi_x, hi_y};
    nb_render_bounds_from_keys(key, bounds);
}

void nb_fit_view(const float *bounds, uint32_t width, uint32_t height, RenderView *view) {
    NB_CHECK(view != NULL, "NULL RenderView");
    NB_CHECK(width >= 1u && height >= 1u && (uint64_t)width * height <= NB_RENDER_MAX_PIXELS,
             "invalid screen %u x %u: at least 1 x 1, at most 2^24 pixels", width, height);
    const float w = (float)width, h = (float)height;
    view->width = width;
    view->height = height;
    view->offset[0] = w * 0.5f;
    view->offset[1] = h * 0.5f;
    view->core_mass = MIN_GC_MASS;
    view->target[0] = view->target[1] = 0.0f;
    view->zoom = 1.0f;
    if (bounds[0] > bounds[2]) return;   /* no finite particle */
    view->target[0] = 0.5f * (bounds[0] + bounds[2]);
    view->target[1] = 0.5f * (bounds[1] + bounds[3]);
    const float ex = bounds[2] - bounds[0], ey = bounds[3] - bounds[1];
    if (ex > 0.0f && ey > 0.0f) {
        const float zx = w / ex, zy = h / ey;
        view->zoom = 0.9f * (zx < zy ? zx : zy);
    } else if (ex > 0.0f) {
        view->zoom = 0.9f * (w / ex);
    } else if (ey > 0.0f) {
        view->zoom = 0.9f * (h / ey);
    }
}

void nb_cpu_render_counts(const Particle *ps, uint32_t n, const RenderView *view, uint32_t *counts) {
    check_view(view);
    NB_CHECK(counts != NULL, "NULL count image");
    const uint32_t width = view->width, height = view->height;
    const size_t plane = (size_t)width * height;
    memset(counts, 0, plane * NB_RENDER_CLASSES * sizeof(uint32_t));
#pragma omp parallel for schedule(dynamic, 4096)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        NbSplat s;
        const int kind = nb_render_classify(ps[i].pos.x, ps[i].pos.y, ps[i].mass, ps[i].radius, view->target[0], view->target[1],
                                            view->offset[0], view->offset[1], view->zoom, view->core_mass, &s);
        uint32_t *img = counts + plane * s.cls;
        if (kind == NB_RENDER_POINT) {
            uint32_t px, py;
            if (!nb_render_point_pixel(s.sx, s.sy, width, height, &px, &py)) continue;
#pragma omp atomic update
            img[(size_t)py * width + px] += 1u;
        } else if (kind == NB_RENDER_DISC) {
            uint32_t x0, x1, y0, y1;
            if (!nb_render_disc_span(s.sx, s.rho, width, &x0, &x1) || !nb_render_disc_span(s.sy, s.rho, height, &y0, &y1)) continue;
            for (uint32_t py = y0; py <= y1; py++)
                for (uint32_t px = x0; px <= x1; px++)
                    if (nb_render_disc_covers(s.sx, s.sy, s.rho, px, py)) {
#pragma omp atomic update
                        img[(size_t)py * width + px] += 1u;
                    }
        }
    }
}

void nb_cpu_render_rgba(const Particle *ps, uint32_t n, const RenderView *view, const RenderPalette *palette, uint8_t *rgba) {
    check_view(view);
    NB_CHECK(rgba != NULL, "NULL frame");
    RenderPalette pal;
    if (palette)
        pal = *palette;
    else
        DefaultRenderPalette(&pal);
    NB_CHECK(pal.saturation >= 1u, "RenderPalette saturation must be at least 1");
    const size_t plane = (size_t)view->width * view->height;
    uint32_t *counts = NB_NEW(plane * NB_RENDER_CLASSES, uint32_t);
    NB_CHECK(counts != NULL, "Failed to alloc a %u x %u count image", view->width, view->height);
    nb_cpu_render_counts(ps, n, view, counts);
#pragma omp parallel for schedule(static)
    for (int64_t p = 0; p < (int64_t)plane; p++) {
        const uint32_t v = nb_render_shade_pixel(counts[p], counts[plane + p], counts[2 * plane + p], &pal);
        rgba[4 * p + 0] = (uint8_t)(v & 0xffu);
        rgba[4 * p + 1] = (uint8_t)((v >> 8) & 0xffu);
        rgba[4 * p + 2] = (uint8_t)((v >> 16) & 0xffu);
        rgba[4 * p + 3] = (uint8_t)(v >> 24);
    }
    free(counts);
}

void DefaultRenderPalette(RenderPalette *out) {
    NB_CHECK(out != NULL, "NULL RenderPalette");
    const RenderPalette p = {.background = {6, 8, 16, 255},
                             .color = {{96, 120, 168, 255}, {255, 214, 150, 255}, {255, 255, 255, 255}},
                             .saturation = 8u};
    *out = p;
}
