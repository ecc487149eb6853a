/*
 * gravity_cpu.c -- the host path of include/nbody_gravity.h: GetWorldAccelerationAt / RenderWorldAcceleration of a World
 * whose particle array holds the newest state (it only ever stepped on the CPU, or stepped on the CPU last).
 *
 * Same definitions as the GPU path (gravity.hip).  G*m_j is the float32 product the step kernels use; every term and both
 * sums are float64 from the stored float32 state, rounded once (field_cpu.c's convention).  OpenMP splits the samples; each
 * component is one sequential sum over j in index order, so the result does not depend on the thread count.  A map is the
 * probes product at the pixel centres of render_common.h: the same function evaluates both.
 * O(samples * M): fine for checks and small worlds; the GPU path is the one to use for a frame of a large world.
 */
#include <math.h>
#include <stdint.h>

#include "gravity_common.h"
#include "nb_util.h"

static void check_gravity(float softening, uint64_t samples) {
    const char *fault = nb_field_fault(softening, samples);
    NB_CHECK(fault == NULL, "invalid gravity call (softening %g, %llu points): %s", (double)softening, (unsigned long long)samples, fault);
}

/* G*m_j as float64 values of the float32 products, j < mass_len */
static double *source_gm(const Particle *ps, uint32_t mass_len) {
    double *gm = NB_NEW(mass_len ? mass_len : 1, double);
    NB_CHECK(gm != NULL, "Failed to alloc %u source masses", mass_len);
    for (uint32_t j = 0; j < mass_len; j++) {
        const float g = NB_G * ps[j].mass;
        gm[j] = (double)g;
    }
    return gm;
}

static V2 g_at(const Particle *ps, const double *gm, uint32_t mass_len, float x, float y, double s) {
    if (!nb_render_finite(x) || !nb_render_finite(y)) return (V2){NAN, NAN};
    const double px = x, py = y;
    double ax = 0.0, ay = 0.0;
    for (uint32_t j = 0; j < mass_len; j++) {
        const double dx = (double)ps[j].pos.x - px, dy = (double)ps[j].pos.y - py;
        const double q = dx * dx + dy * dy + s;
        const double f = gm[j] / (q * sqrt(q));
        ax += dx * f;
        ay += dy * f;
    }
    return (V2){(float)ax, (float)ay};
}

void nb_cpu_acceleration_at(const Particle *ps, uint32_t mass_len, const V2 *points, uint32_t n, float softening, V2 *acc) {
    check_gravity(softening, n);
    NB_CHECK((points != NULL && acc != NULL) || n == 0, "NULL points or acc");
    if (n == 0) return;
    double *gm = source_gm(ps, mass_len);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; i++) acc[i] = g_at(ps, gm, mass_len, points[i].x, points[i].y, (double)softening);
    free(gm);
}

void nb_cpu_acceleration_map(const Particle *ps, uint32_t mass_len, const RenderView *view, float softening, V2 *acc) {
    NB_CHECK(view != NULL, "NULL RenderView");
    const char *fault = nb_render_view_fault(view);
    NB_CHECK(fault == NULL, "invalid RenderView (%u x %u, zoom %g): %s", view->width, view->height, (double)view->zoom, fault);
    check_gravity(softening, (uint64_t)view->width * view->height);
    NB_CHECK(acc != NULL, "NULL acceleration map");
    const uint32_t width = view->width, height = view->height;
    float *xs = NB_NEW((size_t)width + height, float), *ys = xs + width;
    NB_CHECK(xs != NULL, "Failed to alloc %u + %u pixel coordinates", width, height);
    nb_render_pixel_centres(view, xs, ys);
    double *gm = source_gm(ps, mass_len);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)width * height; i++)
        acc[i] = g_at(ps, gm, mass_len, xs[i % width], ys[i / width], (double)softening);
    free(gm);
    free(xs);
}
