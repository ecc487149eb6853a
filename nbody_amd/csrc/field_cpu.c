/*
 * field_cpu.c -- the host path of include/nbody_field.h, include/nbody_gravity.h and include/nbody_tidal.h:
 * GetWorldPotentialAt / RenderWorldPotential, GetWorldAccelerationAt / RenderWorldAcceleration and GetWorldTidalAt /
 * RenderWorldTidal of a World whose particle array holds the newest state (it only ever stepped on the CPU, or stepped on
 * the CPU last).
 *
 * Same definitions as the GPU path (field.hip).  G*m_j is the float32 product the step kernels use; every term and every
 * sum are float64 from the stored float32 state, rounded once (diag_cpu.c's convention for the per-particle Phi).  OpenMP
 * splits the samples; every Phi and every component of g and of T is one sequential sum over j in index order, so the
 * result does not depend on the thread count.  A map is the probes product at the pixel centres of render_common.h: the same function
 * evaluates both.
 * O(samples * M): fine for checks and small worlds; the GPU path is the one to use for a frame of a large world.
 */
#include <math.h>
#include <stdint.h>

#include "field_common.h"
#include "nb_util.h"

static float phi_at(const Particle *ps, const double *gm, uint32_t mass_len, float x, float y, double s) {
    if (!nb_render_finite(x) || !nb_render_finite(y)) return NAN;
    const double px = x, py = y;
    double sum = 0.0;
    for (uint32_t j = 0; j < mass_len; j++) {
        const double dx = (double)ps[j].pos.x - px, dy = (double)ps[j].pos.y - py;
        sum += gm[j] / sqrt(dx * dx + dy * dy + s);
    }
    return (float)-sum;
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

/* T = dg/dp: (xx, xy, yy) = sum G*m_j (3 d_a d_b u^5 - delta_ab u^3), u = q^(-1/2); a point on a source gets its
 * finite term diag(-G*m s^(-3/2)) */
static TidalTensor t_at(const Particle *ps, const double *gm, uint32_t mass_len, float x, float y, double s) {
    if (!nb_render_finite(x) || !nb_render_finite(y)) return (TidalTensor){NAN, NAN, NAN};
    const double px = x, py = y;
    double xx = 0.0, xy = 0.0, yy = 0.0;
    for (uint32_t j = 0; j < mass_len; j++) {
        const double dx = (double)ps[j].pos.x - px, dy = (double)ps[j].pos.y - py;
        const double q = dx * dx + dy * dy + s;
        const double u3 = gm[j] / (q * sqrt(q)), u5x3 = 3.0 * u3 / q;   /* G*m u^3 and 3 G*m u^5 */
        xx += dx * dx * u5x3 - u3;
        xy += dx * dy * u5x3;
        yy += dy * dy * u5x3 - u3;
    }
    return (TidalTensor){(float)xx, (float)xy, (float)yy};
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

/*
 * The one driver behind the six entry points: n samples into phi[] (the potential) or, where phi is NULL, into acc[] or,
 * where both are NULL, into tid[].
 * Probes: sample i is points[i].  A map (points NULL): sample i is pixel (i % width, i / width) at (xs[i % width], ys[i / width]).
 */
static void sample(const char *noun, const Particle *ps, uint32_t mass_len, const V2 *points, const float *xs, const float *ys,
                   uint32_t width, uint64_t n, float softening, float *phi, V2 *acc, TidalTensor *tid) {
    const char *fault = nb_field_fault(softening, n);
    NB_CHECK(fault == NULL, "invalid %s call (softening %g, %llu points): %s", noun, (double)softening, (unsigned long long)n, fault);
    NB_CHECK(((points != NULL || xs != NULL) && (phi != NULL || acc != NULL || tid != NULL)) || n == 0, "NULL %s points or result", noun);
    if (n == 0) return;
    double *gm = source_gm(ps, mass_len);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)n; i++) {
        const float x = points ? points[i].x : xs[i % width], y = points ? points[i].y : ys[i / width];
        if (phi)
            phi[i] = phi_at(ps, gm, mass_len, x, y, (double)softening);
        else if (acc)
            acc[i] = g_at(ps, gm, mass_len, x, y, (double)softening);
        else
            tid[i] = t_at(ps, gm, mass_len, x, y, (double)softening);
    }
    free(gm);
}

static void sample_map(const char *noun, const Particle *ps, uint32_t mass_len, const RenderView *view, float softening, float *phi,
                       V2 *acc, TidalTensor *tid) {
    NB_CHECK(view != NULL, "NULL RenderView");
    const char *fault = nb_render_view_fault(view);
    NB_CHECK(fault == NULL, "invalid RenderView (%u x %u, zoom %g): %s", view->width, view->height, (double)view->zoom, fault);
    const uint32_t width = view->width, height = view->height;
    float *xs = NB_NEW((size_t)width + height, float), *ys = xs + width;
    NB_CHECK(xs != NULL, "Failed to alloc %u + %u pixel coordinates", width, height);
    nb_render_pixel_centres(view, xs, ys);
    sample(noun, ps, mass_len, NULL, xs, ys, width, (uint64_t)width * height, softening, phi, acc, tid);
    free(xs);
}

void nb_cpu_potential_at(const Particle *ps, uint32_t mass_len, const V2 *points, uint32_t n, float softening, float *phi) {
    sample("field", ps, mass_len, points, NULL, NULL, 0, n, softening, phi, NULL, NULL);
}

void nb_cpu_potential_map(const Particle *ps, uint32_t mass_len, const RenderView *view, float softening, float *phi) {
    sample_map("field", ps, mass_len, view, softening, phi, NULL, NULL);
}

void nb_cpu_acceleration_at(const Particle *ps, uint32_t mass_len, const V2 *points, uint32_t n, float softening, V2 *acc) {
    sample("gravity", ps, mass_len, points, NULL, NULL, 0, n, softening, NULL, acc, NULL);
}

void nb_cpu_acceleration_map(const Particle *ps, uint32_t mass_len, const RenderView *view, float softening, V2 *acc) {
    sample_map("gravity", ps, mass_len, view, softening, NULL, acc, NULL);
}

void nb_cpu_tidal_at(const Particle *ps, uint32_t mass_len, const V2 *points, uint32_t n, float softening, TidalTensor *t) {
    sample("tidal", ps, mass_len, points, NULL, NULL, 0, n, softening, NULL, NULL, t);
}

void nb_cpu_tidal_map(const Particle *ps, uint32_t mass_len, const RenderView *view, float softening, TidalTensor *t) {
    sample_map("tidal", ps, mass_len, view, softening, NULL, NULL, t);
}
