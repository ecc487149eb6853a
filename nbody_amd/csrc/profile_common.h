/*
 * profile_common.h -- the statement of include/nbody_profile.h written once, for the GPU path (profile.hip) and the host path
 * (profile_cpu.c): the six float64 values of one particle about a centre, the row a squared radius falls in, and the checks
 * of a call.  Both translation units build with -ffp-contract=off, so every float64 operation below is rounded on its own on
 * both sides; only + - * are used (no divide, no sqrt), which is what lets the device, the host and numpy agree bit for bit.
 * The host path's entry point (hidden, libnbody.so) is declared at the bottom.
 */
#ifndef NB_PROFILE_COMMON_H
#define NB_PROFILE_COMMON_H

#include <stddef.h>
#include <stdint.h>

#include "nbody_profile.h"

#if defined(__HIPCC__)
#define NB_PROFILE_HD __host__ __device__ static inline
#else
#define NB_PROFILE_HD static inline
#endif

/* the terms a placed particle adds to its row's columns 1 .. 5 (column 0 counts it) */
enum { NB_PROFILE_TERMS = NB_PROFILE_QTY - 1 };

NB_PROFILE_HD int nb_profile_finite(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return (b.u & 0x7f800000u) != 0x7f800000u;
}

/* e2[t] = edges[t]^2: the product of two float32 values is exact in float64, so e2 is as strictly increasing as edges */
NB_PROFILE_HD double nb_profile_edge2(float edge) { return (double)edge * (double)edge; }

/*
 * One particle about the centre c = (cx, cy, ux, uy) with weight wgt: its squared radius q (returned) and
 * term[] = (wgt, wgt q, wgt j, wgt w, wgt k), every difference, product and sum rounded on its own.
 */
NB_PROFILE_HD double nb_profile_terms(float x, float y, float vx, float vy, double wgt, const float *c, double *term) {
    const double dx = (double)x - (double)c[0], dy = (double)y - (double)c[1];
    const double sx = (double)vx - (double)c[2], sy = (double)vy - (double)c[3];
    const double dxdx = dx * dx, dydy = dy * dy;
    const double q = dxdx + dydy;
    const double a = dx * sy, b = dy * sx;
    const double j = a - b;
    const double e = dx * sx, f = dy * sy;
    const double w = e + f;
    const double g = sx * sx, h = sy * sy;
    const double k = g + h;
    term[0] = wgt;
    term[1] = wgt * q;
    term[2] = wgt * j;
    term[3] = wgt * w;
    term[4] = wgt * k;
    return q;
}

/*
 * The row of q: the number of t <= bins with e2[t] <= q -- 0 below the first edge, t inside bin t, bins + 1 at or beyond the
 * last edge (+inf included).  NB_PROFILE_UNPLACED for a NaN q, which lies in no row.
 */
#define NB_PROFILE_UNPLACED 0xffffu
NB_PROFILE_HD uint32_t nb_profile_row(const double *e2, uint32_t bins, double q) {
    if (q != q) return NB_PROFILE_UNPLACED;
    uint32_t lo = 0, hi = bins + 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (e2[mid] <= q)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

/* NULL when the edges, `count` centres of four floats and the weights are what include/nbody_profile.h allows, else what is wrong */
static inline const char *nb_profile_fault(const float *edges, uint32_t bins, const float *centres, uint32_t count, int weights) {
    if (bins < 1 || bins > NB_PROFILE_MAX_BINS) return "bins must be 1 .. 254";
    for (uint32_t t = 0; t <= bins; t++)
        if (!nb_profile_finite(edges[t])) return "edges must be finite";
    if (!(edges[0] >= 0.0f)) return "edges must not be negative";
    for (uint32_t t = 0; t < bins; t++)
        if (!(edges[t] < edges[t + 1])) return "edges must be strictly increasing";
    for (size_t i = 0; i < (size_t)count * 4; i++)
        if (!nb_profile_finite(centres[i])) return "centre and centre velocity must be finite";
    if (weights != NB_PROFILE_BY_MASS && weights != NB_PROFILE_BY_NUMBER) return "weights must be NB_PROFILE_BY_MASS or NB_PROFILE_BY_NUMBER";
    return NULL;
}

#ifdef __cplusplus
extern "C" {
#endif

/* profile_cpu.c (libnbody.so, not exported): the same statement in the same order, one thread */
__attribute__((visibility("hidden"))) void nb_cpu_profile(const Particle *ps, uint32_t total_len, uint32_t mass_len, const float *edges,
                                                          uint32_t bins, const float *centre, int weights, double *out,
                                                          uint32_t *unplaced);

#ifdef __cplusplus
}
#endif

#endif /* NB_PROFILE_COMMON_H */
