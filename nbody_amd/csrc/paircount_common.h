/*
 * paircount_common.h -- the statement of include/nbody_paircount.h written once, for the GPU path (paircount.hip) and the host
 * path (paircount_cpu.c): the squared separation of a pair, the row it falls in, the float32 thresholds the device compares
 * against, and the checks of a call.  Both translation units build with -ffp-contract=off, so the two products and the sum of q
 * are rounded one by one on both sides.  The host path's entry point (hidden, libnbody.so) is declared at the bottom.
 *
 * The thresholds.  The row rule compares (double)q with e2[t] = (double)edges[t]^2.  c[t] is the smallest float32 with
 * (double)c[t] >= e2[t].  For a float32 q that is not NaN:  q >= c[t]  <=>  (double)q >= e2[t].
 *   =>  (double)q >= (double)c[t] >= e2[t], conversion being exact and monotone.
 *   <=  (double)q >= e2[t] makes q itself a float32 with (double)q >= e2[t], and c[t] is the smallest of those.
 * Ties: when e2[t] is a float32, c[t] equals it and q == c[t] lies at or above the edge, as (double)q == e2[t] does; when it
 * is not, the float32 just below c[t] lies below e2[t] on both sides.  An e2[t] above FLT_MAX gives c[t] = +inf, which only
 * q = +inf reaches, on both sides; one below the smallest denormal gives that denormal, which only q = 0 stays under.  c[]
 * is nondecreasing (two edges may share a threshold), and the number of t with c[t] <= q is still the row.
 */
#ifndef NB_PAIRCOUNT_COMMON_H
#define NB_PAIRCOUNT_COMMON_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "nbody_paircount.h"

#if defined(__HIPCC__)
#define NB_PAIR_HD __host__ __device__ static inline
#else
#define NB_PAIR_HD static inline
#endif

enum { NB_PAIRS_TABLE = 255 }; /* the thresholds, padded to 2^k - 1 entries for the search */
#define NB_PAIR_UNPLACED 0xffffu

NB_PAIR_HD int nb_pair_finite(float v) {
    union { float f; uint32_t u; } b;
    b.f = v;
    return (b.u & 0x7f800000u) != 0x7f800000u;
}

/* q of the pair (i, j): two differences, two products, one sum, each rounded to float32 on its own; symmetric in (i, j) */
NB_PAIR_HD float nb_pair_q(float xi, float yi, float xj, float yj) {
    const float dx = xi - xj, dy = yi - yj;
    const float dxdx = dx * dx, dydy = dy * dy;
    return dxdx + dydy;
}

/* e2[t] = edges[t]^2: the product of two float32 values is exact in float64 */
NB_PAIR_HD double nb_pair_edge2(float edge) { return (double)edge * (double)edge; }

/* The row of q: the number of t <= bins with e2[t] <= (double)q; NB_PAIR_UNPLACED for a NaN q. */
NB_PAIR_HD uint32_t nb_pair_row(const double *e2, uint32_t bins, float q) {
    if (q != q) return NB_PAIR_UNPLACED;
    const double qd = (double)q;
    uint32_t lo = 0, hi = bins + 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (e2[mid] <= qd)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

/* c = the smallest float32 with (double)c >= edge^2 */
static inline float nb_pair_threshold(float edge) {
    const double e2 = nb_pair_edge2(edge);
    float c = (float)e2; /* to nearest: at most one float32 below the one wanted */
    if ((double)c < e2) c = nextafterf(c, INFINITY);
    return c;
}

/*
 * The device's table: c[0 .. bins] = the thresholds, then NaN (which no q reaches) up to 2 top - 1 entries, top the power of two
 * with bins + 2 <= 2 top.  Returns top; c holds NB_PAIRS_TABLE floats.
 */
static inline uint32_t nb_pair_thresholds(const float *edges, uint32_t bins, float *c) {
    uint32_t top = 1;
    while (2 * top < bins + 2) top *= 2;
    for (uint32_t t = 0; t < NB_PAIRS_TABLE; t++) c[t] = t <= bins ? nb_pair_threshold(edges[t]) : NAN;
    return top;
}

/* The same row from the table, for a q that is not NaN: log2(2 top) comparisons, no branch.  One step, and all of them. */
NB_PAIR_HD uint32_t nb_pair_step_f32(const float *c, uint32_t pos, uint32_t step, float q) { return pos + (c[pos + step - 1] <= q ? step : 0u); }
NB_PAIR_HD uint32_t nb_pair_row_f32(const float *c, uint32_t top, float q) {
    uint32_t pos = 0;
    for (uint32_t step = top; step > 0; step /= 2) pos = nb_pair_step_f32(c, pos, step, q);
    return pos;
}

/* the number of pairs of column `col` (0 MM, 1 MT, 2 TT) of a world of n particles, m of them massive */
NB_PAIR_HD uint64_t nb_pair_total(uint32_t col, uint64_t n, uint64_t m) {
    const uint64_t t = n - m;
    return col == 0 ? m * (m - (m > 0)) / 2 : col == 1 ? m * t : t * (t - (t > 0)) / 2;
}

/* NULL when the edges and the classes are what include/nbody_paircount.h allows, else what is wrong */
static inline const char *nb_pair_fault(const float *edges, uint32_t bins, uint32_t classes) {
    if (bins < 1 || bins > NB_PAIRS_MAX_BINS) return "bins must be 1 .. 254";
    for (uint32_t t = 0; t <= bins; t++)
        if (!nb_pair_finite(edges[t])) return "edges must be finite";
    if (!(edges[0] >= 0.0f)) return "edges must not be negative";
    for (uint32_t t = 0; t < bins; t++)
        if (!(edges[t] < edges[t + 1])) return "edges must be strictly increasing";
    if (classes == 0 || (classes & ~(uint32_t)NB_PAIRS_ALL) != 0) return "classes must be a non-empty set of NB_PAIRS_MM | NB_PAIRS_MT | NB_PAIRS_TT";
    return NULL;
}

#ifdef __cplusplus
extern "C" {
#endif

/* paircount_cpu.c (libnbody.so, not exported): the same statement, over sim_cpu.c's threads (integer counts have no order) */
__attribute__((visibility("hidden"))) void nb_cpu_pair_counts(const Particle *ps, uint32_t total_len, uint32_t mass_len, const float *edges,
                                                              uint32_t bins, uint32_t classes, uint64_t *out, uint64_t *unplaced);

#ifdef __cplusplus
}
#endif

#endif /* NB_PAIRCOUNT_COMMON_H */
