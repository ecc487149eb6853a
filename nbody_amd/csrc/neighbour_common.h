/*
 * neighbour_common.h -- the statement of include/nbody_neighbour.h written once, for the GPU path (neighbour.hip) and the host
 * path (neighbour_cpu.c): the range of a class mask, what one pair does to a receiver's (q, index, count), the 64-bit key that
 * makes the result independent of the order of evaluation, and the checks of a call.  q of a pair is nb_pair_q of
 * paircount_common.h, taken as it is; the device's threshold for the count is nb_pair_threshold of the same header, with its
 * proof that  q < c  <=>  (double)q < (double)radius^2  for every q that is not NaN (a NaN q fails both).  Both translation
 * units build with -ffp-contract=off.  The host path's entry point (hidden, libnbody.so) is declared at the bottom.
 *
 * The key.  A candidate's q is a float32 in [+0, +inf): differences may be -0 but a product of a value with itself and the sum of
 * two such are +0 or above.  For such values the bit pattern orders like the value, so
 *
 *     key(q, j) = (bits(q) << 32) | j
 *
 * as an unsigned 64-bit integer orders candidates by q first and by j among equal q: the smallest key is the neighbour the
 * statement asks for.  Minimum is associative and commutative, so any split of the sources into parts, evaluated in any order
 * and merged by minimum, ends in the same key; the counts merge by integer addition.  The key of "no candidate" is all ones:
 * above every candidate's, and its low word is NB_NEIGH_NONE.
 */
#ifndef NB_NEIGHBOUR_COMMON_H
#define NB_NEIGHBOUR_COMMON_H

#include "nbody_neighbour.h"
#include "paircount_common.h"

#define NB_NEIGH_KEY_NONE 0xFFFFFFFFFFFFFFFFull

/* the particles [*lo, *hi) of a class mask in a world of n particles, m of them massive */
NB_PAIR_HD void nb_neigh_range(uint32_t mask, uint32_t n, uint32_t m, uint32_t *lo, uint32_t *hi) {
    *lo = (mask & NB_NEIGH_MASSIVE) ? 0u : m;
    *hi = (mask & NB_NEIGH_MASSLESS) ? n : m;
}

NB_PAIR_HD uint32_t nb_neigh_bits(float q) {
    union { float f; uint32_t u; } b;
    b.f = q;
    return b.u;
}

NB_PAIR_HD float nb_neigh_unbits(uint32_t u) {
    union { float f; uint32_t u; } b;
    b.u = u;
    return b.f;
}

/*
 * Source j with pair value q, offered to a receiver that holds (*best_q, *best_j), +inf and NB_NEIGH_NONE at first: taken when
 * q is strictly smaller.  A NaN q and a q of +inf are never smaller than what is held, so they are never candidates.  Offered in
 * increasing j this keeps the smallest index among equal q; offered in any order, nb_neigh_key merges.
 */
NB_PAIR_HD void nb_neigh_take(float q, uint32_t j, float *best_q, uint32_t *best_j) {
    const int closer = q < *best_q;
    *best_q = closer ? q : *best_q;
    *best_j = closer ? j : *best_j;
}

NB_PAIR_HD uint64_t nb_neigh_key(float best_q, uint32_t best_j) {
    return best_j == NB_NEIGH_NONE ? NB_NEIGH_KEY_NONE : ((uint64_t)nb_neigh_bits(best_q) << 32) | best_j;
}

/* a merged key back to (q, index): a low word of NB_NEIGH_NONE is "no candidate" */
NB_PAIR_HD void nb_neigh_decode(uint64_t key, float *q, uint32_t *index) {
    const uint32_t j = (uint32_t)key;
    *index = j;
    *q = j == NB_NEIGH_NONE ? nb_neigh_unbits(0x7f800000u) : nb_neigh_unbits((uint32_t)(key >> 32));
}

/* what a particle that is no receiver, or a receiver without a candidate, gets */
static inline void nb_neigh_defaults(uint64_t len, float *q, uint32_t *index, uint32_t *count) {
    for (uint64_t i = 0; i < len; i++) {
        q[i] = INFINITY;
        index[i] = NB_NEIGH_NONE;
        if (count) count[i] = 0;
    }
}

/* NULL when the masks and the radius are what include/nbody_neighbour.h allows, else what is wrong */
static inline const char *nb_neigh_fault(uint32_t receivers, uint32_t sources, float radius, int counted) {
    if (receivers == 0 || (receivers & ~(uint32_t)NB_NEIGH_ALL) != 0) return "receivers must be a non-empty set of NB_NEIGH_MASSIVE | NB_NEIGH_MASSLESS";
    if (sources == 0 || (sources & ~(uint32_t)NB_NEIGH_ALL) != 0) return "sources must be a non-empty set of NB_NEIGH_MASSIVE | NB_NEIGH_MASSLESS";
    if (counted && !nb_pair_finite(radius)) return "radius must be finite";
    if (counted && !(radius >= 0.0f)) return "radius must not be negative";
    return NULL;
}

#ifdef __cplusplus
extern "C" {
#endif

/* neighbour_cpu.c (libnbody.so, not exported): the same statement, over sim_cpu.c's threads (receivers are independent) */
__attribute__((visibility("hidden"))) void nb_cpu_neighbours(const Particle *ps, uint32_t total_len, uint32_t mass_len, uint32_t receivers,
                                                             uint32_t sources, float radius, float *q, uint32_t *index, uint32_t *count);

#ifdef __cplusplus
}
#endif

#endif /* NB_NEIGHBOUR_COMMON_H */
