/*
 * profile_cpu.c -- the host path of include/nbody_profile.h: GetWorldProfile of a World whose particle array holds the newest
 * state, and every member of a WorldBatch that never stepped on the GPU.
 *
 * The statement of profile_common.h in the order of the header: chunks of NB_PROFILE_CHUNK consecutive particles, inside a
 * chunk every row's terms in index order from +0.0, then the chunk totals in chunk order from +0.0 (a row the chunk left
 * empty adds +0.0).  One thread: O(N log bins), and the order is the contract.
 */
#include "profile_common.h"

#include <string.h>

void nb_cpu_profile(const Particle *ps, uint32_t total_len, uint32_t mass_len, const float *edges, uint32_t bins, const float *centre,
                    int weights, double *out, uint32_t *unplaced) {
    const uint32_t rows = bins + 2;
    const uint32_t n = weights == NB_PROFILE_BY_MASS ? mass_len : total_len;
    double e2[NB_PROFILE_MAX_BINS + 1];
    double chunk[(NB_PROFILE_MAX_BINS + 2) * NB_PROFILE_QTY];
    for (uint32_t t = 0; t <= bins; t++) e2[t] = nb_profile_edge2(edges[t]);
    for (uint32_t i = 0; i < rows * NB_PROFILE_QTY; i++) out[i] = 0.0;
    uint32_t lost = 0;
    for (uint32_t first = 0; first < n; first += NB_PROFILE_CHUNK) {
        const uint32_t last = n - first < NB_PROFILE_CHUNK ? n : first + NB_PROFILE_CHUNK;
        for (uint32_t i = 0; i < rows * NB_PROFILE_QTY; i++) chunk[i] = 0.0;
        for (uint32_t i = first; i < last; i++) {
            const Particle *p = ps + i;
            double term[NB_PROFILE_TERMS];
            const double wgt = weights == NB_PROFILE_BY_MASS ? (double)p->mass : 1.0;
            const double q = nb_profile_terms(p->pos.x, p->pos.y, p->vel.x, p->vel.y, wgt, centre, term);
            const uint32_t r = nb_profile_row(e2, bins, q);
            if (r == NB_PROFILE_UNPLACED) {
                lost++;
                continue;
            }
            double *row = chunk + (size_t)r * NB_PROFILE_QTY;
            row[0] += 1.0;
            for (uint32_t c = 0; c < NB_PROFILE_TERMS; c++) row[1 + c] += term[c];
        }
        for (uint32_t i = 0; i < rows * NB_PROFILE_QTY; i++) out[i] += chunk[i];
    }
    if (unplaced) *unplaced = lost;
}
