/*
 * neighbour_cpu.c -- the host path of include/nbody_neighbour.h: GetWorldNeighbours of a World whose particle array holds the
 * newest state, and every member of a WorldBatch that never stepped on the GPU.
 *
 * The statement of neighbour_common.h, receiver by receiver: the sources of the source mask in increasing j, the receiver's own
 * index left out, every pair offered to nb_neigh_take.  A class that is neither receiver nor source is never walked, so its
 * particles are never read.  The receivers are dealt to sim_cpu.c's OpenMP threads; each writes only its own entries, so the
 * thread count cannot show.
 */
#include "neighbour_common.h"

void nb_cpu_neighbours(const Particle *ps, uint32_t total_len, uint32_t mass_len, uint32_t receivers, uint32_t sources, float radius, float *q,
                       uint32_t *index, uint32_t *count) {
    const uint32_t n = total_len, m = mass_len;
    uint32_t r0, r1, s0, s1;
    nb_neigh_range(receivers, n, m, &r0, &r1);
    nb_neigh_range(sources, n, m, &s0, &s1);
    nb_neigh_defaults(n, q, index, count);
    if (r1 <= r0 || s1 <= s0) return;
    const double r2 = count ? nb_pair_edge2(radius) : 0.0;
    const int go_parallel = (double)(r1 - r0) * (double)(s1 - s0) >= 2.0e6;
#pragma omp parallel for schedule(static) if (go_parallel)
    for (uint32_t i = r0; i < r1; i++) {
        const float xi = ps[i].pos.x, yi = ps[i].pos.y;
        float best_q = INFINITY;
        uint32_t best_j = NB_NEIGH_NONE, within = 0;
        for (uint32_t j = s0; j < s1; j++) {
            if (j == i) continue;
            const float v = nb_pair_q(xi, yi, ps[j].pos.x, ps[j].pos.y);
            nb_neigh_take(v, j, &best_q, &best_j);
            within += (double)v < r2; /* false for a NaN and for +inf: only candidates count */
        }
        nb_neigh_decode(nb_neigh_key(best_q, best_j), &q[i], &index[i]);
        if (count) count[i] = within;
    }
}
