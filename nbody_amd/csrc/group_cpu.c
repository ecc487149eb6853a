/*
 * group_cpu.c -- the host path of include/nbody_group.h: GetWorldGroups of a World whose particle array holds the newest state,
 * and every member of a WorldBatch that never stepped on the GPU.
 *
 * The statement of group_common.h: the pairs j < i of the mask (a link is symmetric), every linked pair united through the same
 * union-find the device uses, here over the compiler's __atomic builtins, then group[i] = find(i).  A class that is not of the
 * mask is never walked, so its particles are never read.  The receivers are dealt to sim_cpu.c's OpenMP threads; the table's
 * final roots are the smallest indices of the components whatever the threads did in between (group_common.h, the argument), so
 * the thread count cannot show.  A thread keeps the last root it saw for its receiver and skips the hook when a linked source
 * already has it: a speed device only.
 */
#include "group_common.h"

void nb_cpu_groups(const Particle *ps, uint32_t total_len, uint32_t mass_len, uint32_t members, float linking_length, uint32_t *group,
                   uint32_t *n_groups) {
    const uint32_t n = total_len, m = mass_len;
    uint32_t lo, hi;
    nb_neigh_range(members, n, m, &lo, &hi);
    nb_group_defaults(n, m, members, group); /* parent = identity on the mask */
    if (linking_length > 0.0f && hi > lo + 1) {
        const double l2 = nb_pair_edge2(linking_length);
        uint32_t *parent = group;
        const int go_parallel = (double)(hi - lo) * (double)(hi - lo) >= 4.0e6;
#pragma omp parallel for schedule(dynamic, 64) if (go_parallel)
        for (uint32_t i = lo; i < hi; i++) {
            const float xi = ps[i].pos.x, yi = ps[i].pos.y;
            uint32_t root = i;
            for (uint32_t j = lo; j < i; j++) {
                if (!nb_group_linked(nb_pair_q(xi, yi, ps[j].pos.x, ps[j].pos.y), l2)) continue;
                const uint32_t rj = nb_group_find(parent, j);
                if (rj != root) root = nb_group_unite(parent, root, rj);
            }
        }
        /* behind the parallel region: every hook is in the table.  In place: a label is a valid, fully compressed parent */
        for (uint32_t i = lo; i < hi; i++) group[i] = nb_group_find(parent, i);
    }
    if (n_groups) *n_groups = nb_group_count(group, n);
}
