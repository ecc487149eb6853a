/*
 * paircount_cpu.c -- the host path of include/nbody_paircount.h: GetWorldPairCounts of a World whose particle array holds the
 * newest state, and every member of a WorldBatch that never stepped on the GPU.
 *
 * The statement of paircount_common.h, every unordered pair once: receiver i against the sources j > i of the classes asked
 * for.  A class that is not asked for is never walked, so a particle only it would read is never read.  The receivers are
 * dealt to sim_cpu.c's OpenMP threads, each with a table of its own; the tables are integers, so the order they are added in
 * cannot show.
 */
#include "paircount_common.h"

#include <string.h>

enum { ROWS_MAX = NB_PAIRS_MAX_BINS + 2, CELLS = (ROWS_MAX + 1) * NB_PAIRS_COLUMNS }; /* one more row: the unplaced pairs */

static void count_range(const Particle *ps, uint32_t i, uint32_t j0, uint32_t j1, const double *e2, uint32_t bins, uint32_t col, uint64_t *tab) {
    const float xi = ps[i].pos.x, yi = ps[i].pos.y;
    for (uint32_t j = j0; j < j1; j++) {
        const uint32_t r = nb_pair_row(e2, bins, nb_pair_q(xi, yi, ps[j].pos.x, ps[j].pos.y));
        tab[(r == NB_PAIR_UNPLACED ? ROWS_MAX : r) * NB_PAIRS_COLUMNS + col]++;
    }
}

void nb_cpu_pair_counts(const Particle *ps, uint32_t total_len, uint32_t mass_len, const float *edges, uint32_t bins, uint32_t classes,
                        uint64_t *out, uint64_t *unplaced) {
    const uint32_t rows = bins + 2, n = total_len, m = mass_len;
    double e2[NB_PAIRS_MAX_BINS + 1];
    for (uint32_t t = 0; t <= bins; t++) e2[t] = nb_pair_edge2(edges[t]);
    uint64_t total[CELLS];
    memset(total, 0, sizeof total);
    /* the receivers some requested class starts from */
    const uint32_t first = (classes & (NB_PAIRS_MM | NB_PAIRS_MT)) ? 0 : m;
    const uint32_t last = (classes & NB_PAIRS_TT) ? n : m;
    const int go_parallel = (double)n * (double)n >= 2.0e6;
#pragma omp parallel if (go_parallel)
    {
        uint64_t tab[CELLS];
        memset(tab, 0, sizeof tab);
#pragma omp for schedule(dynamic, 16) nowait
        for (uint32_t i = first; i < last; i++) {
            if (i < m) {
                if (classes & NB_PAIRS_MM) count_range(ps, i, i + 1, m, e2, bins, 0, tab);
                if (classes & NB_PAIRS_MT) count_range(ps, i, m, n, e2, bins, 1, tab);
            } else {
                count_range(ps, i, i + 1, n, e2, bins, 2, tab); /* i >= m is only reached with NB_PAIRS_TT */
            }
        }
#pragma omp critical(nb_pair_counts_join)
        for (uint32_t k = 0; k < CELLS; k++) total[k] += tab[k];
    }
    memcpy(out, total, (size_t)rows * NB_PAIRS_COLUMNS * sizeof(uint64_t));
    if (unplaced) memcpy(unplaced, total + (size_t)ROWS_MAX * NB_PAIRS_COLUMNS, NB_PAIRS_COLUMNS * sizeof(uint64_t));
}
