/*
 * world_partition.h -- the mass partition every World-layer constructor applies (world.c CreateWorld*, world_batch.c
 * CreateWorldBatch): one copy, because its output permutation is the index order every later read returns.
 * Internal to the C layer; not installed.
 */
#ifndef NB_WORLD_PARTITION_H
#define NB_WORLD_PARTITION_H

#include <stdint.h>

#include "nbody.h"

/*
 * In-place unstable partition, massive particles first; returns their count.
 * `lo` hunts upward for a massless slot, `hi` downward for a massive one, and
 * they swap until they meet -- the reference's scheme, kept because its output
 * permutation is part of the observable contract.
 */
static inline uint32_t partition_by_mass(Particle *p, uint32_t count) {
    uint32_t lo = 0, hi = count;
    for (;;) {
        for (; lo < hi && p[lo].mass > 0; lo++) {
        }
        while (lo < hi) {
            hi--;
            if (!(p[hi].mass <= 0)) break;
        }
        if (lo == hi) return hi;
        const Particle keep = p[lo];
        p[lo] = p[hi];
        p[hi] = keep;
    }
}

#endif /* NB_WORLD_PARTITION_H */
