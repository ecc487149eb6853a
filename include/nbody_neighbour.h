/*
 * nbody_neighbour.h -- the nearest neighbour and the neighbour count of every particle of a World (libnbody.so): for each
 * particle, which other particle is closest, how far away it is, and how many lie within a radius.  Not part of nbody.h /
 * galaxy.h: the reference has no counterpart.  It is the per-particle answer below include/nbody_paircount.h's per-bin one:
 * which pair set the adaptive step (include/nbody_adaptive.h), which close pairs exist, the local density 1 / (pi d^2) or
 * count / (pi h^2), and overlap candidates (the numpy helpers: nbody_amd.neighbour_distance, nbody_amd.closest_pairs).
 *
 * Definitions.  Particles are in the World's partitioned order (mass > 0 first), N = total_len, M = mass_len.  The massive
 * class is [0, M), the massless class [M, N).
 *
 *   receivers, sources   each a non-empty mask of NB_NEIGH_MASSIVE = 1 | NB_NEIGH_MASSLESS = 2
 *   radius               float32, finite and >= 0; used only when a count is asked for
 *
 * q(i, j) is the q of include/nbody_paircount.h, float32 with every operation rounded on its own:
 *
 *   dx = x_i - x_j      dy = y_i - y_j      q = dx*dx + dy*dy
 *
 * Candidates of receiver i: the sources j of the source mask with j != i BY INDEX and q(i, j) < +inf.  Two distinct particles
 * at one place are candidates with q = +0.  A NaN q is not a candidate, and neither is a q that overflowed to +inf.
 *
 *   index[i]   the candidate with the smallest q; among equal q the smallest j.  NB_NEIGH_NONE with no candidate
 *   q[i]       that q; +inf with no candidate
 *   count[i]   the number of candidates with (double)q < (double)radius * (double)radius; evaluated only when the caller
 *              passes a count array.  The device compares the float32 q against the float32 threshold of
 *              nbody_amd/csrc/paircount_common.h, which is the same comparison
 *
 * A particle that is not a receiver gets (+inf, NB_NEIGH_NONE, 0).  A class that is neither receiver nor source is never read:
 * whatever it holds changes no bit of the result.
 *
 * No order of evaluation.  For q >= +0 the bit pattern of q orders like q, so the 64-bit key (bits(q) << 32) | j orders
 * candidates exactly as the rule above and the minimum of a set of keys does not depend on how the set is split; the counts
 * are integers.  The result is therefore a function of the state and the arguments alone, bit for bit on device, host and
 * numpy, with integer atomics only.  There is no float atomic.
 *
 * Not built: the k > 1 nearest neighbours, periodic boundaries, a radius per member of an ensemble, and a nearest distance
 * recorded along a traced update.
 *
 * Where it runs follows GetWorldPairCounts: when the device holds the World's newest state, on the GPU (nb_hip_neighbours of
 * include/nbody_hip.h) without copying a particle back; otherwise on the host, the same statement.  A World that only ever
 * steps on the CPU never touches a GPU.  The call changes neither the World's state nor a dirty flag.  Sharded Worlds abort.
 * Every fault of the arguments ends in the library's usual "file:line [func] ..." + abort().
 */
#ifndef NBODY_AMD_NBODY_NEIGHBOUR_H
#define NBODY_AMD_NBODY_NEIGHBOUR_H

#include <stdint.h>

#include "nbody.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { NB_NEIGH_MASSIVE = 1, NB_NEIGH_MASSLESS = 2, NB_NEIGH_ALL = 3 };
#define NB_NEIGH_NONE 0xFFFFFFFFu

typedef struct WorldNeighbourSpec {
    uint32_t receivers; /* NB_NEIGH_MASSIVE | NB_NEIGH_MASSLESS */
    uint32_t sources;   /* likewise */
    float radius;       /* of the count; read only when count is not NULL */
} WorldNeighbourSpec;

/* q, index and count (nullable) hold one entry per particle, in the order GetWorldParticles returns them. */
void GetWorldNeighbours(World *w, const WorldNeighbourSpec *spec, float *q, uint32_t *index, uint32_t *count);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_NEIGHBOUR_H */
