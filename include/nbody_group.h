/*
 * nbody_group.h -- the friends-of-friends groups of a World (libnbody.so): which particles belong together under a linking
 * length, every particle labelled with the smallest index of the connected structure it lies in.  Not part of nbody.h /
 * galaxy.h: the reference has no counterpart.  It is the structure above include/nbody_neighbour.h's per-particle answer: the
 * bound remnants of a collision, the clumps of a tidal tail, the fragments of a merger sweep (the numpy helpers:
 * nbody_amd.group_table, nbody_amd.group_members, nbody_amd.linking_length_for).
 *
 * Definitions.  Particles are in the World's partitioned order (mass > 0 first), N = total_len, M = mass_len.  The massive
 * class is [0, M), the massless class [M, N).
 *
 *   members          a non-empty mask of NB_NEIGH_MASSIVE = 1 | NB_NEIGH_MASSLESS = 2 (include/nbody_neighbour.h's enum): the
 *                    classes that take part
 *   linking_length   float32, finite and >= 0
 *
 * q(i, j) is the q of include/nbody_paircount.h, float32 with every operation rounded on its own:
 *
 *   dx = x_i - x_j      dy = y_i - y_j      q = dx*dx + dy*dy
 *
 *   linked(i, j)   i != j BY INDEX, both of the mask, and (double)q < (double)linking_length * (double)linking_length.  The
 *                  device compares the float32 q against the float32 threshold of nbody_amd/csrc/paircount_common.h, which is
 *                  the same comparison; a NaN q links nothing
 *   group[i]       the smallest index among the particles connected to i through any chain of links; i itself with no link.
 *                  NB_GROUP_NONE for a particle that is not of the mask
 *   n_groups       the number of particles of the mask with group[i] == i; evaluated only when the caller passes a pointer
 *
 * What follows from it.
 *   - Two distinct particles at one place are linked whenever linking_length > 0: q = +0.
 *   - With linking_length == 0 nothing is linked and every particle of the mask is its own group; nothing is launched.
 *   - A particle whose position is NaN or +-inf has a NaN or +inf q to everyone; a +inf q fails the comparison too (the
 *     threshold side is finite, or both are +inf).  Such a particle is a singleton.
 *   - A class that is not of the mask is never read and cannot bridge two groups: whatever it holds changes no bit of the result.
 *
 * No order of evaluation.  The label is the minimum index of a connected component, which is a property of the link graph
 * alone: however the links are found and merged (nbody_amd/csrc/group_common.h: a lock-free union-find whose stored values
 * only ever fall), the result is a function of the state and the arguments, bit for bit on device, host and numpy, with
 * integer atomics only.  There is no float atomic.
 *
 * Not built: periodic boundaries, a linking length per member of an ensemble, velocity-space (6-D) linking, unbinding of group
 * members by energy, groups recorded along a traced update, and sharded pipelines and Worlds (the diagnostics' abort).
 *
 * Where it runs follows GetWorldNeighbours: when the device holds the World's newest state, on the GPU (nb_hip_groups of
 * include/nbody_hip.h) without copying a particle back; otherwise on the host, the same statement.  A World that only ever
 * steps on the CPU never touches a GPU.  The call changes neither the World's state nor a dirty flag.  Sharded Worlds abort.
 * Every fault of the arguments ends in the library's usual "file:line [func] ..." + abort().
 */
#ifndef NBODY_AMD_NBODY_GROUP_H
#define NBODY_AMD_NBODY_GROUP_H

#include <stdint.h>

#include "nbody.h"
#include "nbody_neighbour.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NB_GROUP_NONE 0xFFFFFFFFu

typedef struct WorldGroupSpec {
    uint32_t members;     /* NB_NEIGH_MASSIVE | NB_NEIGH_MASSLESS */
    float linking_length; /* finite and >= 0 */
} WorldGroupSpec;

/* group holds one label per particle, in the order GetWorldParticles returns them; n_groups (nullable) one number. */
void GetWorldGroups(World *w, const WorldGroupSpec *spec, uint32_t *group, uint32_t *n_groups);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_GROUP_H */
