/*
 * group_common.h -- the statement of include/nbody_group.h written once, for the GPU path (group.hip) and the host path
 * (group_cpu.c): which pairs link, the union-find the links are merged through, and the checks of a call.  The range of the
 * mask is nb_neigh_range of neighbour_common.h; q of a pair and the device's threshold are nb_pair_q and nb_pair_threshold of
 * paircount_common.h, taken as they are, with that header's proof that  q < c  <=>  (double)q < (double)linking_length^2  for
 * every q that is not NaN (a NaN q fails both).  Both translation units build with -ffp-contract=off.  The host path's entry
 * point (hidden, libnbody.so) is declared at the bottom.
 *
 * The union-find.  parent[] holds one 32-bit word per particle; the three operations on it are NB_GROUP_LOAD, NB_GROUP_CAS and
 * NB_GROUP_MIN below: relaxed atomics, of agent scope on the device and the compiler's __atomic builtins on the host.  Nothing
 * else touches the table while pairs are being merged.  Why the result is right under any interleaving and any stale read:
 *
 *   1. INVARIANT: parent[x] <= x always, and a stored value only ever falls.  The table starts as parent[x] = x.  A hook
 *      (nb_group_unite) stores the smaller of two roots into the larger, by compare-and-swap against the larger's own index.
 *      Compression (nb_group_find) is an atomic minimum towards a value read further up the same tree.  So no cycle can exist
 *      (every non-root points strictly down), the root of a tree is its smallest index, and a value once stored in parent[x] is
 *      an index of x's own tree for ever: trees are only ever merged, never split.  A tree lies within one component of the link
 *      graph (every hook joins the trees of two linked particles); once every link has been united its two ends share a tree;
 *      so in the end tree = component and the root of a particle is the smallest index of its component.
 *   2. find(x) follows x <- load(parent[x]) until the value equals x.  Every hop strictly decreases x, so it ends in at most x
 *      hops whatever the loads return.
 *   3. unite(a, b) loops: a = find(a), b = find(b); equal: done; else compare-and-swap parent[hi] from hi to lo, hi the larger.
 *      Taken: done.  Not taken: the atomic hands back what parent[hi] holds, a value below hi, and the loop goes on with
 *      (that value, lo) -- never with a re-read.  max(a, b) strictly falls at every failed round, so it ends.  No thread ever
 *      waits for another: no spin, no lock, no flag.
 *   4. STALE READS are harmless by construction.  A compute unit's L1 is never refreshed by another's stores and every XCD has
 *      an L2 of its own; but an old value of parent[x] is still <= x and still of x's tree, so a find that walks old values
 *      ends on a node of the right tree that may no longer be a root -- and then the compare-and-swap, which acts on memory,
 *      fails and hands back the current value.  Nothing is published and nothing needs a release/acquire hand-off: only
 *      monotone integers meet, and only through atomics.  Still, inside the pair launch every access to the table is one of the
 *      three atomics on a global address, never a plain load and never a scalar load: the table stays off the scalar cache the
 *      positions come through.
 *   5. The labels are read off in a launch of their own behind the pair launch (the kernel boundary makes the table visible):
 *      group[i] = find(i).
 * tests/group_schedule.c runs nb_group_find and nb_group_unite as they stand below over every schedule of tiny cases and seeded
 * schedules of larger ones, a load returning any value its word ever held, and checks 1 to 3 after every operation.
 */
#ifndef NB_GROUP_COMMON_H
#define NB_GROUP_COMMON_H

#include "nbody_group.h"
#include "neighbour_common.h"
#include "paircount_common.h"

/* the three operations on the table; NB_GROUP_CAS returns what the word held before */
#if defined(__HIP_DEVICE_COMPILE__)
#define NB_GROUP_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define NB_GROUP_CAS(p, expected, desired) atomicCAS((p), (expected), (desired))
#define NB_GROUP_MIN(p, v) ((void)atomicMin((p), (v)))
#elif defined(NB_GROUP_OPS_HEADER)
/* a stand-alone host program supplies the three operations itself: tests/group_schedule.c runs nb_group_find and nb_group_unite
 * as they stand here under a scheduler that picks every interleaving and every stale value */
#include NB_GROUP_OPS_HEADER
#else
static inline uint32_t nb_group_host_cas(uint32_t *p, uint32_t expected, uint32_t desired) {
    __atomic_compare_exchange_n(p, &expected, desired, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expected; /* taken: still the expected value; not taken: what the word holds */
}
static inline void nb_group_host_min(uint32_t *p, uint32_t v) {
    uint32_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < old && !__atomic_compare_exchange_n(p, &old, v, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
}
#define NB_GROUP_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define NB_GROUP_CAS(p, expected, desired) nb_group_host_cas((p), (expected), (desired))
#define NB_GROUP_MIN(p, v) nb_group_host_min((p), (v))
#endif

/* does the pair value q link under the float64 rule (the host) */
NB_PAIR_HD int nb_group_linked(float q, double l2) { return (double)q < l2; }

/*
 * The root of x's tree as the loads show it (argument 2).  On the way every node met is pointed at its grandparent where that
 * lies lower: an atomic minimum towards a value of the same tree, a speed device only -- without it the same root is found.
 */
NB_PAIR_HD uint32_t nb_group_find(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = NB_GROUP_LOAD(parent + x);
        if (p == x) return x;
        const uint32_t g = NB_GROUP_LOAD(parent + p);
        if (g < p) NB_GROUP_MIN(parent + x, g);
        x = g;
    }
}

/*
 * Joins the trees of a and b (argument 3) and returns a node of the joined tree that is not above a nor above b: the root as this
 * call's last operation showed it.  Another thread may have hooked that node lower by the time the call returns, and a stale
 * find may have ended on a node that was no root any more (tests/group_schedule.c counts such returns), so it is NOT "the root
 * when the call ended".  The callers need no more than this: they compare it and hand it to the next find or unite.
 */
NB_PAIR_HD uint32_t nb_group_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = nb_group_find(parent, a);
        b = nb_group_find(parent, b);
        if (a == b) return a;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = NB_GROUP_CAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        a = old; /* what the atomic returned: below hi, of hi's tree */
        b = lo;
    }
}

/* what a call with nothing to link gives (linking_length == 0, or fewer than two particles of the mask): every particle of the
 * mask its own group */
static inline void nb_group_defaults(uint32_t n, uint32_t m, uint32_t members, uint32_t *group) {
    uint32_t lo, hi;
    nb_neigh_range(members, n, m, &lo, &hi);
    for (uint32_t i = 0; i < n; i++) group[i] = i >= lo && i < hi ? i : NB_GROUP_NONE;
}

/* n_groups of one world's labels: the particles that are their own label (a particle outside the mask holds NB_GROUP_NONE) */
static inline uint32_t nb_group_count(const uint32_t *group, uint32_t n) {
    uint32_t roots = 0;
    for (uint32_t i = 0; i < n; i++) roots += group[i] == i;
    return roots;
}

/* NULL when the mask and the linking length are what include/nbody_group.h allows, else what is wrong */
static inline const char *nb_group_fault(uint32_t members, float linking_length) {
    if (members == 0 || (members & ~(uint32_t)NB_NEIGH_ALL) != 0) return "members must be a non-empty set of NB_NEIGH_MASSIVE | NB_NEIGH_MASSLESS";
    if (!nb_pair_finite(linking_length)) return "linking_length must be finite";
    if (!(linking_length >= 0.0f)) return "linking_length must not be negative";
    return NULL;
}

#ifdef __cplusplus
extern "C" {
#endif

/* group_cpu.c (libnbody.so, not exported): the same statement, the pair scan over sim_cpu.c's threads */
__attribute__((visibility("hidden"))) void nb_cpu_groups(const Particle *ps, uint32_t total_len, uint32_t mass_len, uint32_t members,
                                                         float linking_length, uint32_t *group, uint32_t *n_groups);

#ifdef __cplusplus
}
#endif

#endif /* NB_GROUP_COMMON_H */
