/*
 * timestep_cpu.c -- the host path of include/nbody_adaptive.h: the criterion of timestep_common.h over a particle array.
 * The minimum of floats is exact in any order, so this serial loop gives the bits of the device kernels (timestep.hip); it is
 * O(N) beside a host step's O(N * M) and is not threaded.
 */
#include "timestep_common.h"

/* (hidden, libnbody.so) q = min over ps[0 .. n) of q_i; +inf when no particle contributes */
__attribute__((visibility("hidden"))) float nb_cpu_timestep_q(const Particle *ps, uint32_t n) {
    float q = NB_TS_INF;
    for (uint32_t i = 0; i < n; i++) {
        const float qi = nb_timestep_q(ps[i].acc.x, ps[i].acc.y, ps[i].radius);
        if (qi < q) q = qi;
    }
    return q;
}

/* (hidden) the criterion without the span clip */
__attribute__((visibility("hidden"))) float nb_cpu_timestep(const Particle *ps, uint32_t n, const NbAdaptive *cfg) {
    return nb_timestep_dt(nb_cpu_timestep_q(ps, n), cfg->eta, cfg->dt_min, cfg->dt_max);
}
