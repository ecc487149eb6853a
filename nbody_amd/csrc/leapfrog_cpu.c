/*
 * leapfrog_cpu.c -- the host path of include/nbody_leapfrog.h: the kick / drift passes of leapfrog_common.h over a particle
 * array.  O(N) beside a host step's O(N * M) and not threaded; world.c puts UpdateWorld_CPU(w, 0, 1) between them.
 */
#include "leapfrog_common.h"
#include "nbody.h"

/* (hidden, libnbody.so) open(dt): the opening half kick with the stored acc, then the drift with the new velocity */
__attribute__((visibility("hidden"))) void nb_cpu_leapfrog_open(Particle *ps, uint32_t n, float dt) {
    const float h = nb_leapfrog_half(dt);
    for (uint32_t i = 0; i < n; i++) {
        ps[i].vel.x = nb_leapfrog_kick(ps[i].vel.x, ps[i].acc.x, h);
        ps[i].vel.y = nb_leapfrog_kick(ps[i].vel.y, ps[i].acc.y, h);
        ps[i].pos.x = nb_leapfrog_drift(ps[i].pos.x, ps[i].vel.x, dt);
        ps[i].pos.y = nb_leapfrog_drift(ps[i].pos.y, ps[i].vel.y, dt);
    }
}

/* (hidden) close(dt): the closing half kick with the acc the force step left */
__attribute__((visibility("hidden"))) void nb_cpu_leapfrog_close(Particle *ps, uint32_t n, float dt) {
    const float h = nb_leapfrog_half(dt);
    for (uint32_t i = 0; i < n; i++) {
        ps[i].vel.x = nb_leapfrog_kick(ps[i].vel.x, ps[i].acc.x, h);
        ps[i].vel.y = nb_leapfrog_kick(ps[i].vel.y, ps[i].acc.y, h);
    }
}
