/*
 * diag_cpu.c -- the host path of include/nbody_diag.h: GetWorldEnergy / GetWorldPotential of a World whose particle
 * array holds the newest state (it only ever stepped on the CPU, or stepped on the CPU last).
 *
 * Same definitions as the GPU path (diagnostics.hip), all in float64: G*m_j = (double)NB_G * m_j, the receiver's
 * radius added to the squared distance, the self term skipped by index.  OpenMP splits the receivers; every Phi_i is
 * one sequential sum over j in index order, and the sums over i run sequentially afterwards, so the result does not
 * depend on the thread count.  O(N * M): fine for checks and small worlds, slow for 2^20 particles (seconds to minutes),
 * where the GPU path is the one to use.
 */
#include "nbody_diag.h"

#include <math.h>
#include <stdint.h>

#include "diag_sums.h"
#include "nb_util.h"

static double potential_of(const Particle *ps, uint32_t mass_len, uint32_t i) {
    const double xi = ps[i].pos.x, yi = ps[i].pos.y, ri = ps[i].radius;
    double sum = 0.0;
    for (uint32_t j = 0; j < mass_len; j++) {
        if (j == i) continue;
        const double dx = (double)ps[j].pos.x - xi, dy = (double)ps[j].pos.y - yi;
        sum += (double)NB_G * (double)ps[j].mass / sqrt(dx * dx + dy * dy + ri);
    }
    return -sum;
}

void nb_cpu_potential(const Particle *ps, uint32_t total_len, uint32_t mass_len, float *phi) {
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)total_len; i++) phi[i] = (float)potential_of(ps, mass_len, (uint32_t)i);
}

void nb_cpu_energy(const Particle *ps, uint32_t total_len, uint32_t mass_len, WorldEnergy *out) {
    (void)total_len;   /* massless particles add nothing */
    double *phi = NB_NEW(mass_len ? mass_len : 1, double);
    NB_CHECK(phi != NULL, "Failed to alloc %u potentials", mass_len);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < (int64_t)mass_len; i++) phi[i] = potential_of(ps, mass_len, (uint32_t)i);
    double q[NB_DIAG_SUMS] = {0};
    for (uint32_t i = 0; i < mass_len; i++) {
        const double m = ps[i].mass, x = ps[i].pos.x, y = ps[i].pos.y, vx = ps[i].vel.x, vy = ps[i].vel.y;
        q[0] += m * phi[i];
        q[1] += m * (vx * vx + vy * vy);
        q[2] += m;
        q[3] += m * vx;
        q[4] += m * vy;
        q[5] += m * (x * vy - y * vx);
        q[6] += m * x;
        q[7] += m * y;
    }
    free(phi);
    nb_energy_from_sums(q, out);
}
