/*
 * timestep_common.h -- the adaptive step-size criterion of include/nbody_adaptive.h, written once for the device kernels
 * (timestep.hip) and the host path (timestep_cpu.c).  Both sides must give the same bits, so what defines a step size lives
 * here and nowhere else:
 *   nb_timestep_q      one particle's q_i = (radius > 0 ? radius : +0) / fmaf(ax, ax, ay * ay), +inf for a particle that is skipped
 *   nb_timestep_dt     dt = fminf(fmaxf(eta * sqrtf(sqrtf(q)), dt_min), dt_max) of the minimum q
 *   nb_timestep_clip   the span clip in float64; advances t
 *   nb_timestep_count  the bookkeeping of NbAdaptiveResult for one step
 * Both compilers build this with fp contraction off (nbody_amd/csrc/Makefile): the fmaf is the only fused operation, the
 * product inside it is rounded on its own.  The division and both square roots are the correctly rounded IEEE operations on
 * both sides: gcc emits divss / sqrtss, and hipcc's default for HIP code (fp32 divide and sqrt correctly rounded, no fast-math
 * flag in HIPFLAGS) expands them to the v_div_scale / v_div_fmas / v_div_fixup and the refined v_sqrt sequences, with fp32
 * denormals kept.  The radius is clamped by a comparison, not by fmaxf: C leaves the sign of fmaxf(-0, +0) open, and a q_i of
 * -0 would lose the device's minimum (taken on the bits) where it ties the host's.  So every q_i is +0, positive or +inf: the
 * minimum over the particles is taken with `<` by the callers, +inf never wins and no q_i is a NaN or negative.
 */
#ifndef NB_TIMESTEP_COMMON_H
#define NB_TIMESTEP_COMMON_H

#include <math.h>
#include <stdint.h>

#include "nbody_adaptive.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NB_TS_FN __host__ __device__ static inline
#else
#define NB_TS_FN static inline
#endif

#define NB_TS_INF (__builtin_inff())

NB_TS_FN float nb_timestep_q(float ax, float ay, float radius) {
    const float a2 = __builtin_fmaf(ax, ax, ay * ay);
    if (!(a2 > 0.0f && a2 < NB_TS_INF)) return NB_TS_INF; /* zero, NaN or overflowed: skipped */
    return (radius > 0.0f ? radius : 0.0f) / a2; /* -0, negative and NaN radii give +0 */
}

NB_TS_FN float nb_timestep_dt(float q, float eta, float dt_min, float dt_max) {
    const float dt_raw = eta * __builtin_sqrtf(__builtin_sqrtf(q));
    return __builtin_fminf(__builtin_fmaxf(dt_raw, dt_min), dt_max);
}

NB_TS_FN float nb_timestep_clip(float dt, double span, double *t) {
    const double rem = span - *t;
    if (rem <= 0.0) return 0.0f;
    if ((double)dt >= rem) {
        *t = span;
        return (float)rem;
    }
    *t += (double)dt;
    return dt;
}

NB_TS_FN void nb_timestep_count(float dt, uint32_t *steps, uint32_t *idle_steps, float *dt_last, float *dt_smallest) {
    if (dt > 0.0f) {
        *steps += 1;
        *dt_last = dt;
        if (*dt_smallest == 0.0f || dt < *dt_smallest) *dt_smallest = dt;
    } else {
        *idle_steps += 1;
    }
}

/* NULL when cfg is acceptable, else what is wrong with it (the callers print it the library's usual way) */
NB_TS_FN const char *nb_timestep_cfg_fault(const NbAdaptive *cfg) {
    if (!(cfg->eta > 0.0f && cfg->eta < NB_TS_INF)) return "eta must be finite and > 0";
    if (!(cfg->dt_max > 0.0f && cfg->dt_max < NB_TS_INF)) return "dt_max must be finite and > 0";
    if (!(cfg->dt_min >= 0.0f && cfg->dt_min <= cfg->dt_max)) return "dt_min must be within [0, dt_max]";
    if (!(cfg->span > 0.0)) return "span must be > 0 (+inf: no clip)";
    return (const char *)0;
}

#if !defined(__HIPCC__) && !defined(__CUDACC__)
/* timestep_cpu.c (libnbody.so, not exported): the minimum q of a particle array, and the criterion without the span clip */
__attribute__((visibility("hidden"))) float nb_cpu_timestep_q(const Particle *ps, uint32_t n);
__attribute__((visibility("hidden"))) float nb_cpu_timestep(const Particle *ps, uint32_t n, const NbAdaptive *cfg);
#endif

#endif /* NB_TIMESTEP_COMMON_H */
