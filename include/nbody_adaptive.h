/*
 * nbody_adaptive.h -- adaptive time steps: the step size of every step chosen from the state itself, on the side that
 * holds it (libnbody.so).  Not part of nbody.h / galaxy.h: the reference has no counterpart.
 *
 * The criterion (one statement, nbody_amd/csrc/timestep_common.h, shared by the device kernels and the host path; float32
 * unless marked).  For every particle i < N, massless ones included:
 *
 *   a2  = fmaf(acc.x, acc.x, acc.y * acc.y)             a particle whose a2 is zero or not finite is skipped
 *   q_i = (radius_i > 0 ? radius_i : +0) / a2           IEEE division; a radius of -0, below 0 or NaN counts as +0
 *   q   = min_i q_i                                     taken with `<`; +inf when no particle contributes
 *   dt  = fminf(fmaxf(eta * sqrtf(sqrtf(q)), dt_min), dt_max)
 *
 * which is eta * sqrt(eps / |a|) with eps = sqrt(radius), because the step adds `radius` to the squared distance.  Then the
 * span clip, in float64, with t the time this call has covered so far and rem = span - t:
 *
 *   rem <= 0            dt = 0: an idle step
 *   (double)dt >= rem   dt = (float)rem and t = span exactly
 *   else                t += (double)dt
 *
 * span = +inf disables the clip.  The minimum of floats is exact in any order and everything after it is evaluated once per
 * step, so a step size is a function of the state and the configuration alone: not of the side that computed it, the grid,
 * the wave order or the kernel shape.
 *
 * `acc` is what the state holds: the acceleration the PREVIOUS step used.  A fresh world (acc = 0) therefore takes its
 * first step at dt_max; NB_ADAPT_PRIME runs one dt = 0 step first (a force evaluation that moves nothing), which is neither
 * logged nor counted.
 *
 * An idle step is a dt = 0 step of the ordinary stepper: positions and velocities compare equal afterwards, acc is
 * re-evaluated, and it costs a whole force evaluation.  The Advance calls keep idle steps rare by sizing their calls from
 * the last step size; a caller of the Update calls who sets a span pays one force evaluation for every step after it ends.
 *
 * Errors follow nbody.h: a bad configuration -- eta not finite or <= 0, dt_max not finite or <= 0, dt_min outside
 * [0, dt_max], span <= 0 or NaN, n or max_steps > 2^20 -- prints "file:line [func] ..." and abort()s before any device is
 * touched.  Sharded Worlds and ragged batches abort, naming the call.  n = 0 does nothing.
 */
#ifndef NBODY_AMD_NBODY_ADAPTIVE_H
#define NBODY_AMD_NBODY_ADAPTIVE_H

#include <stdint.h>

#include "nbody.h"
#include "nbody_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NB_ADAPT_PRIME 1u            /* NbAdaptive.flags: one unlogged dt = 0 step first, so that acc is current */
#define NB_ADAPT_CONTINUE 2u         /* GPU calls: go on from the previous adaptive call of this World / batch -- its clock and
                                        counts are kept on the device, span is measured from the call that started them, and
                                        the result is cumulative (the log is this call's).  Without a previous call: ignored */
#define NB_ADAPT_LEAPFROG 4u         /* every step is a kick-drift-kick step (include/nbody_leapfrog.h) of the size the criterion
                                        gives for the CURRENT acc: criterion, span clip, open(dt), force, close(dt).  Implies
                                        NB_ADAPT_PRIME, which is applied only when acc is not already the state's own; an idle
                                        step is open(0), force, close(0) */
#define NB_ADAPT_MAX_STEPS (1u << 20) /* steps of one call */

typedef struct NbAdaptive {
    float eta;      /* accuracy parameter, finite and > 0 */
    float dt_min;   /* 0 <= dt_min <= dt_max */
    float dt_max;   /* finite and > 0 */
    uint32_t flags; /* NB_ADAPT_PRIME | NB_ADAPT_CONTINUE | NB_ADAPT_LEAPFROG, or 0 */
    double span;    /* time one Update call may cover, > 0; +inf: no clip.  The Advance calls ignore it (they take a span) */
    uint32_t chunk; /* Advance calls only: most steps of one inner call; 0 means 64 */
    uint32_t reserved;
} NbAdaptive;

typedef struct NbAdaptiveResult {
    double elapsed;       /* sum of the step sizes in float64; == span exactly once the span is reached */
    uint32_t steps;       /* steps with dt > 0 */
    uint32_t idle_steps;  /* steps with dt = 0 */
    float dt_last;        /* the last step size > 0; 0 when there was none */
    float dt_smallest;    /* the smallest step size > 0; 0 when there was none */
} NbAdaptiveResult;

/*
 * n adaptive steps on the MI355X with the coherence rules of UpdateWorld_GPU: the array is uploaded only if the host changed
 * it, nothing returns to the host between the steps, and one copy at the end brings the log and the result.  dt_log (n
 * floats, may be NULL) receives every step's size; out may be NULL.
 */
void UpdateWorld_GPU_Adaptive(World *w, uint32_t n, const NbAdaptive *cfg, float *dt_log, NbAdaptiveResult *out);

/* The same on the host cores: per step GetWorldTimestep, the span clip, UpdateWorld_CPU(w, dt, 1). */
void UpdateWorld_CPU_Adaptive(World *w, uint32_t n, const NbAdaptive *cfg, float *dt_log, NbAdaptiveResult *out);

/* The criterion alone (no span clip) for the World's newest state: on the device when it holds it, else on the host.
 * Changes no state and moves no dirty flag. */
void GetWorldTimestep(World *w, const NbAdaptive *cfg, float *dt);

/*
 * Advance by `span`: adaptive calls are repeated until elapsed == span or max_steps steps were made.  The first call has one
 * step, every later one clamp(floor(remaining / dt_last), 1, cfg->chunk) steps; cfg->span is ignored and NB_ADAPT_PRIME
 * applies to the first call only.  dt_log (max_steps floats, may be NULL) receives the sizes of the steps made, idle ones
 * included: out->steps + out->idle_steps of them.
 */
void AdvanceWorld_GPU(World *w, double span, const NbAdaptive *cfg, uint32_t max_steps, float *dt_log, NbAdaptiveResult *out);

/*
 * The same for every member of a WorldBatch, each with its own step size at every step, in the launches that step all of
 * them.  dt_log is [n][count] (AdvanceWorldBatch_GPU: [max_steps][count]), out is [count]; either may be NULL.  The next
 * inner call of AdvanceWorldBatch_GPU is sized by the largest floor(remaining / dt_last) over the unfinished members, so
 * members that finish early take idle steps (out[b].idle_steps counts them) while the others catch up.
 */
void UpdateWorldBatch_GPU_Adaptive(WorldBatch *batch, uint32_t n, const NbAdaptive *cfg, float *dt_log, NbAdaptiveResult *out);
void AdvanceWorldBatch_GPU(WorldBatch *batch, double span, const NbAdaptive *cfg, uint32_t max_steps, float *dt_log,
                           NbAdaptiveResult *out);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_ADAPTIVE_H */
