/*
 * nbody_leapfrog.h -- leapfrog (kick-drift-kick) steps, fixed and adaptive (libnbody.so).  Not part of nbody.h / galaxy.h:
 * the reference steps with semi-implicit Euler and nothing else.
 *
 * The statement (one place, nbody_amd/csrc/leapfrog_common.h, shared by the device kernels and the host path).  float32,
 * every product rounded before its sum, no FMA:
 *
 *   h = 0.5f * dt
 *   open (dt):  v = v + a*h ;  x = x + v*dt        per component, a = the particle's stored acc
 *   force    :  what a one-step dt = 0 update of the same object does: acc = F(x), and the dt = 0 integrate it carries
 *   close(dt):  v = v + a*h
 *
 * A leapfrog step of size dt is open, force, close, for every particle, massless ones included.  n steps are n of those with
 * nothing merged: a close followed by an open stays two roundings of v, so n steps in one call have the bits of the same
 * steps in any split into calls.  The scheme is second order and time-reversible at the cost of the same one force
 * evaluation per step as UpdateWorld_CPU / UpdateWorld_GPU.
 *
 * open needs a = F(x) of the state it starts from.  Every object remembers whether that holds: it does right after a leapfrog
 * call on the same side, and anything else that changes the particles -- a new array, a transfer between host and device,
 * an Euler update, an Euler adaptive call -- clears it.  A call that finds it cleared first runs one dt = 0 update, unlogged
 * and uncounted: the first call of a sequence costs n + 1 force evaluations, every following one n.
 *
 * What the dt = 0 force step does to odd values: a -0 coordinate of a particle with v >= +0 becomes +0, and a non-finite v or
 * a gives NaN (inf * 0), as in any idle step of the adaptive calls.
 *
 * Adaptive leapfrog: NB_ADAPT_LEAPFROG in NbAdaptive.flags (include/nbody_adaptive.h).  UpdateWorld_GPU_Adaptive,
 * UpdateWorld_CPU_Adaptive, AdvanceWorld_GPU and the WorldBatch calls then make every step a leapfrog step of the size the
 * criterion gives for the current acc -- which is now the state's own, so NB_ADAPT_PRIME is implied and never applied twice.
 *
 * Errors follow nbody.h: NULL arguments print "file:line [func] ..." and abort().  Sharded Worlds (GPU calls) and ragged
 * batches abort, naming the call, before any device is touched.  n = 0 does nothing.
 */
#ifndef NBODY_AMD_NBODY_LEAPFROG_H
#define NBODY_AMD_NBODY_LEAPFROG_H

#include <stdint.h>

#include "nbody.h"
#include "nbody_adaptive.h"
#include "nbody_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* n leapfrog steps of size dt on the MI355X with the coherence rules of UpdateWorld_GPU: the array is uploaded only if the
 * host changed it, and nothing returns to the host between the steps. */
void UpdateWorld_GPU_Leapfrog(World *w, float dt, uint32_t n);

/* The same on the host cores: the shared statement around UpdateWorld_CPU(w, 0, 1), with UpdateWorld_CPU's coherence rules. */
void UpdateWorld_CPU_Leapfrog(World *w, float dt, uint32_t n);

/* n leapfrog steps of every member of a WorldBatch in the launches that step all of them: one dt for all, or dt[count]. */
void UpdateWorldBatch_GPU_Leapfrog(WorldBatch *batch, float dt, uint32_t n);
void UpdateWorldBatch_GPU_Leapfrog_dts(WorldBatch *batch, const float *dt, uint32_t n);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_LEAPFROG_H */
