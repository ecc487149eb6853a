/*
 * leapfrog_common.h -- the kick-drift-kick statement of include/nbody_leapfrog.h, written once for the device kernels
 * (leapfrog.hip) and the host path (leapfrog_cpu.c).  Both sides must give the same bits, so what defines a leapfrog step
 * lives here and nowhere else.  float32, every product rounded before its sum, no FMA:
 *
 *   h = 0.5f * dt
 *   open (dt):  v = v + a*h ;  x = x + v*dt        per component, a = the particle's stored acc, the drift uses the NEW v
 *   force    :  a one-step dt = 0 update of the same object: acc = F(x), and the dt = 0 integrate it carries
 *   close(dt):  v = v + a*h
 *
 * A leapfrog step of size dt is open, force, close, for every particle, massless ones included.  n steps are n of those with
 * nothing merged: a close followed by an open stays two roundings of v (v + a*h, then + a*h again is not v + a*dt in
 * float32), so that n steps in one call have the bits of the same steps in any split into calls.
 *
 * What the dt = 0 force step does to odd values, and so does a leapfrog step: its integrate is v = v + a*0, x = x + v*0.
 * A -0 velocity component or coordinate becomes +0 unless the product it is added to is -0 as well (a -0 coordinate of a
 * particle with v >= +0 becomes +0).  A non-finite v or a gives NaN: inf*0 is NaN, so an infinite velocity component turns
 * itself and its coordinate into NaN, an infinite or NaN acc turns the velocity and then the coordinate into NaN -- as in
 * any idle step of the adaptive calls.  The kicks and the drift themselves follow IEEE: inf stays inf, NaN stays NaN.
 *
 * Both compilers build this with fp contraction off (nbody_amd/csrc/Makefile); the device side also spells the operations as
 * the round-to-nearest intrinsics of kernels.hip integrate(), which no option can fuse.
 */
#ifndef NB_LEAPFROG_COMMON_H
#define NB_LEAPFROG_COMMON_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NB_LF_FN __host__ __device__ static inline
#else
#define NB_LF_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define NB_LF_MUL(a, b) __fmul_rn((a), (b))
#define NB_LF_ADD(a, b) __fadd_rn((a), (b))
#else
#define NB_LF_MUL(a, b) ((a) * (b))
#define NB_LF_ADD(a, b) ((a) + (b))
#endif

/* h of a step of size dt (exact unless dt is subnormal) */
NB_LF_FN float nb_leapfrog_half(float dt) { return NB_LF_MUL(0.5f, dt); }

/* one component of a half kick: v + a*h, the product rounded on its own */
NB_LF_FN float nb_leapfrog_kick(float v, float a, float h) { return NB_LF_ADD(v, NB_LF_MUL(a, h)); }

/* one component of the drift: x + v*dt with the velocity the opening kick left */
NB_LF_FN float nb_leapfrog_drift(float x, float v, float dt) { return NB_LF_ADD(x, NB_LF_MUL(v, dt)); }

#endif /* NB_LEAPFROG_COMMON_H */
