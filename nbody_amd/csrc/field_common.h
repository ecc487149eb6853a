/*
 * field_common.h -- what the two paths of include/nbody_field.h, include/nbody_gravity.h and include/nbody_tidal.h share: the
 * argument checks of a field call (the limits of the three headers are the same), written once for the GPU path (field.hip) and the host path
 * (field_cpu.c), and the host path's entry points (hidden, libnbody.so).  The pixel centres of a map come from
 * render_common.h's nb_render_pixel_centres on both paths.
 */
#ifndef NB_FIELD_COMMON_H
#define NB_FIELD_COMMON_H

#include "nbody_field.h"
#include "nbody_gravity.h"
#include "nbody_tidal.h"
#include "render_common.h"

/* NULL when the softening and the sample count are within the limits of include/nbody_field.h, else what is wrong */
static inline const char *nb_field_fault(float softening, uint64_t samples) {
    if (!nb_render_finite(softening) || !(softening > 0.0f)) return "softening must be finite and > 0";
    if (samples > NB_FIELD_MAX_POINTS) return "at most 2^24 points per call";
    return NULL;
}

#ifdef __cplusplus
extern "C" {
#endif

/* field_cpu.c (libnbody.so, not exported): float64 on the host, OpenMP over the samples, every sum in index order */
__attribute__((visibility("hidden"))) void nb_cpu_potential_at(const Particle *ps, uint32_t mass_len, const V2 *points, uint32_t n,
                                                               float softening, float *phi);
__attribute__((visibility("hidden"))) void nb_cpu_potential_map(const Particle *ps, uint32_t mass_len, const RenderView *view,
                                                                float softening, float *phi);
__attribute__((visibility("hidden"))) void nb_cpu_acceleration_at(const Particle *ps, uint32_t mass_len, const V2 *points, uint32_t n,
                                                                  float softening, V2 *acc);
__attribute__((visibility("hidden"))) void nb_cpu_acceleration_map(const Particle *ps, uint32_t mass_len, const RenderView *view,
                                                                   float softening, V2 *acc);
__attribute__((visibility("hidden"))) void nb_cpu_tidal_at(const Particle *ps, uint32_t mass_len, const V2 *points, uint32_t n,
                                                           float softening, TidalTensor *t);
__attribute__((visibility("hidden"))) void nb_cpu_tidal_map(const Particle *ps, uint32_t mass_len, const RenderView *view,
                                                            float softening, TidalTensor *t);

#ifdef __cplusplus
}
#endif

#endif /* NB_FIELD_COMMON_H */
