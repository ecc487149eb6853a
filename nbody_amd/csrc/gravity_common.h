/*
 * gravity_common.h -- what the two paths of include/nbody_gravity.h share: the argument checks (field_common.h's, the
 * limits are the same) and the host path's entry points (hidden, libnbody.so).  The pixel centres of a map come from
 * render_common.h's nb_render_pixel_centres on both paths.
 */
#ifndef NB_GRAVITY_COMMON_H
#define NB_GRAVITY_COMMON_H

#include "nbody_gravity.h"
#include "field_common.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gravity_cpu.c (libnbody.so, not exported): float64 on the host, OpenMP over the samples, every sum in index order */
__attribute__((visibility("hidden"))) void nb_cpu_acceleration_at(const Particle *ps, uint32_t mass_len, const V2 *points, uint32_t n,
                                                                  float softening, V2 *acc);
__attribute__((visibility("hidden"))) void nb_cpu_acceleration_map(const Particle *ps, uint32_t mass_len, const RenderView *view,
                                                                   float softening, V2 *acc);

#ifdef __cplusplus
}
#endif

#endif /* NB_GRAVITY_COMMON_H */
