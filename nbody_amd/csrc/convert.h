// convert.h -- the utility kernels around the force path (convert.hip): AoS <-> SoA split / merge of the reference
// Particle layout (include/nbody.h), inert pads, G*m, fills; for one world and for whole ensembles.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nb {

// whole-ensemble converters: member-major AoS <-> SoA [count][stride] (member b's rows at b * stride); split also writes
// G*m.  Without n_len every member has n records, member b's at aos[b * n]; with it (a ragged ensemble) member b's
// n_len[b] records sit packed at aos[offsets[b]] and n is the largest member.  offsets, n_len and mass_len are device arrays.
void launch_batch_split(hipStream_t st, const void *aos, const uint64_t *offsets, const uint32_t *n_len, const uint32_t *mass_len,
                        uint32_t count, uint32_t n, uint32_t stride, float2 *pos, float2 *vel, float2 *acc, float *radius, float *mass,
                        float *gm, float g);
void launch_batch_merge(hipStream_t st, void *aos, const uint64_t *offsets, const uint32_t *n_len, uint32_t first, uint32_t count,
                        uint32_t n, uint32_t stride, const float2 *pos, const float2 *vel, const float2 *acc, const float *radius,
                        const float *mass);
void launch_batch_fill(hipStream_t st, float *dst, uint32_t count, float value);   // dst[0 .. count) = value, in stream order

// ragged ensembles: to[rows of members[0 .. count)] = from[the same rows]: position rows across the two ping-pong buffers
void launch_ragged_copy_rows(hipStream_t st, const uint32_t *members, const uint32_t *n_len, uint32_t count, uint32_t max_n,
                             uint32_t stride, const float2 *from, float2 *to);

// AoS <-> SoA converters (reference Particle layout, include/nbody.h).
// split: aos[first .. first+count) -> soa slots [slot0 .. slot0+count)
void launch_split(hipStream_t st, const void *aos, uint32_t first, uint32_t count, float2 *pos, float2 *vel, float2 *acc,
                  float *radius, float *mass, uint32_t slot0);
// fill pad slots so that they are inert sources / harmless receivers
void launch_fill_pad(hipStream_t st, float2 *pos, float2 *vel, float2 *acc, float *radius, float *mass, uint32_t slot0,
                     uint32_t count);
// gm[j] = g * mass[j] for j < count (0 where mass <= 0); g = the host's NB_G, the only place the value is written down
void launch_make_gm(hipStream_t st, const float *mass, float *gm, uint32_t count, float g);
// merge: soa slots [slot0 .. slot0+count) -> aos[first .. first+count)
void launch_merge(hipStream_t st, void *aos, uint32_t first, uint32_t count, const float2 *pos, const float2 *vel,
                  const float2 *acc, const float *radius, const float *mass, uint32_t slot0);
// *dst = value, in stream order (the step-size upload): one thread
void launch_set_scalar(hipStream_t st, float *dst, float value);
// sharded upload: both gathered source arrays + G*m from the AoS world; slots in [mass_len, n_src) become inert pads
void launch_split_sources(hipStream_t st, const void *aos, uint32_t mass_len, uint32_t n_src, float2 *pos0, float2 *pos1,
                          float *gm, float g);

}  // namespace nb
