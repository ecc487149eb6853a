// batch_field.h -- what batch_observe.hip needs of batch_field.hip and tidal.hip (the ensemble's field sampler).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace nb {
namespace field {

// The SoA arrays of a SimBatch (member b's rows start at b * stride) and the samples of one call: every member has n of them.
struct EnsembleParams {
    const float2 *pos;         // pos[cur]: the latest state
    const float *gm;           // G * m_j
    const uint32_t *mass_len;  // [count] M_b, on the device
    uint32_t stride;           // rows per member (a multiple of 64)
    const float *in;           // member b's samples start at b * in_stride floats
    uint32_t in_stride;        // probes: 2 * n ((x, y) pairs); map: width + height (column, then row coordinates)
    uint32_t n;                // samples per member
    uint32_t width;            // map only
    float soft;
    void *out;                 // member b's results start at b * n: float (potential), float2 (acceleration) or three floats (tidal)
};

// Phi (acceleration = false) or g at every sample of every member, one launch: grid (tiles of 128 samples / 4, count)
void launch_ensemble_sample(hipStream_t stream, const EnsembleParams &p, uint32_t count, bool acceleration, bool map);

// T = dg/dp the same way (tidal.hip): (xx, xy, yy) per sample
void launch_ensemble_tidal(hipStream_t stream, const EnsembleParams &p, uint32_t count, bool map);

}  // namespace field
}  // namespace nb
