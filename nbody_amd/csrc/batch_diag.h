// batch_diag.h -- what batch_observe.hip and batch.hip (the SimBatch and its C-ABI) need of batch_diag.hip (the ensemble's diagnostics kernels).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace nbd {

// The SoA arrays of a SimBatch: member b's rows start at b * stride.  Members are found by block index: each has n particles.
struct EnsembleDiagParams {
    const float2 *pos;         // pos[cur]: the latest state
    const float2 *vel;
    const float *radius;
    const float *mass;
    const float *gm;           // G * m_j
    const uint32_t *mass_len;  // [count] M_b, on the device
    uint32_t n;                // particles per member
    uint32_t stride;           // rows per member (a multiple of 64)
    uint32_t tiles;            // ceil(n / 128): slab rows per member
    uint32_t waves;            // waves (= tiles) per workgroup
    float *phi;                // potential: [count][n]; else NULL
    double *slab;              // energy: [count][tiles][8]; else NULL
};

// The potential of a ragged ensemble: member b has n_len[b] particles (n = the largest member) and its values go to
// phi + offsets[b]; both arrays on the device.  The kernel is one template over the two parameter types.
struct RaggedDiagParams : EnsembleDiagParams {
    const uint32_t *n_len;     // [count]
    const uint64_t *offsets;   // [count]
};

uint32_t ensemble_tiles(uint32_t n);   // 128-receiver tiles of one member
// Phi of every particle of every member (p.phi) or the per-tile energy rows of every member's M_b massive receivers (p.slab).
// With n_len (and offsets) the members are those of a ragged ensemble, p.phi only; the energy rows of a ragged ensemble are
// launched without: they are sized by p.n = the largest member.
void launch_ensemble_potential(hipStream_t stream, EnsembleDiagParams p, uint32_t count, const uint32_t *n_len = nullptr,
                               const uint64_t *offsets = nullptr);
// out[b][8] = member b's rows added in the fixed order of energy_reduce_kernel
void launch_ensemble_reduce(hipStream_t stream, const double *slab, const uint32_t *mass_len, uint32_t tiles, uint32_t count,
                            double *out);

}  // namespace nbd
