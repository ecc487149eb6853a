// ragged_diag.hip -- the per-particle potential of a RAGGED ensemble (members of different N; include/nbody_hip.h
// nb_hip_ragged_create), the one diagnostics kernel a ragged SimBatch cannot share with a uniform one.
//
// The energy sums need nothing new: ensemble_phi_kernel (batch_diag.hip) runs them over a member's mass_len[b] massive
// receivers, which it reads from the device already, and its slab rows only have to be sized by the largest member.  The
// potential runs over ALL of a member's particles and is stored packed, so its receiver count and its output offset are
// per member: ragged_phi_kernel reads both from device arrays and is otherwise the potential half of ensemble_phi_kernel,
// statement for statement over the same diag_common.h functions -- a wave owns one tile of 128 receivers, walks its
// member's sources on the scalar-cache route (rows start 256-byte aligned: stride is a multiple of 64) in the order of
// potential_kernel's eight waves, and a wave whose tile lies beyond the member's receivers leaves at once.  Member b's
// values are therefore the bits nb_hip_ensemble_potential gives the same particles in a uniform ensemble.  No LDS, no
// barrier, vector stores only.
#include "batch_diag.h"
#include "diag_common.h"

namespace nbd {
namespace {

constexpr int WAVES_MAX = 4;   // tiles (waves) per workgroup, as ensemble_phi_kernel

template <typename T>
__device__ __forceinline__ T uniform_load(const T *p) {   // wave-uniform address, read-only for the launch: s_load
    return *(const T __attribute__((address_space(4))) *)(uintptr_t)p;
}

__global__ __launch_bounds__(WAVE * WAVES_MAX) void ragged_phi_kernel(const EnsembleDiagParams p, const uint32_t *n_len,
                                                                      const uint64_t *offsets) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t member = blockIdx.y;
    const uint32_t tile = blockIdx.x * p.waves + wid;
    const uint32_t n_src = uniform_load(p.mass_len + member);
    const uint32_t n_recv = uniform_load(n_len + member);
    const uint32_t rb = tile * TILE;                // first receiver of this wave's tile, member-local
    if (rb >= n_recv) return;
    const size_t base = (size_t)member * p.stride;
    const float2 *pos = p.pos + base;

    float px[K], py[K], r[K];
    uint32_t ri[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        uint32_t i = rb + k * WAVE + lane;
        i = i < n_recv ? i : n_recv - 1;  // tail lanes redo the last receiver; their results are dropped
        const float2 q = pos[i];
        px[k] = q.x;
        py[k] = q.y;
        r[k] = p.radius[base + i];
        ri[k] = i;
    }

    double sum[K];
    tile_potential(sum, px, py, r, ri, rb, n_src, ScalarSources{(ConstF)(uintptr_t)pos, (ConstF)(uintptr_t)(p.gm + base)});

    float *out = p.phi + uniform_load(offsets + member);
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t i = rb + k * WAVE + lane;
        if (i < n_recv) out[i] = (float)(-sum[k]);
    }
}

}  // namespace

void launch_ragged_potential(hipStream_t stream, EnsembleDiagParams p, uint32_t count, const uint32_t *n_len, const uint64_t *offsets) {
    p.tiles = ensemble_tiles(p.n);   // p.n = the largest member
    p.waves = p.tiles < (uint32_t)WAVES_MAX ? p.tiles : (uint32_t)WAVES_MAX;
    const dim3 grid((p.tiles + p.waves - 1) / p.waves, count);
    hipLaunchKernelGGL(ragged_phi_kernel, grid, dim3(WAVE * p.waves), 0, stream, p, n_len, offsets);
}

}  // namespace nbd
