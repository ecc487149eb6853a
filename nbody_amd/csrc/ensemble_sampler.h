// ensemble_sampler.h -- the sampler of an ensemble, for the translation units that instantiate it: batch_field.hip
// (Potential, Acceleration) and tidal.hip (Tidal).  One kernel shape and its launcher; what the kernel computes and how it
// finds a member is stated at the head of batch_field.hip.  A template over the quantity policy, so each translation unit
// holds the kernels of its own policies only.  Include it from a .hip file.
#pragma once

#include "batch_field.h"
#include "field_kernels.h"

namespace nb {
namespace field {
namespace {

template <typename T>
__device__ __forceinline__ T uniform_load(const T *p) {   // wave-uniform address, read-only for the launch: s_load
    return *(const T __attribute__((address_space(4))) *)(uintptr_t)p;
}

// 1..4 waves of one member, one tile each, at most 64 VGPRs.  The member's view of the call is a local Params: a reference
// to the by-value kernel argument would cost the result stores their global address space (batch_diag.hip).  The tile's
// statements are sample_wave_kernel's, written out here: as one function called from both, field.hip's kernels come out
// with other register assignments, and that file's instructions are held as they are.
template <typename Q, bool MAP>
__global__ __launch_bounds__(WAVE * WAVES_MAX, 8) void ensemble_sample_kernel(const EnsembleParams e) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t rb = (blockIdx.x * WAVES_MAX + wid) * TILE;   // first sample of this wave's tile, member-local
    if (rb >= e.n) return;
    const uint32_t member = blockIdx.y;
    const size_t base = (size_t)member * e.stride;

    Params p;
    p.pos = e.pos + base;
    p.src_gm = e.gm + base;
    p.n_src = uniform_load(e.mass_len + member);
    p.in = e.in + (size_t)member * e.in_stride;
    p.n = e.n;
    p.width = e.width;
    p.soft = e.soft;
    p.out = static_cast<typename Q::Out *>(e.out) + (size_t)member * e.n;

    float px[K], py[K];
    double sum[Q::C][K];
    load_samples<MAP>(p, rb, lane, px, py);
#pragma unroll
    for (int k = 0; k < K; k++)
        for (int c = 0; c < Q::C; c++) sum[c][k] = 0.0;
    // the eight source slices of sample_split_kernel's waves, one after another: sample_wave_kernel's statements
#pragma unroll 1
    for (uint32_t w = 0; w < W; w++) {
        double s[Q::C][K];
#pragma unroll
        for (int k = 0; k < K; k++)
            for (int c = 0; c < Q::C; c++) s[c][k] = 0.0;
        slice_sum<Q>(s, px, py, p, w);
#pragma unroll
        for (int k = 0; k < K; k++)
            for (int c = 0; c < Q::C; c++) sum[c][k] += s[c][k];
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        double t[Q::C];
#pragma unroll
        for (int c = 0; c < Q::C; c++) t[c] = sum[c][k];
        store_sample<Q>(p, rb + k * WAVE + lane, px[k], py[k], t);
    }
}

template <typename Q>
void launch(hipStream_t stream, const EnsembleParams &p, uint32_t count, bool map) {
    const uint32_t tiles = (p.n + TILE - 1) / TILE;
    const uint32_t waves = tiles < (uint32_t)WAVES_MAX ? tiles : (uint32_t)WAVES_MAX;
    const dim3 grid((tiles + WAVES_MAX - 1) / WAVES_MAX, count), block(WAVE * waves);
    if (map)
        hipLaunchKernelGGL((ensemble_sample_kernel<Q, true>), grid, block, 0, stream, p);
    else
        hipLaunchKernelGGL((ensemble_sample_kernel<Q, false>), grid, block, 0, stream, p);
}

}  // namespace
}  // namespace field
}  // namespace nb
