// field_sampler.h -- the sampler of one pipeline, for the translation units that instantiate it: field.hip (Potential,
// Acceleration) and tidal.hip (Tidal).  The two kernel shapes, the one rule that picks between them and the host side of a
// call: its checks, and its launch inside pipeline_internal.h's read_call.  The statements are field_kernels.h's; the
// definitions and the summation order are stated at the head of field.hip.  The kernels are templates over the quantity policy, so each translation unit
// holds the kernels of its own policies only.  Include it from a .hip file after field_kernels.h.
#pragma once

#include "pipeline_internal.h"
#include "diag_common.h"
#include "field_common.h"
#include "field_kernels.h"
#include "nbody_hip_tuning.h"

#include <math.h>

#include <vector>

namespace nb {
namespace field {

using namespace nbd;

// 512 threads, at most 64 VGPRs (8 waves per SIMD: four workgroups per CU, 8 KiB of LDS each per running sum), as
// potential_kernel.
template <typename Q, bool MAP>
__global__ __launch_bounds__(WAVE * W, 8) void sample_split_kernel(const Params p) {
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t rb = blockIdx.x * TILE;  // first sample of the tile

    float px[K], py[K];
    double s[Q::C][K];
    load_samples<MAP>(p, rb, lane, px, py);
#pragma unroll
    for (int k = 0; k < K; k++)
        for (int c = 0; c < Q::C; c++) s[c][k] = 0.0;
    slice_sum<Q>(s, px, py, p, wid);

    // the W slices in wave order (float64); thread t of the first two waves holds sample rb + t's coordinates in slot
    // t / 64 of lane t % 64, which is its own slot k = wid
    __shared__ double part[Q::C][W][TILE];
#pragma unroll
    for (int k = 0; k < K; k++)
        for (int c = 0; c < Q::C; c++) part[c][wid][k * WAVE + lane] = s[c][k];
    __syncthreads();
    if (tid < TILE) {
        double sum[Q::C];
#pragma unroll
        for (int c = 0; c < Q::C; c++) sum[c] = 0.0;
#pragma unroll
        for (int w = 0; w < W; w++)
            for (int c = 0; c < Q::C; c++) sum[c] += part[c][w][tid];
        store_sample<Q>(p, rb + tid, wid ? px[1] : px[0], wid ? py[1] : py[0], sum);
    }
}
static_assert(K == 2, "sample_split_kernel's finishing threads pick their sample by wave index 0 / 1");

// 1..4 waves, one tile each, at most 64 VGPRs.
template <typename Q, bool MAP>
__global__ __launch_bounds__(WAVE * WAVES_MAX, 8) void sample_wave_kernel(const Params p) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t rb = (blockIdx.x * WAVES_MAX + wid) * TILE;   // first sample of this wave's tile
    if (rb >= p.n) return;

    float px[K], py[K];
    double sum[Q::C][K];
    load_samples<MAP>(p, rb, lane, px, py);
#pragma unroll
    for (int k = 0; k < K; k++)
        for (int c = 0; c < Q::C; c++) sum[c][k] = 0.0;
    // the eight source slices of the split kernel's waves, one after another
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

}  // namespace field
}  // namespace nb

namespace {

using namespace nbi;
namespace fd = nb::field;

// The one place that picks the kernel shape.  One wave per tile pays when both hold: the world has at most 2 blocks of 256
// sources (most of a split workgroup's 8 waves would walk nothing) and there are enough tiles to fill the chip with one
// wave each.  Measured for the Phi pair (tools/field_probe.py, profiles/r12_field_probe.json; wave / split device time): at
// 1280 x 720 (7 200 tiles) 0.51 - 0.55 at 1 block, 0.80 at 2, 1.12 - 1.19 from 4 blocks up; at 256 x 256 (512 tiles, a
// sixteenth of the chip's 8 192 wave slots) the split is ahead at every M, by 1.05 - 1.06 at 1 block and 1.8 - 3.8 beyond.
// 3 blocks and tile counts between 512 and 7 200 are not measured: the rule keeps the split there, and puts the tile bound
// at half the wave slots.  The g pair (10 VALU instructions per pair against the Phi pair's 6) inherited both thresholds;
// measured since (tools/gravity_probe.py, profiles/r13_gravity_probe.json): at 1280 x 720 0.54 - 0.59 at 1 block, 0.85 at 2,
// 0.97 at 3, 1.11 - 1.16 from 4 blocks up; at 256 x 256 the split is ahead at every M, 1.03 - 1.04 at 1 block and 1.76 - 3.58
// beyond.  The same crossover, so one pair of thresholds serves both.  The T pair (14 VALU instructions) inherits them too;
// tools/tidal_probe.py reports where its crossover lies.
constexpr uint32_t WAVE_SHAPE_BLOCKS_MAX = 2;
constexpr uint32_t WAVE_SHAPE_TILES_MIN = 4096;

inline bool pick_wave_shape(int shape_knob, uint32_t mass_len, uint32_t tiles) {
    if (shape_knob) return shape_knob == 2;
    const uint32_t nblocks = (mass_len + nbd::BLOCK - 1) / nbd::BLOCK;
    return nblocks <= WAVE_SHAPE_BLOCKS_MAX && tiles >= WAVE_SHAPE_TILES_MIN;
}

template <typename Q, bool MAP>
void launch(SimPipeline *s, const fd::Params &p) {
    const uint32_t tiles = (p.n + nbd::TILE - 1) / nbd::TILE;
    if (pick_wave_shape(s->*Q::SHAPE, p.n_src, tiles))
        hipLaunchKernelGGL((fd::sample_wave_kernel<Q, MAP>), dim3((tiles + fd::WAVES_MAX - 1) / fd::WAVES_MAX),
                           dim3(nbd::WAVE * fd::WAVES_MAX), 0, s->stream, p);
    else
        hipLaunchKernelGGL((fd::sample_split_kernel<Q, MAP>), dim3(tiles), dim3(nbd::WAVE * nbd::W), 0, s->stream, p);
    ASSERT_HIP(hipGetLastError(), "%s kernel launch (%u samples, %u sources)", Q::NOUN, p.n, p.n_src);
}

// one read_call: upload `in_floats` floats (the probes' (x, y) pairs, or a map's width column + height row coordinates), evaluate
// n samples into Q::OUT floats each, copy them to `out`
template <typename Q>
void run(SimPipeline *s, const char *what, bool map, const float *in, size_t in_floats, uint32_t n, uint32_t width, float softening,
         typename Q::Out *out) {
    const size_t out_bytes = (size_t)n * sizeof(typename Q::Out);
    read_call(s, s->read.iv, what, in, in_floats * sizeof(float), out_bytes, out, out_bytes, [&](void *in_dev, void *work) -> const void * {
        fd::Params p{};
        p.pos = s->pos[s->cur];
        p.src_gm = s->src_gm;
        p.n_src = s->data.mass_len;
        p.in = static_cast<const float *>(in_dev);
        p.n = n;
        p.width = width;
        p.soft = softening;
        p.out = work;
        if (map)
            launch<Q, true>(s, p);
        else
            launch<Q, false>(s, p);
        return work;
    });
}

inline void check(const char *noun, float softening, uint64_t samples) {
    const char *fault = nb_field_fault(softening, samples);
    NB_ASSERT(fault == nullptr, "invalid %s call (softening %g, %llu points): %s", noun, (double)softening, (unsigned long long)samples, fault);
}

template <typename Q>
void sample_at(SimPipeline *s, const char *what, const float *points, uint32_t n, float softening, typename Q::Out *out) {
    check_diag(s, what);
    check(Q::NOUN, softening, n);
    NB_ASSERT((points != nullptr && out != nullptr) || n == 0, "NULL points or result");
    if (n == 0) {
        s->read.iv.clear();
        return;
    }
    run<Q>(s, what, false, points, (size_t)n * 2, n, 0, softening, out);
}

// a map is the probes product at the view's pixel centres: width column coordinates, then height row coordinates
template <typename Q>
void sample_map(SimPipeline *s, const char *what, const RenderView *view, float softening, typename Q::Out *out) {
    check_diag(s, what);
    check_view(view);
    check(Q::NOUN, softening, (uint64_t)view->width * view->height);
    NB_ASSERT(out != nullptr, "NULL %s map", Q::NOUN);
    std::vector<float> coords((size_t)view->width + view->height);
    nb_render_pixel_centres(view, coords.data(), coords.data() + view->width);
    run<Q>(s, what, true, coords.data(), coords.size(), view->width * view->height, view->width, softening, out);
}

}  // namespace
