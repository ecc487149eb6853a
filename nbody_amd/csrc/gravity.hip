// gravity.hip -- the acceleration field of the state a pipeline holds at points that are not particles: probes the caller
// chooses and the pixel centres of a view (include/nbody_gravity.h; nb_hip_acceleration_at / nb_hip_acceleration_map).
//
// Definitions (also in include/nbody_gravity.h and DESIGN.md section 3): for a sample p and a softening s
//     g(p; s) = sum_{j < M} G*m_j (x_j - p) / (|x_j - p|^2 + s)^(3/2),      G*m_j = src_gm[j], M = mass_len
// = what a step stores in acc[] for a massless receiver at p with radius s.  A sample is never a source, so no term is
// excluded; a sample exactly on a source gets (x_j - p) = 0 over a finite denominator, a zero term.
//
// The pair is the step kernels' own statement (interaction_asm.h NB_INTERACTION2_ASM: the lane's two samples against one
// wave-uniform source, both v_rsq_f32 inside one raised-priority window) with r0 = r1 = s.  The summation is field.hip's
// and diag_common.h's: fp32 sums from 0.0f over a block of 256 sources with j ascending, float64 totals per block, and the
// eight source slices [w * per, (w + 1) * per), per = ceil(ceil(M / 256) / 8), added in wave order from 0.0, each component
// rounded once to float32.  A result is defined by that order, not by which wave adds what, so the two kernels below give
// the same bits:
//   gravity_split_kernel   the 8 waves of a workgroup share one tile of 128 samples (64 lanes x 2) and each walks 1/8 of
//                          the source blocks; the slices meet in LDS as float64.  For large M.
//   gravity_wave_kernel    every wave owns a tile and walks the eight slices itself.  No LDS, no barrier.  For small worlds
//                          under large images.
// pick_wave_shape() below chooses between them, in one place.  Sources stay on the scalar-cache route in both
// (s_load_dwordx16 / x8, 8 per fetch, single sources for a ragged end, as diag_common.h's block_sum).  MAP = true: a lane
// forms its two samples from the view's column and row coordinates (sample i = py * width + px reads xs[px] and ys[py]; the
// host computed both arrays, render_common.h); MAP = false: it loads them.  A sample with a non-finite coordinate stores
// (NaN, NaN).  No atomics; vector stores only, one float2 per sample.
#include "pipeline_internal.h"
#include "diag_common.h"
#include "gravity_common.h"
#include "interaction_asm.h"
#include "nbody_hip_tuning.h"

#include <math.h>

namespace nb {
namespace gravity {

using namespace nbd;

constexpr int WAVES_MAX = 4;   // gravity_wave_kernel: tiles (waves) per workgroup

struct GravityParams {
    const float2 *pos;     // pos[cur]: the latest state
    const float *src_gm;   // G * m_j, j < n_src
    uint32_t n_src;        // sources [0, M)
    const float *in;       // probes: (x, y) pairs; map: width column coordinates, then height row coordinates
    uint32_t n;            // samples
    uint32_t width;        // map only
    float soft;
    float2 *acc;           // g of sample i, i < n
};

static_assert(K == 2, "NB_INTERACTION2_ASM is the statement for two samples per lane");

// one source (wave-uniform, SGPRs) against the lane's two samples: the step kernels' statement, both radii = s
__device__ __forceinline__ void pair2(float (&ax)[K], float (&ay)[K], const float (&px)[K], const float (&py)[K], float s, float sx,
                                      float sy, float g) {
    asm(NB_INTERACTION2_ASM
        : [ax0] "+v"(ax[0]), [ay0] "+v"(ay[0]), [ax1] "+v"(ax[1]), [ay1] "+v"(ay[1])
        : [sx] "s"(sx), [sy] "s"(sy), [g] "s"(g), [px0] "v"(px[0]), [py0] "v"(py[0]), [r0] "v"(s), [px1] "v"(px[1]), [py1] "v"(py[1]),
          [r1] "v"(s)
        : NB_CLOBBERS2);
}

// Sources [j0, j1) of one block added to ax[], ay[]: 8 per scalar fetch, then single sources for a ragged end (the walk of
// diag_common.h's block_sum, one register set).
__device__ __forceinline__ void block_sum2(float (&ax)[K], float (&ay)[K], const float (&px)[K], const float (&py)[K], float s, ConstF sp,
                                           ConstF sg, uint32_t j0, uint32_t j1) {
    uint32_t j = j0;
    for (; j + 8 <= j1; j += 8) {
        const v16f P = cload<v16f>(sp + 2 * (size_t)j);
        const v8f G = cload<v8f>(sg + j);
#pragma unroll
        for (int u = 0; u < 8; u++) pair2(ax, ay, px, py, s, P[2 * u], P[2 * u + 1], G[u]);
    }
    for (; j < j1; j++) pair2(ax, ay, px, py, s, sp[2 * (size_t)j], sp[2 * (size_t)j + 1], sg[j]);
}

// blocks [b_lo, b_hi) into the float64 slice sums sx[], sy[] (from whatever they hold), one fp32 block sum at a time
__device__ __forceinline__ void slice_sum(double (&sx)[K], double (&sy)[K], const float (&px)[K], const float (&py)[K], float s, ConstF sp,
                                          ConstF sg, uint32_t b_lo, uint32_t b_hi, uint32_t n_src) {
    float ax[K], ay[K];
#pragma unroll
    for (int k = 0; k < K; k++) ax[k] = ay[k] = 0.0f;
#pragma unroll 1
    for (uint32_t b = b_lo; b < b_hi; b++) {
        const uint32_t j0 = b * BLOCK, j1 = min(j0 + BLOCK, n_src);
        block_sum2(ax, ay, px, py, s, sp, sg, j0, j1);
#pragma unroll
        for (int k = 0; k < K; k++) {
            sx[k] += (double)ax[k];
            sy[k] += (double)ay[k];
            ax[k] = ay[k] = 0.0f;
        }
    }
}

// the K samples of this lane: tile rows lane and lane + 64; tail lanes redo the last sample, their results are dropped
template <bool MAP>
__device__ __forceinline__ void load_samples(const GravityParams &p, uint32_t rb, uint32_t lane, float (&px)[K], float (&py)[K]) {
#pragma unroll
    for (int k = 0; k < K; k++) {
        uint32_t i = rb + k * WAVE + lane;
        i = i < p.n ? i : p.n - 1;
        if constexpr (MAP) {
            const uint32_t row = i / p.width, col = i - row * p.width;
            px[k] = p.in[col];
            py[k] = p.in[p.width + row];
        } else {
            const float2 q = reinterpret_cast<const float2 *>(p.in)[i];
            px[k] = q.x;
            py[k] = q.y;
        }
    }
}

__device__ __forceinline__ void store_sample(const GravityParams &p, uint32_t i, float x, float y, double gx, double gy) {
    if (i >= p.n) return;
    const bool finite = nb_render_finite(x) && nb_render_finite(y);
    const float nan = __builtin_nanf("");
    p.acc[i] = finite ? make_float2((float)gx, (float)gy) : make_float2(nan, nan);
}

// 512 threads, at most 64 VGPRs (8 waves per SIMD: four workgroups per CU, 16 KiB of LDS each).
template <bool MAP>
__global__ __launch_bounds__(WAVE * W, 8) void gravity_split_kernel(const GravityParams p) {
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t rb = blockIdx.x * TILE;  // first sample of the tile

    float px[K], py[K];
    double sx[K], sy[K];
    load_samples<MAP>(p, rb, lane, px, py);
#pragma unroll
    for (int k = 0; k < K; k++) sx[k] = sy[k] = 0.0;

    // this wave's slice of the sources, in whole blocks
    const uint32_t nblocks = (p.n_src + BLOCK - 1) / BLOCK;
    const uint32_t per_wave = (nblocks + W - 1) / W;
    const uint32_t b_lo = min(wid * per_wave, nblocks);
    const uint32_t b_hi = min(b_lo + per_wave, nblocks);
    slice_sum(sx, sy, px, py, p.soft, (ConstF)(uintptr_t)p.pos, (ConstF)(uintptr_t)p.src_gm, b_lo, b_hi, p.n_src);

    // the W slices in wave order (float64); thread t of the first two waves holds sample rb + t's coordinates in slot
    // t / 64 of lane t % 64, which is its own slot k = wid
    __shared__ double part_x[W][TILE], part_y[W][TILE];
#pragma unroll
    for (int k = 0; k < K; k++) {
        part_x[wid][k * WAVE + lane] = sx[k];
        part_y[wid][k * WAVE + lane] = sy[k];
    }
    __syncthreads();
    if (tid < TILE) {
        double gx = 0.0, gy = 0.0;
#pragma unroll
        for (int w = 0; w < W; w++) {
            gx += part_x[w][tid];
            gy += part_y[w][tid];
        }
        store_sample(p, rb + tid, wid ? px[1] : px[0], wid ? py[1] : py[0], gx, gy);
    }
}

// 1..4 waves, one tile each, at most 64 VGPRs.
template <bool MAP>
__global__ __launch_bounds__(WAVE * WAVES_MAX, 8) void gravity_wave_kernel(const GravityParams p) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t rb = (blockIdx.x * WAVES_MAX + wid) * TILE;   // first sample of this wave's tile
    if (rb >= p.n) return;

    float px[K], py[K];
    double gx[K], gy[K];
    load_samples<MAP>(p, rb, lane, px, py);
#pragma unroll
    for (int k = 0; k < K; k++) gx[k] = gy[k] = 0.0;
    // the eight source slices of the split kernel's waves, one after another
    const uint32_t nblocks = (p.n_src + BLOCK - 1) / BLOCK;
    const uint32_t per = (nblocks + W - 1) / W;
#pragma unroll 1
    for (uint32_t w = 0; w < W; w++) {
        const uint32_t b_lo = min(w * per, nblocks);
        const uint32_t b_hi = min(b_lo + per, nblocks);
        double sx[K], sy[K];
#pragma unroll
        for (int k = 0; k < K; k++) sx[k] = sy[k] = 0.0;
        slice_sum(sx, sy, px, py, p.soft, (ConstF)(uintptr_t)p.pos, (ConstF)(uintptr_t)p.src_gm, b_lo, b_hi, p.n_src);
#pragma unroll
        for (int k = 0; k < K; k++) {
            gx[k] += sx[k];
            gy[k] += sy[k];
        }
    }
#pragma unroll
    for (int k = 0; k < K; k++) store_sample(p, rb + k * WAVE + lane, px[k], py[k], gx[k], gy[k]);
}

}  // namespace gravity
}  // namespace nb

namespace {

using namespace nbi;
namespace gv = nb::gravity;

// The one place that picks the kernel shape.  One wave per tile when the world has at most 2 blocks of 256 sources (most of
// a split workgroup's 8 waves would walk nothing) and the call has enough tiles to fill the chip with one wave each.  Both
// thresholds are inherited from field.hip's pick_wave_shape (measured there for the Phi pair, profiles/r12_field_probe.json)
// and are not yet measured for this pair body (10 VALU instructions per pair against the Phi pair's 6).
constexpr uint32_t WAVE_SHAPE_BLOCKS_MAX = 2;
constexpr uint32_t WAVE_SHAPE_TILES_MIN = 4096;

bool pick_wave_shape(const SimPipeline *s, uint32_t tiles) {
    if (s->gravity_shape) return s->gravity_shape == 2;
    const uint32_t nblocks = (s->data.mass_len + nbd::BLOCK - 1) / nbd::BLOCK;
    return nblocks <= WAVE_SHAPE_BLOCKS_MAX && tiles >= WAVE_SHAPE_TILES_MIN;
}

template <typename T>
void grow(SimPipeline *s, T *&buf, size_t &cap, size_t need, const char *what) {
    if (cap >= need && buf) return;
    if (buf) {
        ASSERT_HIP(hipStreamSynchronize(s->stream), "sync before regrowing the %s", what);
        dev_free(buf);
    }
    buf = dev_alloc<T>(need);
    cap = need;
}

template <bool MAP>
void launch(SimPipeline *s, const gv::GravityParams &p) {
    const uint32_t tiles = (p.n + nbd::TILE - 1) / nbd::TILE;
    if (pick_wave_shape(s, tiles))
        hipLaunchKernelGGL(gv::gravity_wave_kernel<MAP>, dim3((tiles + gv::WAVES_MAX - 1) / gv::WAVES_MAX), dim3(nbd::WAVE * gv::WAVES_MAX),
                           0, s->stream, p);
    else
        hipLaunchKernelGGL(gv::gravity_split_kernel<MAP>, dim3(tiles), dim3(nbd::WAVE * nbd::W), 0, s->stream, p);
    ASSERT_HIP(hipGetLastError(), "gravity kernel launch (%u samples, %u sources)", p.n, p.n_src);
}

// upload `in_floats` floats, evaluate n samples, one copy of the result, one sync; `in` stays alive until the sync
void run_gravity(SimPipeline *s, bool map, const float *in, size_t in_floats, uint32_t n, uint32_t width, float softening, float *acc) {
    use_device();
    grow(s, s->gravity_in, s->gravity_in_cap, in_floats, "gravity samples");
    grow(s, s->gravity_acc, s->gravity_acc_cap, (size_t)n, "gravity result");
    ASSERT_HIP(hipMemcpyAsync(s->gravity_in, in, in_floats * sizeof(float), hipMemcpyHostToDevice, s->stream), "H2D of the gravity samples");
    gv::GravityParams p{};
    p.pos = s->pos[s->cur];
    p.src_gm = s->src_gm;
    p.n_src = s->data.mass_len;
    p.in = s->gravity_in;
    p.n = n;
    p.width = width;
    p.soft = softening;
    p.acc = s->gravity_acc;
    begin_diag(s);
    if (map)
        launch<true>(s, p);
    else
        launch<false>(s, p);
    end_diag(s);
    ASSERT_HIP(hipMemcpyAsync(acc, s->gravity_acc, (size_t)n * sizeof(float2), hipMemcpyDeviceToHost, s->stream), "D2H of %u accelerations", n);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after the gravity kernel");
}

void check_gravity(float softening, uint64_t samples) {
    const char *fault = nb_field_fault(softening, samples);
    NB_ASSERT(fault == nullptr, "invalid gravity call (softening %g, %llu points): %s", (double)softening, (unsigned long long)samples, fault);
}

}  // namespace

namespace nbi {

void gravity_release(SimPipeline *s) {
    dev_free(s->gravity_in);
    dev_free(s->gravity_acc);
    s->gravity_in = nullptr;
    s->gravity_acc = nullptr;
    s->gravity_in_cap = s->gravity_acc_cap = 0;
}

}  // namespace nbi

extern "C" {

void nb_hip_acceleration_at(SimPipeline *s, const float *points, uint32_t n, float softening, float *acc) {
    check_diag(s, "nb_hip_acceleration_at");
    check_gravity(softening, n);
    NB_ASSERT((points != nullptr && acc != nullptr) || n == 0, "NULL points or acc");
    if (n == 0) {
        s->diag_timed = false;
        return;
    }
    run_gravity(s, false, points, (size_t)n * 2, n, 0, softening, acc);
}

void nb_hip_acceleration_map(SimPipeline *s, const RenderView *view, float softening, float *acc) {
    check_diag(s, "nb_hip_acceleration_map");
    NB_ASSERT(view != nullptr, "NULL RenderView");
    const char *fault = nb_render_view_fault(view);
    NB_ASSERT(fault == nullptr, "invalid RenderView (%u x %u, zoom %g): %s", view->width, view->height, (double)view->zoom, fault);
    check_gravity(softening, (uint64_t)view->width * view->height);
    NB_ASSERT(acc != nullptr, "NULL acceleration map");
    std::vector<float> coords((size_t)view->width + view->height);
    nb_render_pixel_centres(view, coords.data(), coords.data() + view->width);
    run_gravity(s, true, coords.data(), coords.size(), view->width * view->height, view->width, softening, acc);
}

}  // extern "C"
