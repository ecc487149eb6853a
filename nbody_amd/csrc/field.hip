// field.hip -- the potential of the state a pipeline holds at points that are not particles: probes the caller chooses and
// the pixel centres of a view (include/nbody_field.h; nb_hip_potential_at / nb_hip_potential_map).
//
// Definitions (also in include/nbody_field.h and DESIGN.md section 3): for a sample p and a softening s
//     Phi(p; s) = - sum_{j < M} G*m_j / sqrt(|x_j - p|^2 + s),      G*m_j = src_gm[j], M = mass_len
// = diagnostics.hip's Phi_i of a massless receiver at p with radius s.  A sample is never a source, so no term is excluded
// and only the unmasked pair statement runs.
//
// The arithmetic is diag_common.h's and nothing else: the pair statement, the fp32 sum over a block of 256 sources with j
// ascending, float64 totals per block, and the eight source slices [w * per, (w + 1) * per) added in wave order from 0.0.
// A result is defined by that order, not by which wave adds what, so the two kernels below give the same bits, and both
// give the bits potential_kernel gives a massless particle of radius s at the same place:
//   field_split_kernel   potential_kernel's shape: the 8 waves of a workgroup share one tile of 128 samples (64 lanes x 2)
//                        and each walks 1/8 of the source blocks; the slices meet in part[W][TILE] (LDS).  For large M.
//   field_wave_kernel    ensemble_phi_kernel's shape: every wave owns a tile and walks the whole source list itself
//                        (tile_potential over ScalarSources, with rb = M so that the masked segment of every block is
//                        empty).  No LDS, no barrier.  For small worlds under large images, where the split's workgroups
//                        are mostly waves without a block (7 of 8 at M <= 256) and the tiles alone fill the chip.
// pick_wave_shape() below chooses between them, in one place.  Sources stay on the scalar-cache route in both (wave-uniform,
// s_load_dwordx16 / x8).  MAP = true: a lane forms its two samples from the view's column and row coordinates (sample
// i = py * width + px reads xs[px] and ys[py]; the host computed both arrays, render_common.h); MAP = false: it loads them.
// A sample with a non-finite coordinate stores NaN.  No atomics; vector stores only.
#include "pipeline_internal.h"
#include "diag_common.h"
#include "field_common.h"
#include "nbody_hip_tuning.h"

#include <math.h>

namespace nb {
namespace field {

using namespace nbd;

constexpr int WAVES_MAX = 4;   // field_wave_kernel: tiles (waves) per workgroup

struct FieldParams {
    const float2 *pos;     // pos[cur]: the latest state
    const float *src_gm;   // G * m_j, j < n_src
    uint32_t n_src;        // sources [0, M)
    const float *in;       // probes: (x, y) pairs; map: width column coordinates, then height row coordinates
    uint32_t n;            // samples
    uint32_t width;        // map only
    float soft;
    float *phi;            // Phi of sample i, i < n
};

// the K samples of this lane: tile rows lane and lane + 64; tail lanes redo the last sample, their results are dropped
template <bool MAP>
__device__ __forceinline__ void load_samples(const FieldParams &p, uint32_t rb, uint32_t lane, float (&px)[K], float (&py)[K]) {
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

__device__ __forceinline__ void store_sample(const FieldParams &p, uint32_t i, float x, float y, double sum) {
    if (i >= p.n) return;
    const bool finite = nb_render_finite(x) && nb_render_finite(y);
    p.phi[i] = finite ? (float)-sum : __builtin_nanf("");
}

// 512 threads, at most 64 VGPRs (8 waves per SIMD: four workgroups per CU), as potential_kernel.
template <bool MAP>
__global__ __launch_bounds__(WAVE * W, 8) void field_split_kernel(const FieldParams p) {
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t rb = blockIdx.x * TILE;  // first sample of the tile

    float px[K], py[K], r[K], a[K];
    uint32_t ri[K];
    double s[K];
    load_samples<MAP>(p, rb, lane, px, py);
#pragma unroll
    for (int k = 0; k < K; k++) {
        r[k] = p.soft;
        ri[k] = 0;       // read by the masked body only
        a[k] = 0.0f;
        s[k] = 0.0;
    }

    // this wave's slice of the sources, in whole blocks
    const uint32_t nblocks = (p.n_src + BLOCK - 1) / BLOCK;
    const uint32_t per_wave = (nblocks + W - 1) / W;
    const uint32_t b_lo = min(wid * per_wave, nblocks);
    const uint32_t b_hi = min(b_lo + per_wave, nblocks);
    const ConstF sp = (ConstF)(uintptr_t)p.pos, sg = (ConstF)(uintptr_t)p.src_gm;
    for (uint32_t b = b_lo; b < b_hi; b++) {
        const uint32_t j0 = b * BLOCK, j1 = min(j0 + BLOCK, p.n_src);
        block_sum<false>(a, px, py, r, ri, sp, sg, j0, j1);
#pragma unroll
        for (int k = 0; k < K; k++) {
            s[k] += (double)a[k];
            a[k] = 0.0f;
        }
    }

    // the W slices in wave order (float64), then Phi = -sum; thread t of the first two waves holds sample rb + t's
    // coordinates in slot t / 64 of lane t % 64, which is its own slot k = wid
    __shared__ double part[W][TILE];
#pragma unroll
    for (int k = 0; k < K; k++) part[wid][k * WAVE + lane] = s[k];
    __syncthreads();
    if (tid < TILE) {
        double sum = 0.0;
#pragma unroll
        for (int w = 0; w < W; w++) sum += part[w][tid];
        store_sample(p, rb + tid, wid ? px[1] : px[0], wid ? py[1] : py[0], sum);
    }
}
static_assert(K == 2, "field_split_kernel's finishing threads pick their sample by wave index 0 / 1");

// 1..4 waves, one tile each, at most 64 VGPRs.
template <bool MAP>
__global__ __launch_bounds__(WAVE * WAVES_MAX, 8) void field_wave_kernel(const FieldParams p) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t rb = (blockIdx.x * WAVES_MAX + wid) * TILE;   // first sample of this wave's tile
    if (rb >= p.n) return;

    float px[K], py[K], r[K];
    uint32_t ri[K];
    load_samples<MAP>(p, rb, lane, px, py);
#pragma unroll
    for (int k = 0; k < K; k++) {
        r[k] = p.soft;
        ri[k] = 0;
    }
    // the eight source slices of the split kernel's waves, one after another; a tile that starts at M holds no source, so
    // every block runs unmasked as a whole
    double sum[K];
    tile_potential(sum, px, py, r, ri, p.n_src, p.n_src, ScalarSources{(ConstF)(uintptr_t)p.pos, (ConstF)(uintptr_t)p.src_gm});
#pragma unroll
    for (int k = 0; k < K; k++) store_sample(p, rb + k * WAVE + lane, px[k], py[k], sum[k]);
}

}  // namespace field
}  // namespace nb

namespace {

using namespace nbi;
namespace fd = nb::field;

// The one place that picks the kernel shape.  One wave per tile pays when both hold: the world has at most 2 blocks of 256
// sources (most of a split workgroup's 8 waves would walk nothing) and there are enough tiles to fill the chip with one
// wave each.  Measured (tools/field_probe.py, profiles/r12_field_probe.json; wave / split device time): at 1280 x 720
// (7 200 tiles) 0.51 - 0.55 at 1 block, 0.80 at 2, 1.12 - 1.19 from 4 blocks up; at 256 x 256 (512 tiles, a sixteenth of
// the chip's 8 192 wave slots) the split is ahead at every M, by 1.05 - 1.06 at 1 block and 1.8 - 3.8 beyond.  3 blocks
// and tile counts between 512 and 7 200 are not measured: the rule keeps the split there, and puts the tile bound at half
// the wave slots.
constexpr uint32_t WAVE_SHAPE_BLOCKS_MAX = 2;
constexpr uint32_t WAVE_SHAPE_TILES_MIN = 4096;

bool pick_wave_shape(const SimPipeline *s, uint32_t tiles) {
    if (s->field_shape) return s->field_shape == 2;
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
void launch(SimPipeline *s, const fd::FieldParams &p) {
    const uint32_t tiles = (p.n + nbd::TILE - 1) / nbd::TILE;
    if (pick_wave_shape(s, tiles))
        hipLaunchKernelGGL(fd::field_wave_kernel<MAP>, dim3((tiles + fd::WAVES_MAX - 1) / fd::WAVES_MAX), dim3(nbd::WAVE * fd::WAVES_MAX), 0,
                           s->stream, p);
    else
        hipLaunchKernelGGL(fd::field_split_kernel<MAP>, dim3(tiles), dim3(nbd::WAVE * nbd::W), 0, s->stream, p);
    ASSERT_HIP(hipGetLastError(), "field kernel launch (%u samples, %u sources)", p.n, p.n_src);
}

// upload `in_floats` floats, evaluate n samples, one copy of the result, one sync; `in` stays alive until the sync
void run_field(SimPipeline *s, bool map, const float *in, size_t in_floats, uint32_t n, uint32_t width, float softening, float *phi) {
    use_device();
    grow(s, s->field_in, s->field_in_cap, in_floats, "field samples");
    grow(s, s->field_phi, s->field_phi_cap, (size_t)n, "field result");
    ASSERT_HIP(hipMemcpyAsync(s->field_in, in, in_floats * sizeof(float), hipMemcpyHostToDevice, s->stream), "H2D of the field samples");
    fd::FieldParams p{};
    p.pos = s->pos[s->cur];
    p.src_gm = s->src_gm;
    p.n_src = s->data.mass_len;
    p.in = s->field_in;
    p.n = n;
    p.width = width;
    p.soft = softening;
    p.phi = s->field_phi;
    begin_diag(s);
    if (map)
        launch<true>(s, p);
    else
        launch<false>(s, p);
    end_diag(s);
    ASSERT_HIP(hipMemcpyAsync(phi, s->field_phi, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s->stream), "D2H of %u potentials", n);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after the field kernel");
}

void check_field(float softening, uint64_t samples) {
    const char *fault = nb_field_fault(softening, samples);
    NB_ASSERT(fault == nullptr, "invalid field call (softening %g, %llu points): %s", (double)softening, (unsigned long long)samples, fault);
}

}  // namespace

namespace nbi {

void field_release(SimPipeline *s) {
    dev_free(s->field_in);
    dev_free(s->field_phi);
    s->field_in = s->field_phi = nullptr;
    s->field_in_cap = s->field_phi_cap = 0;
}

}  // namespace nbi

extern "C" {

void nb_hip_potential_at(SimPipeline *s, const float *points, uint32_t n, float softening, float *phi) {
    check_diag(s, "nb_hip_potential_at");
    check_field(softening, n);
    NB_ASSERT((points != nullptr && phi != nullptr) || n == 0, "NULL points or phi");
    if (n == 0) {
        s->diag_timed = false;
        return;
    }
    run_field(s, false, points, (size_t)n * 2, n, 0, softening, phi);
}

void nb_hip_potential_map(SimPipeline *s, const RenderView *view, float softening, float *phi) {
    check_diag(s, "nb_hip_potential_map");
    NB_ASSERT(view != nullptr, "NULL RenderView");
    const char *fault = nb_render_view_fault(view);
    NB_ASSERT(fault == nullptr, "invalid RenderView (%u x %u, zoom %g): %s", view->width, view->height, (double)view->zoom, fault);
    check_field(softening, (uint64_t)view->width * view->height);
    NB_ASSERT(phi != nullptr, "NULL potential map");
    std::vector<float> coords((size_t)view->width + view->height);
    nb_render_pixel_centres(view, coords.data(), coords.data() + view->width);
    run_field(s, true, coords.data(), coords.size(), view->width * view->height, view->width, softening, phi);
}

}  // extern "C"
