// render.hip -- bounds, per-class count image and RGBA frame of the state a pipeline holds (include/nbody_render.h).
//
// Definitions: include/nbody_render.h; the per-particle and per-pixel arithmetic is render_common.h, the same inline
// functions the host path (render_cpu.c) compiles.  Every result is an integer sum or an integer min / max, so the
// order in which lanes, waves and workgroups arrive cannot change a bit: no float atomics anywhere.
//
// bounds_kernel  x and y of the finite particles as ordered unsigned keys (-0 below +0), min / max per lane over a grid
//                stride, across the wave by shuffles, across the workgroup's waves through LDS, then four no-return
//                global_atomic_umin / umax per workgroup.
// splat_kernel   one lane = PER_LANE particles of pos[cur] / mass / radius (all loads issued before the first add).  A
//                particle is classified and becomes nothing, a point or a disc.  Discs whose candidate box meets the image
//                are appended to a compact list (one returning add per wave and item: ballot + popcount).  Points are
//                added to the count image.  Zoomed out, half a million particles land in a handful of words, so lanes
//                that hit the same word are merged first: the first live lane's word is broadcast (v_readlane), the
//                lanes that match it are counted (ballot + popcount) and leave, and their sum waits in a wave-uniform
//                pending (word, count) pair per class that the next item of the same wave can add to; a pair is written
//                with ONE no-return global_atomic_add_u32 when its word changes or the wave ends.  A round that merges
//                fewer than MERGE_MIN lanes means the words are spread: the lanes still live then add 1 each in one
//                vector atomic and the item is done, so a spread view pays one broadcast and one compare per item.
// disc_kernel    a disc's work is its clipped candidate box.  It is cut into DISC_SLICES interleaved row sets, one wave
//                each, lanes along x: a core zoomed to fill 1280 x 720 runs on 64 waves, a 7-pixel star on 7.  Waves
//                walk (disc, slice) items in a grid stride; the disc count is read from device memory, so the host never
//                waits for the splat.
// shade_kernel   one pixel per lane: the integer formula of the header, one packed RGBA word stored.
//
// The C-ABI entry points nb_hip_bounds / nb_hip_render_counts / nb_hip_render_rgba sit at the bottom of this file.
#include "pipeline_internal.h"
#include "nbody_hip_tuning.h"
#include "render_common.h"

namespace nb {
namespace render {

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int PER_LANE = 8;          // splat: particles per lane
constexpr uint32_t MERGE_MIN = 4;    // splat: a round that merges fewer lanes ends the merging of its item
constexpr uint32_t DISC_SLICES = 64; // waves a disc's rows are dealt to
constexpr uint32_t DISC_GROUPS = 1024;
constexpr uint32_t BOUNDS_GROUPS_MAX = 256;   // one workgroup per compute unit, a grid stride beyond
constexpr uint32_t NO_WORD = 0xffffffffu;   // no count-image word: the image has at most 3 * 2^24 of them

struct ViewParams {
    float tx, ty, ox, oy, zoom, core_mass;
    uint32_t width, height;
};

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d /= 2) v = min(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d /= 2) v = max(v, (uint32_t)__shfl_xor((int)v, d, WAVE));
    return v;
}

// keys[0..3] = min key of x, of y, max key of x, of y; initialised to the identities by the host
__global__ __launch_bounds__(THREADS) void bounds_kernel(const float2 *pos, uint32_t n, uint32_t *keys) {
    uint32_t lo_x = NB_RENDER_KEY_NONE_MIN, lo_y = NB_RENDER_KEY_NONE_MIN;
    uint32_t hi_x = NB_RENDER_KEY_NONE_MAX, hi_y = NB_RENDER_KEY_NONE_MAX;
    for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < n; i += gridDim.x * THREADS) {
        const float2 p = pos[i];
        if (!nb_render_finite(p.x) || !nb_render_finite(p.y)) continue;
        const uint32_t kx = nb_render_order_key(p.x), ky = nb_render_order_key(p.y);
        lo_x = min(lo_x, kx);
        hi_x = max(hi_x, kx);
        lo_y = min(lo_y, ky);
        hi_y = max(hi_y, ky);
    }
    lo_x = wave_min(lo_x);
    lo_y = wave_min(lo_y);
    hi_x = wave_max(hi_x);
    hi_y = wave_max(hi_y);
    // the four waves meet in LDS: four adds on ONE cache line per workgroup (the line takes ~88 atomics per microsecond)
    __shared__ uint32_t part[THREADS / WAVE][4];
    const uint32_t wid = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        part[wid][0] = lo_x;
        part[wid][1] = lo_y;
        part[wid][2] = hi_x;
        part[wid][3] = hi_y;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        uint32_t v = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < THREADS / WAVE; w++) v = threadIdx.x < 2 ? min(v, part[w][threadIdx.x]) : max(v, part[w][threadIdx.x]);
        if (threadIdx.x < 2)
            atomicMin(&keys[threadIdx.x], v);
        else
            atomicMax(&keys[threadIdx.x], v);
    }
}

// a wave-uniform pending (word, count): flushed by one lane with one no-return add
struct Pending {
    uint32_t word = NO_WORD, count = 0;
};

__device__ __forceinline__ void flush(Pending &p, uint32_t *counts, uint32_t lane) {
    if (p.count != 0 && lane == 0) atomicAdd(&counts[p.word], p.count);
    p.word = NO_WORD;
    p.count = 0;
}

__device__ __forceinline__ void pend(Pending &p, uint32_t word, uint32_t count, uint32_t *counts, uint32_t lane) {
    if (p.word != word) {
        flush(p, counts, lane);
        p.word = word;
    }
    p.count += count;
}

template <bool MERGE>
__global__ __launch_bounds__(THREADS) void splat_kernel(const float2 *pos, const float *mass, const float *radius, uint32_t n,
                                                        const ViewParams v, uint32_t *counts, NbSplat *discs, uint32_t *ndisc) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = (blockIdx.x * THREADS + threadIdx.x) / WAVE;
    const uint32_t base = wave * (WAVE * PER_LANE);
    const uint32_t plane = v.width * v.height;
    const uint64_t below = (1ull << lane) - 1ull;

    float2 p[PER_LANE];
    float m[PER_LANE], r[PER_LANE];
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) {
        const uint32_t i = base + k * WAVE + lane;
        const uint32_t c = i < n ? i : n - 1;   // tail lanes reload the last particle; it is not counted twice (live below)
        p[k] = pos[c];
        m[k] = mass[c];
        r[k] = radius[c];
    }

    Pending pending[NB_RENDER_CLASSES];
#pragma unroll
    for (int k = 0; k < PER_LANE; k++) {
        const bool live = base + k * WAVE + lane < n;
        NbSplat s;
        const int kind = nb_render_classify(p[k].x, p[k].y, m[k], r[k], v.tx, v.ty, v.ox, v.oy, v.zoom, v.core_mass, &s);

        // discs that can touch the image: appended to the list, one returning add per wave
        uint32_t x0, x1, y0, y1;
        const bool disc = live && kind == NB_RENDER_DISC && nb_render_disc_span(s.sx, s.rho, v.width, &x0, &x1) &&
                          nb_render_disc_span(s.sy, s.rho, v.height, &y0, &y1);
        const uint64_t dmask = __ballot(disc);
        if (dmask != 0) {
            const int first = __ffsll((unsigned long long)dmask) - 1;
            uint32_t at = 0;
            if ((int)lane == first) at = atomicAdd(ndisc, (uint32_t)__popcll(dmask));
            at = (uint32_t)__builtin_amdgcn_readlane((int)at, first);
            if (disc) discs[at + (uint32_t)__popcll(dmask & below)] = s;
        }

        // points in view
        uint32_t px = 0, py = 0;
        const bool point = live && kind == NB_RENDER_POINT && nb_render_point_pixel(s.sx, s.sy, v.width, v.height, &px, &py);
        const uint32_t word = s.cls * plane + py * v.width + px;
        if constexpr (!MERGE) {
            if (point) atomicAdd(&counts[word], 1u);
        } else {
            uint64_t act = __ballot(point);
            while (act != 0) {
                const int first = __ffsll((unsigned long long)act) - 1;
                const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)word, first);
                const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)s.cls, first);
                const uint64_t same = __ballot(point && word == w0) & act;
                const uint32_t cnt = (uint32_t)__popcll(same);
                if (cnt < MERGE_MIN) {   // spread words: what is left adds 1 per lane, in one vector atomic
                    if ((act >> lane) & 1ull) atomicAdd(&counts[word], 1u);
                    break;
                }
                act &= ~same;
                if (c0 == 0)
                    pend(pending[0], w0, cnt, counts, lane);
                else if (c0 == 1)
                    pend(pending[1], w0, cnt, counts, lane);
                else
                    pend(pending[2], w0, cnt, counts, lane);
            }
        }
    }
    if constexpr (MERGE) {
#pragma unroll
        for (int c = 0; c < NB_RENDER_CLASSES; c++) flush(pending[c], counts, lane);
    }
}

__global__ __launch_bounds__(THREADS) void disc_kernel(const NbSplat *discs, const uint32_t *ndisc, uint32_t width, uint32_t height,
                                                       uint32_t *counts) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * THREADS + threadIdx.x) / WAVE);
    const uint32_t waves = gridDim.x * (THREADS / WAVE);
    const uint64_t items = (uint64_t)*ndisc * DISC_SLICES;
    const uint32_t plane = width * height;
    for (uint64_t it = wave; it < items; it += waves) {
        const NbSplat s = discs[it / DISC_SLICES];
        const uint32_t slice = (uint32_t)(it % DISC_SLICES);
        uint32_t x0, x1, y0, y1;
        if (!nb_render_disc_span(s.sx, s.rho, width, &x0, &x1) || !nb_render_disc_span(s.sy, s.rho, height, &y0, &y1)) continue;
        uint32_t *img = counts + s.cls * plane;
        for (uint32_t py = y0 + slice; py <= y1; py += DISC_SLICES)
            for (uint32_t px = x0 + lane; px <= x1; px += WAVE)
                if (nb_render_disc_covers(s.sx, s.sy, s.rho, px, py)) atomicAdd(&img[py * width + px], 1u);
    }
}

__global__ __launch_bounds__(THREADS) void shade_kernel(const uint32_t *counts, uint32_t plane, const RenderPalette pal, uint32_t *rgba) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= plane) return;
    rgba[i] = nb_render_shade_pixel(counts[i], counts[plane + i], counts[2 * plane + i], &pal);
}

}  // namespace render
}  // namespace nb

namespace {

using namespace nbi;
namespace rd = nb::render;

void check_render(SimPipeline *s, const char *what) {
    NB_ASSERT(s != nullptr, "NULL pipeline");
    NB_ASSERT(!s->sharded, "%s of a sharded pipeline needs a collective over the ranks: not supported", what);
    NB_ASSERT(s->on_device, "%s before SetSimulationData", what);
}

void check_view(const RenderView *view) {
    NB_ASSERT(view != nullptr, "NULL RenderView");
    const char *fault = nb_render_view_fault(view);
    NB_ASSERT(fault == nullptr, "invalid RenderView (%u x %u, zoom %g): %s", view->width, view->height, (double)view->zoom, fault);
}

void ensure_words(SimPipeline *s) {
    if (!s->render_words) s->render_words.alloc(8);
}

// clear + splat + disc on the stream: the count image of the current state is in s->render_counts afterwards
void enqueue_counts(SimPipeline *s, const RenderView *view) {
    use_device();
    const uint32_t N = s->data.total_len;
    const size_t plane = (size_t)view->width * view->height;
    s->render_counts.grown(s->stream, plane * NB_RENDER_CLASSES);
    ensure_words(s);
    if (!s->render_discs) s->render_discs.alloc(N);
    const bool detail = s->render_detail != 0;
    s->render_iv.begin(s->stream);
    ASSERT_HIP(hipMemsetAsync(s->render_counts, 0, plane * NB_RENDER_CLASSES * sizeof(uint32_t), s->stream), "clear the count image");
    if (N > 0) {
        ASSERT_HIP(hipMemsetAsync(s->render_words, 0, sizeof(uint32_t), s->stream), "clear the disc count");
        const rd::ViewParams v = {view->target[0], view->target[1], view->offset[0], view->offset[1],
                                  view->zoom,      view->core_mass, view->width,     view->height};
        const uint32_t per_group = rd::THREADS * rd::PER_LANE;
        const dim3 grid((N + per_group - 1) / per_group), block(rd::THREADS);
        if (s->render_merge)
            hipLaunchKernelGGL(rd::splat_kernel<true>, grid, block, 0, s->stream, s->pos[s->cur], s->mass, s->radius, N, v,
                               s->render_counts, s->render_discs, s->render_words);
        else
            hipLaunchKernelGGL(rd::splat_kernel<false>, grid, block, 0, s->stream, s->pos[s->cur], s->mass, s->radius, N, v,
                               s->render_counts, s->render_discs, s->render_words);
        ASSERT_HIP(hipGetLastError(), "splat_kernel launch (%u particles)", N);
    }
    if (detail) s->ev_splat.record(s->stream);
    if (N > 0) {
        hipLaunchKernelGGL(rd::disc_kernel, dim3(rd::DISC_GROUPS), dim3(rd::THREADS), 0, s->stream, s->render_discs, s->render_words,
                           view->width, view->height, s->render_counts);
        ASSERT_HIP(hipGetLastError(), "disc_kernel launch");
    }
    if (detail) s->ev_disc.record(s->stream);
    s->render_detailed = detail;
}

}  // namespace

extern "C" {

void nb_hip_bounds(SimPipeline *s, float *bounds) {
    check_render(s, "nb_hip_bounds");
    NB_ASSERT(bounds != nullptr, "NULL bounds");
    const uint32_t N = s->data.total_len;
    uint32_t key[4] = {NB_RENDER_KEY_NONE_MIN, NB_RENDER_KEY_NONE_MIN, NB_RENDER_KEY_NONE_MAX, NB_RENDER_KEY_NONE_MAX};
    if (N > 0) {
        use_device();
        ensure_words(s);
        uint32_t *keys = s->render_words + 4;
        s->bounds_iv.begin(s->stream);
        ASSERT_HIP(hipMemsetAsync(keys, 0xff, 2 * sizeof(uint32_t), s->stream), "identity of the min keys");
        ASSERT_HIP(hipMemsetAsync(keys + 2, 0, 2 * sizeof(uint32_t), s->stream), "identity of the max keys");
        const uint32_t groups = (N + rd::THREADS - 1) / rd::THREADS;
        hipLaunchKernelGGL(rd::bounds_kernel, dim3(groups < rd::BOUNDS_GROUPS_MAX ? groups : rd::BOUNDS_GROUPS_MAX), dim3(rd::THREADS), 0,
                           s->stream, s->pos[s->cur], N, keys);
        ASSERT_HIP(hipGetLastError(), "bounds_kernel launch (%u particles)", N);
        s->bounds_iv.end(s->stream);
        ASSERT_HIP(hipMemcpyAsync(key, keys, sizeof(key), hipMemcpyDeviceToHost, s->stream), "D2H of the bounds");
        ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_bounds");
    } else {
        s->bounds_iv.clear();
    }
    nb_render_bounds_from_keys(key, bounds);
}

void nb_hip_render_counts(SimPipeline *s, const RenderView *view, uint32_t *counts) {
    check_render(s, "nb_hip_render_counts");
    check_view(view);
    NB_ASSERT(counts != nullptr, "NULL count image");
    enqueue_counts(s, view);
    s->render_iv.end(s->stream);
    const size_t bytes = (size_t)view->width * view->height * NB_RENDER_CLASSES * sizeof(uint32_t);
    ASSERT_HIP(hipMemcpyAsync(counts, s->render_counts, bytes, hipMemcpyDeviceToHost, s->stream), "D2H of the count image");
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_render_counts");
}

void nb_hip_render_rgba(SimPipeline *s, const RenderView *view, const RenderPalette *palette, uint8_t *rgba) {
    check_render(s, "nb_hip_render_rgba");
    check_view(view);
    NB_ASSERT(palette != nullptr && rgba != nullptr, "NULL argument");
    NB_ASSERT(palette->saturation >= 1u, "RenderPalette saturation must be at least 1");
    const uint32_t plane = view->width * view->height;
    enqueue_counts(s, view);
    s->render_rgba.grown(s->stream, (size_t)plane);
    hipLaunchKernelGGL(rd::shade_kernel, dim3((plane + rd::THREADS - 1) / rd::THREADS), dim3(rd::THREADS), 0, s->stream,
                       s->render_counts, plane, *palette, s->render_rgba);
    ASSERT_HIP(hipGetLastError(), "shade_kernel launch (%u pixels)", plane);
    s->render_iv.end(s->stream);
    ASSERT_HIP(hipMemcpyAsync(rgba, s->render_rgba, (size_t)plane * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream), "D2H of the frame");
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_render_rgba");
}

// tuning hook (nbody_hip_tuning.h)
double nb_hip_last_render_ms(SimPipeline *s, double *parts) {
    NB_ASSERT(s != nullptr, "NULL pipeline");
    if (parts) parts[0] = parts[1] = parts[2] = parts[3] = 0.0;
    if (!s->render_iv.valid() && !s->bounds_iv.valid()) return 0.0;
    use_device();
    if (parts) parts[0] = s->bounds_iv.ms();
    const double whole = s->render_iv.ms();   // waits for the last event: the ones between are done
    if (parts && s->render_iv.valid() && s->render_detailed) {
        parts[1] = elapsed_ms(s->render_iv.first.get(), s->ev_splat.get());
        parts[2] = elapsed_ms(s->ev_splat.get(), s->ev_disc.get());
        parts[3] = elapsed_ms(s->ev_disc.get(), s->render_iv.last.get());
    }
    return whole;
}

}  // extern "C"
