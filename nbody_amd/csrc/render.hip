// render.hip -- bounds, per-class count image and RGBA frame of the state a pipeline holds (include/nbody_render.h): the
// checks, the buffers, the stream order and the C-ABI entry points nb_hip_bounds / nb_hip_render_counts / nb_hip_render_rgba.
// The kernels and their launchers are render_kernels.hip (render_kernels.h), beside the ensemble's (batch_observe.hip is
// their host side).
#include "pipeline_internal.h"
#include "nbody_hip_tuning.h"
#include "render_common.h"

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
        rd::launch_splat(s->stream, s->pos[s->cur], s->mass, s->radius, N, *view, s->render_merge != 0, s->render_counts, s->render_discs,
                         s->render_words);
        ASSERT_HIP(hipGetLastError(), "splat_kernel launch (%u particles)", N);
    }
    if (detail) s->ev_splat.record(s->stream);
    if (N > 0) {
        rd::launch_discs(s->stream, s->render_discs, s->render_words, view->width, view->height, s->render_counts);
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
        rd::launch_bounds(s->stream, s->pos[s->cur], N, keys);
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
    rd::launch_shade(s->stream, s->render_counts, plane, *palette, s->render_rgba);
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
