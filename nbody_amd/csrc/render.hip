// render.hip -- bounds, per-class count image and RGBA frame of the state a pipeline holds (include/nbody_render.h): the
// checks, the sections of the scratch, the stream order and the C-ABI entry points nb_hip_bounds / nb_hip_render_counts /
// nb_hip_render_rgba.  Read-only calls like every other: pipeline_internal.h's read_call on the pipeline's one ReadScratch
// (what each resets is listed there), inside intervals of their own.  The kernels and their launchers are render_kernels.hip
// (render_kernels.h), beside the ensemble's (batch_observe.hip is their host side).
#include "pipeline_internal.h"
#include "nbody_hip_tuning.h"
#include "render_common.h"
#include "render_kernels.h"

using namespace nbi;
namespace rd = nb::render;

void nbi::check_view(const RenderView *view) {
    NB_ASSERT(view != nullptr, "NULL RenderView");
    const char *fault = nb_render_view_fault(view);
    NB_ASSERT(fault == nullptr, "invalid RenderView (%u x %u, zoom %g): %s", view->width, view->height, (double)view->zoom, fault);
}

namespace {

// One read_call inside render_iv: clear + splat + disc pass (+ shade when a palette is given), then the count image [3][h][w]
// or the frame [h][w] to `out`.  The sections of read.work: the count image, the disc cursor, the disc list [N], the frame.
void render(SimPipeline *s, const char *what, const RenderView *view, const RenderPalette *palette, void *out) {
    const uint32_t N = s->data.total_len;
    const size_t plane = (size_t)view->width * view->height;
    const size_t count_bytes = plane * NB_RENDER_CLASSES * sizeof(uint32_t), frame_bytes = plane * sizeof(uint32_t);
    size_t work_bytes = 0;
    const size_t counts_at = section(work_bytes, count_bytes), cursor_at = section(work_bytes, sizeof(uint32_t));
    const size_t discs_at = section(work_bytes, (size_t)N * sizeof(rd::Disc)), rgba_at = palette ? section(work_bytes, frame_bytes) : 0;
    const bool detail = s->render_detail != 0;
    read_call(s, s->render_iv, what, nullptr, 0, work_bytes, out, palette ? frame_bytes : count_bytes, [&](void *, void *work) -> const void * {
        char *base = static_cast<char *>(work);
        uint32_t *counts = reinterpret_cast<uint32_t *>(base + counts_at), *cursor = reinterpret_cast<uint32_t *>(base + cursor_at);
        rd::Disc *discs = reinterpret_cast<rd::Disc *>(base + discs_at);
        ASSERT_HIP(hipMemsetAsync(counts, 0, count_bytes, s->stream), "clear the count image");
        if (N > 0) {
            ASSERT_HIP(hipMemsetAsync(cursor, 0, sizeof(uint32_t), s->stream), "clear the disc count");
            rd::launch_splat(s->stream, s->pos[s->cur], s->mass, s->radius, N, *view, s->render_merge != 0, counts, discs, cursor);
            ASSERT_HIP(hipGetLastError(), "splat_kernel launch (%u particles)", N);
        }
        if (detail) s->ev_splat.record(s->stream);
        if (N > 0) {
            rd::launch_discs(s->stream, discs, cursor, view->width, view->height, counts);
            ASSERT_HIP(hipGetLastError(), "disc_kernel launch");
        }
        if (detail) s->ev_disc.record(s->stream);
        if (!palette) return counts;
        uint32_t *rgba = reinterpret_cast<uint32_t *>(base + rgba_at);
        rd::launch_shade(s->stream, counts, (uint32_t)plane, *palette, rgba);
        ASSERT_HIP(hipGetLastError(), "shade_kernel launch (%zu pixels)", plane);
        return rgba;
    });
    s->render_detailed = detail;
}

}  // namespace

extern "C" {

void nb_hip_bounds(SimPipeline *s, float *bounds) {
    check_diag(s, "nb_hip_bounds");
    NB_ASSERT(bounds != nullptr, "NULL bounds");
    const uint32_t N = s->data.total_len;
    uint32_t key[4] = {NB_RENDER_KEY_NONE_MIN, NB_RENDER_KEY_NONE_MIN, NB_RENDER_KEY_NONE_MAX, NB_RENDER_KEY_NONE_MAX};
    if (N > 0) {
        read_call(s, s->bounds_iv, "nb_hip_bounds", nullptr, 0, sizeof(key), key, sizeof(key), [&](void *, void *work) -> const void * {
            uint32_t *keys = static_cast<uint32_t *>(work);
            ASSERT_HIP(hipMemsetAsync(keys, 0xff, 2 * sizeof(uint32_t), s->stream), "identity of the min keys");
            ASSERT_HIP(hipMemsetAsync(keys + 2, 0, 2 * sizeof(uint32_t), s->stream), "identity of the max keys");
            rd::launch_bounds(s->stream, s->pos[s->cur], N, keys);
            ASSERT_HIP(hipGetLastError(), "bounds_kernel launch (%u particles)", N);
            return keys;
        });
    } else {
        s->bounds_iv.clear();
    }
    nb_render_bounds_from_keys(key, bounds);
}

void nb_hip_render_counts(SimPipeline *s, const RenderView *view, uint32_t *counts) {
    check_diag(s, "nb_hip_render_counts");
    check_view(view);
    NB_ASSERT(counts != nullptr, "NULL count image");
    render(s, "nb_hip_render_counts", view, nullptr, counts);
}

void nb_hip_render_rgba(SimPipeline *s, const RenderView *view, const RenderPalette *palette, uint8_t *rgba) {
    check_diag(s, "nb_hip_render_rgba");
    check_view(view);
    NB_ASSERT(palette != nullptr && rgba != nullptr, "NULL argument");
    NB_ASSERT(palette->saturation >= 1u, "RenderPalette saturation must be at least 1");
    render(s, "nb_hip_render_rgba", view, palette, rgba);
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
