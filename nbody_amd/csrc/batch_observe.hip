// batch_observe.hip -- the read-only calls on a SimBatch: energy and potential of every member (kernels: batch_diag.hip),
// bounds, count images and frames (kernels: render_kernels.hip), the potential, the acceleration field and the tidal tensor at
// probe points and over views (kernels: batch_field.hip, tidal.hip), with their tuning hooks and timers.  Each
// looks at the latest state without reading the particles back: a constant number of launches, one copy, one sync for any B.
// Every one of them runs through pipeline_internal.h's read_call, on the ensemble's one ReadScratch (what each resets is listed
// there); bounds and the renders cut its work buffer into sections and bracket an interval of their own.
#include "batch_internal.h"
#include "batch_diag.h"
#include "batch_field.h"
#include "diag_sums.h"
#include "field_common.h"
#include "nbody_hip_tuning.h"
#include "render_common.h"
#include "render_kernels.h"

using namespace nbi;
namespace rd = nb::render;

namespace {

// ---- diagnostics: the state every member holds, without reading the particles back ----------------------------------

void check_diag(SimBatch *s, const void *out, const char *what) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    NB_ASSERT(out != nullptr, "%s: NULL result array", what);
    NB_ASSERT(s->has_data, "%s before nb_hip_batch_set_data", what);
}

// the three render calls are not wired for ragged ensembles: said before anything touches the device
void check_not_ragged(const SimBatch *s, const char *what) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    NB_ASSERT(!s->ragged, "%s: rendering of ragged ensembles (members of different sizes) is not supported", what);
}

nbd::EnsembleDiagParams diag_params(const SimBatch *s) {   // of the latest state
    nbd::EnsembleDiagParams p{};
    p.pos = s->pos[s->cur];
    p.vel = s->vel;
    p.radius = s->radius;
    p.mass = s->mass;
    p.gm = s->gm;
    p.mass_len = s->mass_len_dev;
    p.n = s->n;
    p.stride = s->stride;
    return p;
}

}  // namespace

namespace nbi {

void launch_energy_sums(SimBatch *s, double *res) {
    const uint32_t tiles = nbd::ensemble_tiles(s->n);
    nbd::EnsembleDiagParams p = diag_params(s);
    p.slab = s->diag;
    nbd::launch_ensemble_potential(s->stream, p, s->count);
    ASSERT_HIP(hipGetLastError(), "ensemble_phi_kernel launch (energy, %u members of %u)", s->count, s->n);
    nbd::launch_ensemble_reduce(s->stream, s->diag, s->mass_len_dev, tiles, s->count, res);
    ASSERT_HIP(hipGetLastError(), "ensemble_reduce_kernel launch (%u members)", s->count);
}

double *energy_slab(SimBatch *s) {
    s->diag.grown(s->stream, (size_t)s->count * (nbd::ensemble_tiles(s->n) + 1) * NB_DIAG_SUMS);
    return s->diag;
}

}  // namespace nbi

namespace {

// ---- rendering: bounds, count tiles and frames of every member, without reading the particles back ------------------

void check_views(const SimBatch *s, const RenderView *views, const char *what) {
    NB_ASSERT(views != nullptr, "%s: NULL RenderView array", what);
    uint32_t member = 0;
    const char *fault = nb_render_views_fault(views, s->count, &member);
    NB_ASSERT(fault == nullptr, "%s: invalid RenderView of member %u of %u (%u x %u, zoom %g): %s", what, member, s->count,
              views[member].width, views[member].height, (double)views[member].zoom, fault);
}

// One read_call inside render_iv: the views are its args; the tile kernel (straight to the frame when a palette is given) or
// clear + splat + disc pass (+ shade); then the count images [count][3][h][w] or the frames [count][h][w] to `out`.  The
// sections of read.work: the tile path's one result; the global path's count words (the cursor behind the images), its disc
// list [count * n] and, for frames, the frames.
void render(SimBatch *s, const char *what, const RenderView *views, const RenderPalette *palette, void *out) {
    const uint32_t width = views[0].width, height = views[0].height;
    const size_t plane = (size_t)width * height;
    const bool tile = rd::tile_fits(width, height) && s->render_mode == 0;
    const size_t count_bytes = (size_t)s->count * NB_RENDER_CLASSES * plane * sizeof(uint32_t), frame_bytes = (size_t)s->count * plane * sizeof(uint32_t);
    const size_t clear_bytes = rd::global_count_words(s->count, width, height) * sizeof(uint32_t);
    size_t work_bytes = 0, counts_at = 0, discs_at = 0, rgba_at = 0;
    if (tile) {   // one section, at 0 under either name: the counts or the frames, whichever the call returns
        section(work_bytes, palette ? frame_bytes : count_bytes);
    } else {
        counts_at = section(work_bytes, clear_bytes);
        discs_at = section(work_bytes, (size_t)s->count * s->n * sizeof(rd::Disc));
        if (palette) rgba_at = section(work_bytes, frame_bytes);
    }
    read_call(s, s->render_iv, what, views, (size_t)s->count * sizeof(RenderView), work_bytes, out, palette ? frame_bytes : count_bytes,
              [&](void *views_dev, void *work) -> const void * {
        char *base = static_cast<char *>(work);
        uint32_t *counts = reinterpret_cast<uint32_t *>(base + counts_at), *rgba = reinterpret_cast<uint32_t *>(base + rgba_at);
        rd::EnsembleRenderParams p{};
        p.pos = s->pos[s->cur];
        p.mass = s->mass;
        p.radius = s->radius;
        p.n = s->n;
        p.stride = s->stride;
        p.count = s->count;
        p.width = width;
        p.height = height;
        p.views = static_cast<const RenderView *>(views_dev);
        if (tile) {
            rd::launch_ensemble_tile(s->stream, p, counts, palette, rgba);   // it stores to the one of the two the call returns
            s->render_launches = 1;
        } else {
            ASSERT_HIP(hipMemsetAsync(counts, 0, clear_bytes, s->stream), "clear %u count images and the disc cursor", s->count);
            rd::launch_ensemble_global(s->stream, p, counts, reinterpret_cast<rd::Disc *>(base + discs_at));
            if (palette) rd::launch_ensemble_shade(s->stream, counts, s->count, (uint32_t)plane, *palette, rgba);
            s->render_launches = palette ? 4 : 3;
        }
        ASSERT_HIP(hipGetLastError(), "ensemble render launch (%u members of %u particles, %u x %u, %s path)", s->count, s->n, width, height,
                   tile ? "tile" : "global");
        return palette ? rgba : counts;
    });
    s->render_tile = tile;
}

// ---- fields: Phi, g and T of every member at n samples each, without reading the particles back ------------------------

// what a field call checks before it looks at its samples; `samples` = all members' together
void check_field(SimBatch *s, const char *what, float softening, uint64_t samples) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    NB_ASSERT(s->has_data, "%s before nb_hip_batch_set_data", what);
    const char *fault = nb_field_fault(softening, samples);
    NB_ASSERT(fault == nullptr, "%s: invalid call (softening %g, %u members, %llu points in all): %s", what, (double)softening, s->count,
              (unsigned long long)samples, fault);
}

// one read_call: upload `in_stride` floats per member ([count] probe sets of (x, y) pairs, or [count] maps' width column + height
// row coordinates), evaluate n samples of every member in one launch, copy the [count][n][comps] floats to `out`
// `comps` floats per sample name the quantity: 1 = Phi, 2 = g, 3 = T
void sample_members(SimBatch *s, const char *what, uint32_t comps, bool map, const float *in, uint32_t in_stride, uint32_t n,
                    uint32_t width, float softening, float *out) {
    const size_t in_bytes = (size_t)s->count * in_stride * sizeof(float), out_bytes = (size_t)s->count * n * comps * sizeof(float);
    read_call(s, s->read.iv, what, in, in_bytes, out_bytes, out, out_bytes, [&](void *in_dev, void *work) -> const void * {
        nb::field::EnsembleParams p{};
        p.pos = s->pos[s->cur];
        p.gm = s->gm;
        p.mass_len = s->mass_len_dev;
        p.stride = s->stride;
        p.in = static_cast<const float *>(in_dev);
        p.in_stride = in_stride;
        p.n = n;
        p.width = width;
        p.soft = softening;
        p.out = work;
        if (comps == 3)
            nb::field::launch_ensemble_tidal(s->stream, p, s->count, map);
        else
            nb::field::launch_ensemble_sample(s->stream, p, s->count, comps == 2, map);
        ASSERT_HIP(hipGetLastError(), "%s: ensemble_sample_kernel launch (%u members, %u samples each)", what, s->count, n);
        return work;
    });
}

void sample_members_at(SimBatch *s, const char *what, uint32_t comps, const float *points, uint32_t n, float softening, float *out) {
    check_field(s, what, softening, s ? (uint64_t)s->count * n : 0);
    NB_ASSERT((points != nullptr && out != nullptr) || n == 0, "%s: NULL points or result", what);
    if (n == 0) {
        s->read.iv.clear();
        return;
    }
    sample_members(s, what, comps, false, points, 2 * n, n, 0, softening, out);
}

// a map is the probes product at the member's own pixel centres: per member width column coordinates, then height row coordinates
void sample_members_map(SimBatch *s, const char *what, uint32_t comps, const RenderView *views, float softening, float *out) {
    check_field(s, what, softening, 0);
    check_views(s, views, what);
    const uint32_t width = views[0].width, height = views[0].height;
    check_field(s, what, softening, (uint64_t)s->count * width * height);
    NB_ASSERT(out != nullptr, "%s: NULL result array", what);
    std::vector<float> coords((size_t)s->count * (width + height));
    for (uint32_t b = 0; b < s->count; b++) {
        float *xs = coords.data() + (size_t)b * (width + height);
        nb_render_pixel_centres(&views[b], xs, xs + width);
    }
    sample_members(s, what, comps, true, coords.data(), width + height, width * height, width, softening, out);
}

}  // namespace

extern "C" {

void nb_hip_ensemble_energy(SimBatch *s, WorldEnergy *out) {
    check_diag(s, out, "nb_hip_ensemble_energy");
    constexpr size_t Q = NB_DIAG_SUMS;
    // the workspace is the ensemble's own slab, which traced updates use too: only the results come back through the protocol
    const void *host = read_call(s, s->read.iv, "nb_hip_ensemble_energy", nullptr, 0, 0, nullptr, (size_t)s->count * Q * sizeof(double),
                                 [&](void *, void *) -> const void * {
        double *res = energy_slab(s) + (size_t)s->count * nbd::ensemble_tiles(s->n) * Q;
        launch_energy_sums(s, res);
        return res;
    });
    for (uint32_t b = 0; b < s->count; b++) nb_energy_from_sums(static_cast<const double *>(host) + (size_t)b * Q, out + b);
}

void nb_hip_ensemble_potential(SimBatch *s, float *phi) {
    check_diag(s, phi, "nb_hip_ensemble_potential");
    const size_t bytes = (size_t)s->offsets[s->count] * sizeof(float);
    read_call(s, s->read.iv, "nb_hip_ensemble_potential", nullptr, 0, bytes, phi, bytes, [&](void *, void *work) -> const void * {
        nbd::EnsembleDiagParams p = diag_params(s);
        p.phi = static_cast<float *>(work);
        // packed member after member; the member sizes and offsets on the device are null in a uniform ensemble
        nbd::launch_ensemble_potential(s->stream, p, s->count, s->n_len_dev, s->offsets_dev);
        ASSERT_HIP(hipGetLastError(), "ensemble_phi_kernel launch (%u members of %u)", s->count, s->n);
        return work;
    });
}

void nb_hip_ensemble_potential_at(SimBatch *s, const float *points, uint32_t n, float softening, float *phi) {
    sample_members_at(s, "nb_hip_ensemble_potential_at", 1, points, n, softening, phi);
}

void nb_hip_ensemble_potential_map(SimBatch *s, const RenderView *views, float softening, float *phi) {
    sample_members_map(s, "nb_hip_ensemble_potential_map", 1, views, softening, phi);
}

void nb_hip_ensemble_acceleration_at(SimBatch *s, const float *points, uint32_t n, float softening, float *acc) {
    sample_members_at(s, "nb_hip_ensemble_acceleration_at", 2, points, n, softening, acc);
}

void nb_hip_ensemble_acceleration_map(SimBatch *s, const RenderView *views, float softening, float *acc) {
    sample_members_map(s, "nb_hip_ensemble_acceleration_map", 2, views, softening, acc);
}

void nb_hip_ensemble_tidal_at(SimBatch *s, const float *points, uint32_t n, float softening, float *t) {
    sample_members_at(s, "nb_hip_ensemble_tidal_at", 3, points, n, softening, t);
}

void nb_hip_ensemble_tidal_map(SimBatch *s, const RenderView *views, float softening, float *t) {
    sample_members_map(s, "nb_hip_ensemble_tidal_map", 3, views, softening, t);
}

// tuning hook (nbody_hip_tuning.h): device time of the kernels of the last read-only call (pipeline_internal.h read_call)
double nb_hip_ensemble_last_diag_ms(SimBatch *s) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (!s->read.iv.valid()) return 0.0;
    use_device();
    return s->read.iv.ms();
}

void nb_hip_ensemble_bounds(SimBatch *s, float *bounds) {
    check_not_ragged(s, "nb_hip_ensemble_bounds");
    check_diag(s, bounds, "nb_hip_ensemble_bounds");
    // the interval is shared with the renders; render_tile / render_launches speak of renders only
    const size_t bytes = (size_t)s->count * 4 * sizeof(uint32_t);
    const void *host = read_call(s, s->render_iv, "nb_hip_ensemble_bounds", nullptr, 0, bytes, nullptr, bytes, [&](void *, void *work) -> const void * {
        rd::launch_ensemble_bounds(s->stream, s->pos[s->cur], s->n, s->stride, s->count, static_cast<uint32_t *>(work));
        ASSERT_HIP(hipGetLastError(), "ensemble_bounds_kernel launch (%u members of %u)", s->count, s->n);
        return work;
    });
    for (uint32_t b = 0; b < s->count; b++) nb_render_bounds_from_keys(static_cast<const uint32_t *>(host) + (size_t)b * 4, bounds + (size_t)b * 4);
}

void nb_hip_ensemble_render_counts(SimBatch *s, const RenderView *views, uint32_t *counts) {
    check_not_ragged(s, "nb_hip_ensemble_render_counts");
    check_diag(s, counts, "nb_hip_ensemble_render_counts");
    check_views(s, views, "nb_hip_ensemble_render_counts");
    render(s, "nb_hip_ensemble_render_counts", views, nullptr, counts);
}

void nb_hip_ensemble_render_rgba(SimBatch *s, const RenderView *views, const RenderPalette *palette, uint8_t *rgba) {
    check_not_ragged(s, "nb_hip_ensemble_render_rgba");
    check_diag(s, rgba, "nb_hip_ensemble_render_rgba");
    check_views(s, views, "nb_hip_ensemble_render_rgba");
    NB_ASSERT(palette != nullptr, "nb_hip_ensemble_render_rgba: NULL RenderPalette");
    NB_ASSERT(palette->saturation >= 1u, "RenderPalette saturation must be at least 1");
    render(s, "nb_hip_ensemble_render_rgba", views, palette, rgba);
}

// tuning hooks (nbody_hip_tuning.h)
void nb_hip_ensemble_render_mode(SimBatch *s, int mode) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    NB_ASSERT(mode == 0 || mode == 1, "render mode %d (0 = auto, 1 = global path)", mode);
    s->render_mode = mode;
}

void nb_hip_ensemble_last_render_info(const SimBatch *s, int *tile_path, uint32_t *launches) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (tile_path) *tile_path = s->render_tile;
    if (launches) *launches = s->render_launches;
}

double nb_hip_ensemble_last_render_ms(SimBatch *s) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (!s->render_iv.valid()) return 0.0;
    use_device();
    return s->render_iv.ms();
}

}  // extern "C"
