/*
 * world_batch.c -- the include/nbody_batch.h surface: an ensemble of Worlds over one SimBatch (include/nbody_hip.h).
 *
 * The World protocol (world.c) for `count` members at once: the caller's particles are copied and every member is
 * partitioned "mass > 0 first" with CreateWorld's own routine (world_partition.h); the array is uploaded before the
 * first GPU step and pulled back only when a read follows a step.  Nothing on the host changes the array after
 * creation (no CPU stepper for ensembles), so one upload is all there ever is.
 *
 * include/nbody_batch_diag.h: GetWorldBatchEnergy / GetWorldBatchPotential compute on the device when it holds the
 * newest state, without pulling the array, and on the host (diag_cpu.c, member by member) otherwise; neither moves
 * device_is_newer.  include/nbody_batch_trace.h: UpdateWorldBatch_GPU_Traced is an update that also records: same upload, same coherence.
 * include/nbody_batch_render.h: bounds, count images and frames of every member follow the same protocol (device:
 * nb_hip_ensemble_*; host: render_cpu.c member by member).
 * include/nbody_batch_ragged.h: CreateWorldBatchRagged makes a batch whose members differ in size over nb_hip_ragged_create;
 * the array is then packed (member b at offset[b]), which is all the protocol above needs to know -- a uniform batch is
 * the case offset[b] = b * size.  The render calls are not wired for such a batch and abort.
 * include/nbody_adaptive.h: UpdateWorldBatch_GPU_Adaptive / AdvanceWorldBatch_GPU are updates whose step sizes the device
 * chooses per member and step: same upload, same coherence; ragged batches abort.
 * include/nbody_leapfrog.h: UpdateWorldBatch_GPU_Leapfrog(_dts) are updates of kick-drift-kick steps: same upload, same
 * coherence; ragged batches abort.
 * include/nbody_batch_field.h: the potential and the acceleration field of every member at probe points and over views follow
 * the diagnostics' protocol (device: nb_hip_ensemble_potential_at and its three siblings, one launch; host: field_cpu.c member
 * by member), for uniform and ragged batches alike.  include/nbody_batch_tidal.h: the tidal tensor likewise
 * (nb_hip_ensemble_tidal_at / _tidal_map), through the same two functions.
 * include/nbody_batch_profile.h: the radial profiles of every member follow the diagnostics' protocol too (device:
 * nb_hip_ensemble_profile, one launch; host: profile_cpu.c member by member), uniform and ragged batches alike.
 * include/nbody_batch_paircount.h: the pair-separation counts of every member likewise (device: nb_hip_ensemble_pair_counts,
 * one launch; host: paircount_cpu.c member by member).
 * include/nbody_batch_group.h: the friends-of-friends groups of every member likewise (device: nb_hip_ensemble_groups; host:
 * group_cpu.c member by member).
 */
#include "nbody_adaptive.h"
#include "nbody_leapfrog.h"
#include "nbody_batch.h"
#include "nbody_batch_diag.h"
#include "nbody_batch_field.h"
#include "nbody_batch_tidal.h"
#include "nbody_batch_profile.h"
#include "nbody_batch_paircount.h"
#include "nbody_batch_neighbour.h"
#include "nbody_batch_group.h"
#include "nbody_batch_ragged.h"
#include "nbody_batch_render.h"
#include "nbody_batch_trace.h"
#include "nbody_hip.h"

#include <stdbool.h>

#include "diag_sums.h"
#include "field_common.h"
#include "nb_util.h"
#include "profile_common.h"
#include "paircount_common.h"
#include "neighbour_common.h"
#include "group_common.h"
#include "render_common.h"
#include "timestep_common.h"
#include "world_partition.h"

struct WorldBatch {
    Particle *particles;  /* packed, member b at offset[b], each member partitioned */
    uint32_t size;        /* particles per member; ragged: of the largest */
    uint32_t count;       /* members */
    uint32_t *sizes;      /* [count] particles of each member */
    size_t *offset;       /* [count + 1] */
    bool ragged;          /* made by CreateWorldBatchRagged */
    uint32_t *massive;    /* [count] particles with mass > 0 of each member; they come first */
    SimBatch *gpu;
    bool uploaded;        /* the device has seen the array */
    bool device_is_newer; /* the device stepped since the array was last refreshed */
};

/* The host side of both constructors: the packed copy, every member partitioned; sizes[b] was checked by the caller. */
static WorldBatch *make_batch(const Particle *ps, const uint32_t *world_size, uint32_t uniform_size, uint32_t count) {
    WorldBatch *w = NB_NEW(1, WorldBatch);
    NB_CHECK(w != NULL, "Failed to alloc WorldBatch");
    w->sizes = NB_NEW(count, uint32_t);
    w->offset = NB_NEW((size_t)count + 1, size_t);
    w->massive = NB_NEW(count, uint32_t);
    NB_CHECK(w->sizes != NULL && w->offset != NULL && w->massive != NULL, "Failed to alloc the tables of %u members", count);
    w->offset[0] = 0;
    w->size = 0;
    for (uint32_t b = 0; b < count; b++) {
        w->sizes[b] = world_size ? world_size[b] : uniform_size;
        w->offset[b + 1] = w->offset[b] + w->sizes[b];
        if (w->sizes[b] > w->size) w->size = w->sizes[b];
    }
    const size_t total = w->offset[count];
    w->particles = NB_NEW(total, Particle);
    NB_CHECK(w->particles != NULL, "Failed to alloc %zu particles of %u members", total, count);
    memcpy(w->particles, ps, total * sizeof(Particle));
    for (uint32_t b = 0; b < count; b++) w->massive[b] = partition_by_mass(w->particles + w->offset[b], w->sizes[b]);
    w->count = count;
    w->ragged = world_size != NULL;
    w->uploaded = false;
    w->device_is_newer = false;
    return w;
}

WorldBatch *CreateWorldBatch(const Particle *ps, uint32_t world_size, uint32_t count) {
    NB_CHECK(ps != NULL, "NULL particle array");
    NB_CHECK(count > 0 && count <= NB_HIP_BATCH_MAX_COUNT, "count %u outside 1 .. %u", count, NB_HIP_BATCH_MAX_COUNT);
    NB_CHECK(world_size > 0 && world_size <= NB_HIP_BATCH_MAX_LEN, "world_size %u outside 1 .. %u", world_size, NB_HIP_BATCH_MAX_LEN);
    WorldBatch *w = make_batch(ps, NULL, world_size, count);
    w->gpu = nb_hip_batch_create(count, world_size, w->massive);
    return w;
}

WorldBatch *CreateWorldBatchRagged(const Particle *ps, const uint32_t *world_size, uint32_t count) {
    NB_CHECK(count > 0 && count <= NB_HIP_BATCH_MAX_COUNT, "count %u outside 1 .. %u", count, NB_HIP_BATCH_MAX_COUNT);
    NB_CHECK(ps != NULL && world_size != NULL, "NULL argument");
    for (uint32_t b = 0; b < count; b++)
        NB_CHECK(world_size[b] > 0 && world_size[b] <= NB_HIP_BATCH_MAX_LEN, "member %u: world_size %u outside 1 .. %u", b, world_size[b],
                 NB_HIP_BATCH_MAX_LEN);
    WorldBatch *w = make_batch(ps, world_size, 0, count);
    w->gpu = nb_hip_ragged_create(count, w->sizes, w->massive);
    return w;
}

static void check_not_ragged(const WorldBatch *w, const char *what) {
    NB_CHECK(w == NULL || !w->ragged, "%s: rendering of ragged ensembles (members of different sizes) is not supported", what);
}

void DestroyWorldBatch(WorldBatch *w) {
    if (w == NULL) return;
    nb_hip_batch_destroy(w->gpu);
    free(w->particles);
    free(w->massive);
    free(w->sizes);
    free(w->offset);
    free(w);
}

const Particle *GetWorldBatchParticles(WorldBatch *w, uint32_t member, uint32_t *size) {
    NB_CHECK(w != NULL, "NULL WorldBatch");
    NB_CHECK(member < w->count, "member %u of %u", member, w->count);
    if (w->device_is_newer) {
        nb_hip_batch_get_data(w->gpu, w->particles);
        w->device_is_newer = false;
    }
    if (size != NULL) *size = w->sizes[member];
    return w->particles + w->offset[member];
}

static void push_once(WorldBatch *w) {
    if (w->uploaded) return;
    nb_hip_batch_set_data(w->gpu, w->particles);
    w->uploaded = true;
}

void UpdateWorldBatch_GPU(WorldBatch *w, float dt, uint32_t n) {
    NB_CHECK(w != NULL, "NULL WorldBatch");
    if (n == 0) return;
    push_once(w);
    nb_hip_batch_update(w->gpu, n, dt);
    w->device_is_newer = true;
}

void UpdateWorldBatch_GPU_dts(WorldBatch *w, const float *dt, uint32_t n) {
    NB_CHECK(w != NULL && dt != NULL, "NULL argument");
    if (n == 0) return;
    push_once(w);
    nb_hip_batch_update_dts(w->gpu, n, dt);
    w->device_is_newer = true;
}

void UpdateWorldBatch_GPU_Traced(WorldBatch *w, float dt, uint32_t n, uint32_t every, WorldEnergy *out) {
    NB_CHECK(w != NULL && out != NULL, "NULL argument");
    NB_CHECK(every > 0, "every = 0: a traced update records every k >= 1 steps");
    push_once(w);
    nb_hip_ensemble_trace(w->gpu, n, dt, every, out);
    if (n > 0) w->device_is_newer = true;
}

void UpdateWorldBatch_GPU_Traced_dts(WorldBatch *w, const float *dt, uint32_t n, uint32_t every, WorldEnergy *out) {
    NB_CHECK(w != NULL && dt != NULL && out != NULL, "NULL argument");
    NB_CHECK(every > 0, "every = 0: a traced update records every k >= 1 steps");
    push_once(w);
    nb_hip_ensemble_trace_dts(w->gpu, n, dt, every, out);
    if (n > 0) w->device_is_newer = true;
}

void GetWorldBatchEnergy(WorldBatch *w, WorldEnergy *out) {
    NB_CHECK(w != NULL && out != NULL, "NULL argument");
    if (w->device_is_newer) {
        nb_hip_ensemble_energy(w->gpu, out);
        return;
    }
    for (uint32_t b = 0; b < w->count; b++) nb_cpu_energy(w->particles + w->offset[b], w->sizes[b], w->massive[b], out + b);
}

void GetWorldBatchPotential(WorldBatch *w, float *phi) {
    NB_CHECK(w != NULL && phi != NULL, "NULL argument");
    if (w->device_is_newer) {
        nb_hip_ensemble_potential(w->gpu, phi);
        return;
    }
    for (uint32_t b = 0; b < w->count; b++)
        nb_cpu_potential(w->particles + w->offset[b], w->sizes[b], w->massive[b], phi + w->offset[b]);
}

void GetWorldBatchBounds(WorldBatch *w, float *bounds) {
    check_not_ragged(w, "GetWorldBatchBounds");
    NB_CHECK(w != NULL && bounds != NULL, "NULL argument");
    if (w->device_is_newer) {
        nb_hip_ensemble_bounds(w->gpu, bounds);
        return;
    }
    for (uint32_t b = 0; b < w->count; b++) nb_cpu_bounds(w->particles + (size_t)b * w->size, w->size, bounds + (size_t)b * 4);
}

void FitWorldBatchViews(WorldBatch *w, uint32_t width, uint32_t height, RenderView *views) {
    check_not_ragged(w, "FitWorldBatchViews");
    NB_CHECK(w != NULL && views != NULL, "NULL argument");
    float *bounds = NB_NEW((size_t)w->count * 4, float);
    NB_CHECK(bounds != NULL, "Failed to alloc %u bounds", w->count);
    GetWorldBatchBounds(w, bounds);
    for (uint32_t b = 0; b < w->count; b++) nb_fit_view(bounds + (size_t)b * 4, width, height, views + b);
    free(bounds);
}

static void check_views(const WorldBatch *w, const RenderView *views) {
    uint32_t member = 0;
    const char *fault = nb_render_views_fault(views, w->count, &member);
    NB_CHECK(fault == NULL, "invalid RenderView of member %u of %u (%u x %u, zoom %g): %s", member, w->count, views[member].width,
             views[member].height, (double)views[member].zoom, fault);
}

void RenderWorldBatchCounts(WorldBatch *w, const RenderView *views, uint32_t *counts) {
    check_not_ragged(w, "RenderWorldBatchCounts");
    NB_CHECK(w != NULL && views != NULL && counts != NULL, "NULL argument");
    check_views(w, views);
    if (w->device_is_newer) {
        nb_hip_ensemble_render_counts(w->gpu, views, counts);
        return;
    }
    const size_t image = (size_t)views[0].width * views[0].height * NB_RENDER_CLASSES;
    for (uint32_t b = 0; b < w->count; b++)
        nb_cpu_render_counts(w->particles + (size_t)b * w->size, w->size, views + b, counts + (size_t)b * image);
}

void RenderWorldBatch(WorldBatch *w, const RenderView *views, const RenderPalette *palette, uint8_t *rgba) {
    check_not_ragged(w, "RenderWorldBatch");
    NB_CHECK(w != NULL && views != NULL && rgba != NULL, "NULL argument");
    check_views(w, views);
    RenderPalette pal;
    if (palette)
        pal = *palette;
    else
        DefaultRenderPalette(&pal);
    NB_CHECK(pal.saturation >= 1u, "RenderPalette saturation must be at least 1");
    if (w->device_is_newer) {
        nb_hip_ensemble_render_rgba(w->gpu, views, &pal, rgba);
        return;
    }
    const size_t frame = (size_t)views[0].width * views[0].height * 4;
    for (uint32_t b = 0; b < w->count; b++)
        nb_cpu_render_rgba(w->particles + (size_t)b * w->size, w->size, views + b, &pal, rgba + (size_t)b * frame);
}

/* ---- include/nbody_adaptive.h ---------------------------------------------------------------------------------------- */

static void check_adaptive_batch(const WorldBatch *w, uint32_t n, const NbAdaptive *cfg, const char *what) {
    NB_CHECK(w != NULL && cfg != NULL, "%s: NULL argument", what);
    const char *fault = nb_timestep_cfg_fault(cfg);
    NB_CHECK(fault == NULL, "%s: %s (eta %g, dt_min %g, dt_max %g, span %g)", what, fault, (double)cfg->eta, (double)cfg->dt_min,
             (double)cfg->dt_max, cfg->span);
    NB_CHECK(n <= NB_ADAPT_MAX_STEPS, "%s: %u steps > 2^20 in one call", what, n);
    NB_CHECK(!w->ragged, "%s: adaptive steps of ragged ensembles (members of different sizes) are not supported", what);
}

void UpdateWorldBatch_GPU_Adaptive(WorldBatch *w, uint32_t n, const NbAdaptive *cfg, float *dt_log, NbAdaptiveResult *out) {
    check_adaptive_batch(w, n, cfg, "UpdateWorldBatch_GPU_Adaptive");
    if (out) memset(out, 0, (size_t)w->count * sizeof *out);
    if (n == 0) return;
    push_once(w);
    nb_hip_ensemble_adaptive_steps(w->gpu, n, cfg, dt_log, out);
    w->device_is_newer = true;
}

void AdvanceWorldBatch_GPU(WorldBatch *w, double span, const NbAdaptive *cfg, uint32_t max_steps, float *dt_log, NbAdaptiveResult *out) {
    NB_CHECK(cfg != NULL, "AdvanceWorldBatch_GPU: NULL argument");
    NbAdaptive c = *cfg;
    c.span = span;
    c.flags &= ~NB_ADAPT_CONTINUE;   /* an advance starts its own clocks; its inner calls then continue them on the device */
    check_adaptive_batch(w, max_steps, &c, "AdvanceWorldBatch_GPU");
    const uint32_t chunk = cfg->chunk ? cfg->chunk : 64u;
    NbAdaptiveResult *total = NB_NEW(w->count, NbAdaptiveResult);
    NB_CHECK(total != NULL, "Failed to alloc the results of %u members", w->count);
    memset(total, 0, (size_t)w->count * sizeof *total);
    uint32_t done = 0, next = 1;
    bool unfinished = true;
    while (done < max_steps && unfinished) {
        const uint32_t k = next < max_steps - done ? next : max_steps - done;
        /* cumulative per member: the device keeps every member's clock, a finished member takes idle steps */
        UpdateWorldBatch_GPU_Adaptive(w, k, &c, dt_log ? dt_log + (size_t)done * w->count : NULL, total);
        c.flags = (c.flags & ~NB_ADAPT_PRIME) | NB_ADAPT_CONTINUE;
        done += k;
        double want = 1.0;
        unfinished = false;
        for (uint32_t b = 0; b < w->count; b++) {
            if (!(total[b].elapsed < span)) continue;
            unfinished = true;
            const double left = total[b].dt_last > 0.0f ? floor((span - total[b].elapsed) / (double)total[b].dt_last) : 1.0;
            if (left > want) want = left;
        }
        next = want > (double)chunk ? chunk : (uint32_t)want;
    }
    if (out) memcpy(out, total, (size_t)w->count * sizeof *out);
    free(total);
}

/* ---- include/nbody_leapfrog.h ---------------------------------------------------------------------------------------- */

void UpdateWorldBatch_GPU_Leapfrog(WorldBatch *w, float dt, uint32_t n) {
    NB_CHECK(w != NULL, "UpdateWorldBatch_GPU_Leapfrog: NULL argument");
    NB_CHECK(!w->ragged, "UpdateWorldBatch_GPU_Leapfrog: leapfrog steps of ragged ensembles (members of different sizes) are not supported");
    if (n == 0) return;
    push_once(w);
    nb_hip_ensemble_leapfrog(w->gpu, n, dt);
    w->device_is_newer = true;
}

void UpdateWorldBatch_GPU_Leapfrog_dts(WorldBatch *w, const float *dt, uint32_t n) {
    NB_CHECK(w != NULL && dt != NULL, "UpdateWorldBatch_GPU_Leapfrog_dts: NULL argument");
    NB_CHECK(!w->ragged, "UpdateWorldBatch_GPU_Leapfrog_dts: leapfrog steps of ragged ensembles (members of different sizes) are not supported");
    if (n == 0) return;
    push_once(w);
    nb_hip_ensemble_leapfrog_dts(w->gpu, n, dt);
    w->device_is_newer = true;
}

/* ---- include/nbody_batch_field.h, include/nbody_batch_tidal.h -------------------------------------------------------- */

static void check_field(const char *what, float softening, uint64_t samples) {
    const char *fault = nb_field_fault(softening, samples);
    NB_CHECK(fault == NULL, "%s: invalid call (softening %g, %llu points in all): %s", what, (double)softening, (unsigned long long)samples,
             fault);
}

/* n probes of every member into phi[] (the potential) or, where phi is NULL, into acc[] or, where both are NULL, into tid[] */
static void batch_field_at(WorldBatch *w, const char *what, const V2 *points, uint32_t n, float softening, float *phi, V2 *acc,
                           TidalTensor *tid) {
    NB_CHECK(w != NULL, "%s: NULL argument", what);
    check_field(what, softening, (uint64_t)w->count * n);
    NB_CHECK((points != NULL && (phi != NULL || acc != NULL || tid != NULL)) || n == 0, "%s: NULL argument", what);
    if (n == 0) return;
    if (w->device_is_newer) {
        if (phi)
            nb_hip_ensemble_potential_at(w->gpu, (const float *)points, n, softening, phi);
        else if (acc)
            nb_hip_ensemble_acceleration_at(w->gpu, (const float *)points, n, softening, (float *)acc);
        else
            nb_hip_ensemble_tidal_at(w->gpu, (const float *)points, n, softening, (float *)tid);
        return;
    }
    for (uint32_t b = 0; b < w->count; b++) {
        const Particle *ps = w->particles + w->offset[b];
        const size_t at = (size_t)b * n;
        if (phi)
            nb_cpu_potential_at(ps, w->massive[b], points + at, n, softening, phi + at);
        else if (acc)
            nb_cpu_acceleration_at(ps, w->massive[b], points + at, n, softening, acc + at);
        else
            nb_cpu_tidal_at(ps, w->massive[b], points + at, n, softening, tid + at);
    }
}

/* the map of every member under its view into phi[] or, where phi is NULL, into acc[] or, where both are NULL, into tid[] */
static void batch_field_map(WorldBatch *w, const char *what, const RenderView *views, float softening, float *phi, V2 *acc,
                            TidalTensor *tid) {
    NB_CHECK(w != NULL && views != NULL && (phi != NULL || acc != NULL || tid != NULL), "%s: NULL argument", what);
    check_views(w, views);
    const size_t image = (size_t)views[0].width * views[0].height;
    check_field(what, softening, (uint64_t)w->count * image);
    if (w->device_is_newer) {
        if (phi)
            nb_hip_ensemble_potential_map(w->gpu, views, softening, phi);
        else if (acc)
            nb_hip_ensemble_acceleration_map(w->gpu, views, softening, (float *)acc);
        else
            nb_hip_ensemble_tidal_map(w->gpu, views, softening, (float *)tid);
        return;
    }
    for (uint32_t b = 0; b < w->count; b++) {
        const Particle *ps = w->particles + w->offset[b];
        if (phi)
            nb_cpu_potential_map(ps, w->massive[b], views + b, softening, phi + (size_t)b * image);
        else if (acc)
            nb_cpu_acceleration_map(ps, w->massive[b], views + b, softening, acc + (size_t)b * image);
        else
            nb_cpu_tidal_map(ps, w->massive[b], views + b, softening, tid + (size_t)b * image);
    }
}

void GetWorldBatchPotentialAt(WorldBatch *w, const V2 *points, uint32_t n, float softening, float *phi) {
    batch_field_at(w, "GetWorldBatchPotentialAt", points, n, softening, phi, NULL, NULL);
}

void RenderWorldBatchPotential(WorldBatch *w, const RenderView *views, float softening, float *phi) {
    batch_field_map(w, "RenderWorldBatchPotential", views, softening, phi, NULL, NULL);
}

void GetWorldBatchAccelerationAt(WorldBatch *w, const V2 *points, uint32_t n, float softening, V2 *acc) {
    batch_field_at(w, "GetWorldBatchAccelerationAt", points, n, softening, NULL, acc, NULL);
}

void RenderWorldBatchAcceleration(WorldBatch *w, const RenderView *views, float softening, V2 *acc) {
    batch_field_map(w, "RenderWorldBatchAcceleration", views, softening, NULL, acc, NULL);
}

void GetWorldBatchTidalAt(WorldBatch *w, const V2 *points, uint32_t n, float softening, TidalTensor *t) {
    batch_field_at(w, "GetWorldBatchTidalAt", points, n, softening, NULL, NULL, t);
}

void RenderWorldBatchTidal(WorldBatch *w, const RenderView *views, float softening, TidalTensor *t) {
    batch_field_map(w, "RenderWorldBatchTidal", views, softening, NULL, NULL, t);
}

/* ---- include/nbody_batch_profile.h ----------------------------------------------------------------------------------- */

void GetWorldBatchProfile(WorldBatch *w, const WorldProfileSpec *specs, uint32_t nspecs, double *out, uint32_t *unplaced) {
    NB_CHECK(w != NULL && specs != NULL && specs[0].edges != NULL && out != NULL, "GetWorldBatchProfile: NULL argument");
    NB_CHECK(nspecs == 1 || nspecs == w->count, "GetWorldBatchProfile: %u specs for %u members (one for all, or one each)", nspecs, w->count);
    const float *edges = specs[0].edges;
    const uint32_t bins = specs[0].bins;
    const int weights = specs[0].weights;
    float *centres = NB_NEW((size_t)w->count * 4, float);
    NB_CHECK(centres != NULL, "Failed to alloc %u centres", w->count);
    for (uint32_t b = 0; b < w->count; b++) {
        const WorldProfileSpec *s = specs + (nspecs == 1 ? 0 : b);
        centres[4 * b + 0] = s->centre[0];
        centres[4 * b + 1] = s->centre[1];
        centres[4 * b + 2] = s->centre_velocity[0];
        centres[4 * b + 3] = s->centre_velocity[1];
    }
    const char *fault = nb_profile_fault(edges, bins, centres, w->count, weights);
    NB_CHECK(fault == NULL, "GetWorldBatchProfile: %s (bins %u, weights %d)", fault, bins, weights);
    for (uint32_t b = 1; b < nspecs; b++) {
        NB_CHECK(specs[b].edges != NULL, "GetWorldBatchProfile: NULL argument");
        NB_CHECK(specs[b].bins == bins && specs[b].weights == weights &&
                     (specs[b].edges == edges || memcmp(specs[b].edges, edges, ((size_t)bins + 1) * sizeof(float)) == 0),
                 "GetWorldBatchProfile: the spec of member %u differs from member 0's in its edges or weights: per-member edges are "
                 "not supported", b);
    }
    if (w->device_is_newer) {
        nb_hip_ensemble_profile(w->gpu, edges, bins, centres, weights, out, unplaced);
    } else {
        const size_t cells = ((size_t)bins + 2) * NB_PROFILE_QTY;
        for (uint32_t b = 0; b < w->count; b++)
            nb_cpu_profile(w->particles + w->offset[b], w->sizes[b], w->massive[b], edges, bins, centres + 4 * b, weights, out + b * cells,
                           unplaced ? unplaced + b : NULL);
    }
    free(centres);
}

/* ---- include/nbody_batch_paircount.h --------------------------------------------------------------------------------- */

void GetWorldBatchPairCounts(WorldBatch *w, const WorldPairSpec *spec, uint64_t *out, uint64_t *unplaced) {
    NB_CHECK(w != NULL && spec != NULL && spec->edges != NULL && out != NULL, "GetWorldBatchPairCounts: NULL argument");
    const char *fault = nb_pair_fault(spec->edges, spec->bins, spec->classes);
    NB_CHECK(fault == NULL, "GetWorldBatchPairCounts: %s (bins %u, classes %u)", fault, spec->bins, spec->classes);
    if (w->device_is_newer) {
        nb_hip_ensemble_pair_counts(w->gpu, spec->edges, spec->bins, spec->classes, out, unplaced);
    } else {
        const size_t cells = ((size_t)spec->bins + 2) * NB_PAIRS_COLUMNS;
        for (uint32_t b = 0; b < w->count; b++)
            nb_cpu_pair_counts(w->particles + w->offset[b], w->sizes[b], w->massive[b], spec->edges, spec->bins, spec->classes, out + b * cells,
                               unplaced ? unplaced + (size_t)b * NB_PAIRS_COLUMNS : NULL);
    }
}

/* ---- include/nbody_batch_neighbour.h --------------------------------------------------------------------------------- */

void GetWorldBatchNeighbours(WorldBatch *w, const WorldNeighbourSpec *spec, float *q, uint32_t *index, uint32_t *count) {
    NB_CHECK(w != NULL && spec != NULL && q != NULL && index != NULL, "GetWorldBatchNeighbours: NULL argument");
    const char *fault = nb_neigh_fault(spec->receivers, spec->sources, spec->radius, count != NULL);
    NB_CHECK(fault == NULL, "GetWorldBatchNeighbours: %s (receivers %u, sources %u, radius %g)", fault, spec->receivers, spec->sources,
             (double)spec->radius);
    if (w->device_is_newer) {
        nb_hip_ensemble_neighbours(w->gpu, spec->receivers, spec->sources, spec->radius, q, index, count);
    } else {
        for (uint32_t b = 0; b < w->count; b++)
            nb_cpu_neighbours(w->particles + w->offset[b], w->sizes[b], w->massive[b], spec->receivers, spec->sources, spec->radius, q + w->offset[b],
                              index + w->offset[b], count ? count + w->offset[b] : NULL);
    }
}

/* ---- include/nbody_batch_group.h ------------------------------------------------------------------------------------- */

void GetWorldBatchGroups(WorldBatch *w, const WorldGroupSpec *spec, uint32_t *group, uint32_t *n_groups) {
    NB_CHECK(w != NULL && spec != NULL && group != NULL, "GetWorldBatchGroups: NULL argument");
    const char *fault = nb_group_fault(spec->members, spec->linking_length);
    NB_CHECK(fault == NULL, "GetWorldBatchGroups: %s (members %u, linking_length %g)", fault, spec->members, (double)spec->linking_length);
    if (w->device_is_newer) {
        nb_hip_ensemble_groups(w->gpu, spec->members, spec->linking_length, group, n_groups);
    } else {
        for (uint32_t b = 0; b < w->count; b++)
            nb_cpu_groups(w->particles + w->offset[b], w->sizes[b], w->massive[b], spec->members, spec->linking_length, group + w->offset[b],
                          n_groups ? n_groups + b : NULL);
    }
}
