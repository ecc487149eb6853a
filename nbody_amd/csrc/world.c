/*
 * world.c -- the include/nbody.h surface: World, its mass partition, and the
 * lazy host<->device coherence between the particle array and the HIP pipeline.
 *
 * Follows the behaviour of the reference's src/lib/world.c:
 *   - CreateWorld copies the caller's particles and partitions them "mass > 0
 *     first" with the reference's two-cursor swap scheme (world.c:32-46), because
 *     that exact permutation is the index order every later read returns
 *     (pinned by reference test/test_particle_sort.c:27-111);
 *   - two dirty flags decide when data crosses PCIe (world.c:18-19,76-89): the
 *     array is uploaded only if the CPU side changed it since the last GPU step,
 *     and downloaded only when GetWorldParticles / UpdateWorld_CPU needs it;
 *   - UpdateWorld_GPU(n == 0) does nothing (world.c:113); UpdateWorld_CPU(n == 0)
 *     still pulls the device state and marks the array dirty (world.c:100,109).
 * Differences: the GPU side is created lazily (no device is touched by a World
 * that only ever steps on the CPU), and DestroyWorld frees the particle array
 * (the reference leaks it, world.c:67-73).
 * Extension (include/nbody_diag.h): GetWorldEnergy / GetWorldPotential compute
 * on the device when it holds the newest state, without pulling the array, and
 * on the host (diag_cpu.c) otherwise; neither moves a dirty flag.
 * Extension (include/nbody_render.h): GetWorldBounds / FitWorldView /
 * RenderWorldCounts / RenderWorld follow the same rule (render.hip and the
 * kernels of render_kernels.hip on the device, render_cpu.c on the host).
 * Extension (include/nbody_field.h): GetWorldPotentialAt / RenderWorldPotential
 * follow the same rule (field.hip on the device, field_cpu.c on the host).
 * Extension (include/nbody_gravity.h): GetWorldAccelerationAt /
 * RenderWorldAcceleration likewise (the same two files).
 * Extension (include/nbody_tidal.h): GetWorldTidalAt / RenderWorldTidal
 * likewise (tidal.hip on the device, field_cpu.c on the host).
 * Extension (include/nbody_profile.h): GetWorldProfile follows the diagnostics'
 * rule (profile.hip on the device, profile_cpu.c on the host).
 * Extension (include/nbody_paircount.h): GetWorldPairCounts likewise
 * (paircount.hip on the device, paircount_cpu.c on the host).
 * Extension (include/nbody_neighbour.h): GetWorldNeighbours likewise
 * (neighbour.hip on the device, neighbour_cpu.c on the host).
 * Extension (include/nbody_group.h): GetWorldGroups likewise
 * (group.hip on the device, group_cpu.c on the host).
 * Extension (include/nbody_adaptive.h): adaptive steps.  UpdateWorld_GPU_Adaptive
 * and AdvanceWorld_GPU follow UpdateWorld_GPU's coherence rules, UpdateWorld_CPU_Adaptive
 * UpdateWorld_CPU's; GetWorldTimestep follows the diagnostics' (timestep.hip on the
 * device, timestep_cpu.c on the host).
 * Extension (include/nbody_leapfrog.h): kick-drift-kick steps.  UpdateWorld_GPU_Leapfrog
 * follows UpdateWorld_GPU's coherence rules, UpdateWorld_CPU_Leapfrog UpdateWorld_CPU's
 * (leapfrog.hip on the device, leapfrog_cpu.c around UpdateWorld_CPU(w, 0, 1) on the host);
 * whether acc belongs to the state is remembered per side, so a transfer primes again.
 */
#include "nbody.h"
#include "nbody_adaptive.h"
#include "nbody_diag.h"
#include "nbody_field.h"
#include "nbody_gravity.h"
#include "nbody_tidal.h"
#include "nbody_profile.h"
#include "nbody_paircount.h"
#include "nbody_neighbour.h"
#include "nbody_group.h"
#include "nbody_hip.h"
#include "nbody_leapfrog.h"
#include "nbody_render.h"

#include <stdbool.h>

#include "diag_sums.h"
#include "field_common.h"
#include "leapfrog_common.h"
#include "profile_common.h"
#include "paircount_common.h"
#include "neighbour_common.h"
#include "group_common.h"
#include "render_common.h"
#include "nb_util.h"
#include "sim_cpu.h"
#include "timestep_common.h"
#include "world_partition.h"

struct World {
    Particle *particles;  /* partitioned copy of the caller's array */
    uint32_t count;       /* all particles */
    uint32_t massive;     /* particles with mass > 0; they occupy [0, massive) */
    SimPipeline *gpu;     /* HIP pipeline (include/nbody_hip.h) */
    CpuSim *cpu;          /* host-core stepper */
    bool host_is_newer;   /* array changed since the device last saw it */
    bool device_is_newer; /* device stepped since the array was last refreshed */
    int nranks;           /* > 1: sharded (the pipeline holds 1/nranks of the receivers) */
    bool cpu_acc_current; /* the array's acc is F(x) of the array's state: true after a CPU leapfrog call only (the device
                             side of the same knowledge lives in the pipeline) */
};

/* leapfrog_cpu.c */
__attribute__((visibility("hidden"))) void nb_cpu_leapfrog_open(Particle *ps, uint32_t n, float dt);
__attribute__((visibility("hidden"))) void nb_cpu_leapfrog_close(Particle *ps, uint32_t n, float dt);

/* rank < 0: an ordinary single-GPU World; otherwise the sharded pipeline of include/nbody_hip.h. */
static World *create_world(const Particle *ps, uint32_t size, int rank, int nranks, const void *unique_id128,
                           NbAllGatherFn allgather, void *ctx, bool direct) {
    World *w = NB_NEW(1, World);
    NB_CHECK(w != NULL, "Failed to alloc World");
    w->particles = NB_NEW(size ? size : 1, Particle);
    NB_CHECK(w->particles != NULL, "Failed to alloc %u particles", size);
    if (size) memcpy(w->particles, ps, (size_t)size * sizeof(Particle));

    w->count = size;
    w->massive = partition_by_mass(w->particles, size);
    const WorldData data = {.total_len = size, .mass_len = w->massive, .dt = 0.0f};
    w->gpu = rank < 0     ? CreateSimPipeline(data)
             : direct    ? CreateSimPipelineShardedDirect(data, rank, nranks, allgather, ctx)
             : allgather ? CreateSimPipelineShardedWith(data, rank, nranks, allgather, ctx)
                         : CreateSimPipelineSharded(data, rank, nranks, unique_id128);
    /* this array is what every later Set/GetSimulationData moves: let the pipeline page-lock it when (if) it
     * first touches the GPU.  DestroyWorld destroys the pipeline before freeing the array. */
    nb_hip_note_host_array(w->gpu, w->particles, (uint64_t)size * sizeof(Particle));
    w->cpu = CpuSimCreate(w->massive);
    w->host_is_newer = true;    /* the device has seen nothing yet */
    w->device_is_newer = false;
    w->nranks = rank < 0 ? 1 : nranks;
    w->cpu_acc_current = false;
    return w;
}

World *CreateWorld(const Particle *ps, uint32_t size) { return create_world(ps, size, -1, 1, NULL, NULL, NULL, false); }

/*
 * Extension: one World per process and GPU.  The partition is deterministic, so every rank derives the same
 * mass_len and the same index order from the same input; the pipeline then owns the rank's 1/P of the receivers
 * (nb_hip_shard_plan) and the coherence protocol above is unchanged -- Set/Get/Perform are simply collectives.
 */
World *CreateWorldSharded(const Particle *ps, uint32_t size, int rank, int nranks, const void *unique_id128) {
    NB_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, "rank %d of %d", rank, nranks);
    return create_world(ps, size, rank, nranks, unique_id128, NULL, NULL, false);
}

/* Extension: the same over a caller-supplied host all-gather (several ranks on ONE GPU, machines without RCCL). */
World *CreateWorldShardedWith(const Particle *ps, uint32_t size, int rank, int nranks, NbAllGatherFn allgather, void *ctx) {
    NB_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, "rank %d of %d", rank, nranks);
    NB_CHECK(allgather != NULL, "NULL all-gather callback");
    return create_world(ps, size, rank, nranks, NULL, allgather, ctx, false);
}

/* Extension: the same with the direct device-to-device exchange; `control` carries handles and barriers only. */
World *CreateWorldShardedDirect(const Particle *ps, uint32_t size, int rank, int nranks, NbAllGatherFn control, void *ctx) {
    NB_CHECK(nranks >= 1 && rank >= 0 && rank < nranks, "rank %d of %d", rank, nranks);
    NB_CHECK(control != NULL, "NULL control callback");
    return create_world(ps, size, rank, nranks, NULL, control, ctx, true);
}

SimPipeline *GetWorldPipeline(World *w) { return w ? w->gpu : NULL; }

void DestroyWorld(World *w) {
    if (w == NULL) return;
    DestroySimPipeline(w->gpu);
    CpuSimDestroy(w->cpu);
    free(w->particles);
    free(w);
}

static void push_if_stale(World *w) {
    if (!w->host_is_newer) return;
    SetSimulationData(w->gpu, w->particles);
    w->host_is_newer = false;
}

static void pull_if_stale(World *w) {
    if (!w->device_is_newer) return;
    GetSimulationData(w->gpu, w->particles);
    w->device_is_newer = false;
    w->cpu_acc_current = false;
}

const Particle *GetWorldParticles(World *w, uint32_t *size) {
    pull_if_stale(w);
    if (size != NULL) *size = w->count;
    return w->particles;
}

void UpdateWorld_CPU(World *w, float dt, uint32_t n) {
    pull_if_stale(w);
    for (uint32_t step = 0; step < n; step++) CpuSimStep(w->cpu, w->particles, w->count, w->massive, dt);
    w->host_is_newer = true;
    w->cpu_acc_current = false;   /* an Euler step leaves the acc of the state before it */
}

void UpdateWorld_GPU(World *w, float dt, uint32_t n) {
    if (n == 0) return;
    push_if_stale(w);
    PerformSimUpdate(w->gpu, n, dt);
    w->device_is_newer = true;
}

/* The device holds the newest state whenever the array has not changed since it was last pushed (the device may have
 * stepped further).  A World that never stepped on the GPU keeps host_is_newer and never reaches the device here. */
static bool diag_on_device(World *w, const char *what) {
    NB_CHECK(w->nranks <= 1, "%s of a sharded pipeline needs a collective over the ranks: not supported", what);
    return !w->host_is_newer;
}

void GetWorldEnergy(World *w, WorldEnergy *out) {
    NB_CHECK(w != NULL && out != NULL, "NULL argument");
    if (diag_on_device(w, "GetWorldEnergy"))
        nb_hip_energy(w->gpu, out);
    else
        nb_cpu_energy(w->particles, w->count, w->massive, out);
}

void GetWorldPotential(World *w, float *phi) {
    NB_CHECK(w != NULL && (phi != NULL || w->count == 0), "NULL argument");
    if (diag_on_device(w, "GetWorldPotential"))
        nb_hip_potential(w->gpu, phi);
    else
        nb_cpu_potential(w->particles, w->count, w->massive, phi);
}

void GetWorldBounds(World *w, float *bounds) {
    NB_CHECK(w != NULL && bounds != NULL, "NULL argument");
    if (diag_on_device(w, "GetWorldBounds"))
        nb_hip_bounds(w->gpu, bounds);
    else
        nb_cpu_bounds(w->particles, w->count, bounds);
}

void FitWorldView(World *w, uint32_t width, uint32_t height, RenderView *view) {
    float bounds[4];
    GetWorldBounds(w, bounds);
    nb_fit_view(bounds, width, height, view);
}

void RenderWorldCounts(World *w, const RenderView *view, uint32_t *counts) {
    NB_CHECK(w != NULL && view != NULL && counts != NULL, "NULL argument");
    if (diag_on_device(w, "RenderWorldCounts"))
        nb_hip_render_counts(w->gpu, view, counts);
    else
        nb_cpu_render_counts(w->particles, w->count, view, counts);
}

void RenderWorld(World *w, const RenderView *view, const RenderPalette *palette, uint8_t *rgba) {
    NB_CHECK(w != NULL && view != NULL && rgba != NULL, "NULL argument");
    RenderPalette pal;
    if (palette)
        pal = *palette;
    else
        DefaultRenderPalette(&pal);
    if (diag_on_device(w, "RenderWorld"))
        nb_hip_render_rgba(w->gpu, view, &pal, rgba);
    else
        nb_cpu_render_rgba(w->particles, w->count, view, &pal, rgba);
}

void GetWorldPotentialAt(World *w, const V2 *points, uint32_t n, float softening, float *phi) {
    NB_CHECK(w != NULL && ((points != NULL && phi != NULL) || n == 0), "NULL argument");
    if (diag_on_device(w, "GetWorldPotentialAt"))
        nb_hip_potential_at(w->gpu, (const float *)points, n, softening, phi);
    else
        nb_cpu_potential_at(w->particles, w->massive, points, n, softening, phi);
}

void RenderWorldPotential(World *w, const RenderView *view, float softening, float *phi) {
    NB_CHECK(w != NULL && view != NULL && phi != NULL, "NULL argument");
    if (diag_on_device(w, "RenderWorldPotential"))
        nb_hip_potential_map(w->gpu, view, softening, phi);
    else
        nb_cpu_potential_map(w->particles, w->massive, view, softening, phi);
}

void GetWorldAccelerationAt(World *w, const V2 *points, uint32_t n, float softening, V2 *acc) {
    NB_CHECK(w != NULL && ((points != NULL && acc != NULL) || n == 0), "NULL argument");
    if (diag_on_device(w, "GetWorldAccelerationAt"))
        nb_hip_acceleration_at(w->gpu, (const float *)points, n, softening, (float *)acc);
    else
        nb_cpu_acceleration_at(w->particles, w->massive, points, n, softening, acc);
}

void RenderWorldAcceleration(World *w, const RenderView *view, float softening, V2 *acc) {
    NB_CHECK(w != NULL && view != NULL && acc != NULL, "NULL argument");
    if (diag_on_device(w, "RenderWorldAcceleration"))
        nb_hip_acceleration_map(w->gpu, view, softening, (float *)acc);
    else
        nb_cpu_acceleration_map(w->particles, w->massive, view, softening, acc);
}

void GetWorldTidalAt(World *w, const V2 *points, uint32_t n, float softening, TidalTensor *t) {
    NB_CHECK(w != NULL && ((points != NULL && t != NULL) || n == 0), "NULL argument");
    if (diag_on_device(w, "GetWorldTidalAt"))
        nb_hip_tidal_at(w->gpu, (const float *)points, n, softening, (float *)t);
    else
        nb_cpu_tidal_at(w->particles, w->massive, points, n, softening, t);
}

void RenderWorldTidal(World *w, const RenderView *view, float softening, TidalTensor *t) {
    NB_CHECK(w != NULL && view != NULL && t != NULL, "NULL argument");
    if (diag_on_device(w, "RenderWorldTidal"))
        nb_hip_tidal_map(w->gpu, view, softening, (float *)t);
    else
        nb_cpu_tidal_map(w->particles, w->massive, view, softening, t);
}

/* ---- include/nbody_profile.h ----------------------------------------------------------------------------------------- */

void GetWorldProfile(World *w, const WorldProfileSpec *spec, double *out, uint32_t *unplaced) {
    NB_CHECK(w != NULL && spec != NULL && spec->edges != NULL && out != NULL, "NULL argument");
    const float centre[4] = {spec->centre[0], spec->centre[1], spec->centre_velocity[0], spec->centre_velocity[1]};
    const char *fault = nb_profile_fault(spec->edges, spec->bins, centre, 1, spec->weights);
    NB_CHECK(fault == NULL, "GetWorldProfile: %s (bins %u, weights %d)", fault, spec->bins, spec->weights);
    if (diag_on_device(w, "GetWorldProfile"))
        nb_hip_profile(w->gpu, spec->edges, spec->bins, centre, spec->weights, out, unplaced);
    else
        nb_cpu_profile(w->particles, w->count, w->massive, spec->edges, spec->bins, centre, spec->weights, out, unplaced);
}

/* ---- include/nbody_paircount.h --------------------------------------------------------------------------------------- */

void GetWorldPairCounts(World *w, const WorldPairSpec *spec, uint64_t *out, uint64_t *unplaced) {
    NB_CHECK(w != NULL && spec != NULL && spec->edges != NULL && out != NULL, "NULL argument");
    const char *fault = nb_pair_fault(spec->edges, spec->bins, spec->classes);
    NB_CHECK(fault == NULL, "GetWorldPairCounts: %s (bins %u, classes %u)", fault, spec->bins, spec->classes);
    if (diag_on_device(w, "GetWorldPairCounts"))
        nb_hip_pair_counts(w->gpu, spec->edges, spec->bins, spec->classes, out, unplaced);
    else
        nb_cpu_pair_counts(w->particles, w->count, w->massive, spec->edges, spec->bins, spec->classes, out, unplaced);
}

/* ---- include/nbody_neighbour.h --------------------------------------------------------------------------------------- */

void GetWorldNeighbours(World *w, const WorldNeighbourSpec *spec, float *q, uint32_t *index, uint32_t *count) {
    NB_CHECK(w != NULL && spec != NULL && q != NULL && index != NULL, "NULL argument");
    const char *fault = nb_neigh_fault(spec->receivers, spec->sources, spec->radius, count != NULL);
    NB_CHECK(fault == NULL, "GetWorldNeighbours: %s (receivers %u, sources %u, radius %g)", fault, spec->receivers, spec->sources, (double)spec->radius);
    if (diag_on_device(w, "GetWorldNeighbours"))
        nb_hip_neighbours(w->gpu, spec->receivers, spec->sources, spec->radius, q, index, count);
    else
        nb_cpu_neighbours(w->particles, w->count, w->massive, spec->receivers, spec->sources, spec->radius, q, index, count);
}

/* ---- include/nbody_group.h ------------------------------------------------------------------------------------------- */

void GetWorldGroups(World *w, const WorldGroupSpec *spec, uint32_t *group, uint32_t *n_groups) {
    NB_CHECK(w != NULL && spec != NULL && group != NULL, "NULL argument");
    const char *fault = nb_group_fault(spec->members, spec->linking_length);
    NB_CHECK(fault == NULL, "GetWorldGroups: %s (members %u, linking_length %g)", fault, spec->members, (double)spec->linking_length);
    if (diag_on_device(w, "GetWorldGroups"))
        nb_hip_groups(w->gpu, spec->members, spec->linking_length, group, n_groups);
    else
        nb_cpu_groups(w->particles, w->count, w->massive, spec->members, spec->linking_length, group, n_groups);
}

/* ---- include/nbody_adaptive.h ---------------------------------------------------------------------------------------- */

static void check_adaptive_world(const World *w, uint32_t n, const NbAdaptive *cfg, const char *what) {
    NB_CHECK(w != NULL && cfg != NULL, "%s: NULL argument", what);
    const char *fault = nb_timestep_cfg_fault(cfg);
    NB_CHECK(fault == NULL, "%s: %s (eta %g, dt_min %g, dt_max %g, span %g)", what, fault, (double)cfg->eta, (double)cfg->dt_min,
             (double)cfg->dt_max, cfg->span);
    NB_CHECK(n <= NB_ADAPT_MAX_STEPS, "%s: %u steps > 2^20 in one call", what, n);
}

/* one kick-drift-kick step of the array, acc being the array's own before and after */
static void cpu_leapfrog_step(World *w, float dt) {
    nb_cpu_leapfrog_open(w->particles, w->count, dt);
    UpdateWorld_CPU(w, 0.0f, 1);
    nb_cpu_leapfrog_close(w->particles, w->count, dt);
    w->cpu_acc_current = true;
}

void GetWorldTimestep(World *w, const NbAdaptive *cfg, float *dt) {
    check_adaptive_world(w, 0, cfg, "GetWorldTimestep");
    NB_CHECK(dt != NULL, "GetWorldTimestep: NULL argument");
    if (diag_on_device(w, "GetWorldTimestep"))
        nb_hip_timestep(w->gpu, cfg, dt);
    else
        *dt = nb_cpu_timestep(w->particles, w->count, cfg);
}

void UpdateWorld_CPU_Adaptive(World *w, uint32_t n, const NbAdaptive *cfg, float *dt_log, NbAdaptiveResult *out) {
    check_adaptive_world(w, n, cfg, "UpdateWorld_CPU_Adaptive");
    NbAdaptiveResult r = {0.0, 0, 0, 0.0f, 0.0f};
    const bool leapfrog = (cfg->flags & NB_ADAPT_LEAPFROG) != 0;
    if (n > 0 && leapfrog) {
        pull_if_stale(w);
        if (!w->cpu_acc_current) UpdateWorld_CPU(w, 0.0f, 1);
    } else if (n > 0 && (cfg->flags & NB_ADAPT_PRIME)) {
        UpdateWorld_CPU(w, 0.0f, 1);
    }
    for (uint32_t i = 0; i < n; i++) {
        float dt;
        GetWorldTimestep(w, cfg, &dt);
        dt = nb_timestep_clip(dt, cfg->span, &r.elapsed);
        nb_timestep_count(dt, &r.steps, &r.idle_steps, &r.dt_last, &r.dt_smallest);
        if (leapfrog)
            cpu_leapfrog_step(w, dt);
        else
            UpdateWorld_CPU(w, dt, 1);
        if (dt_log) dt_log[i] = dt;
    }
    if (out) *out = r;
}

void UpdateWorld_GPU_Adaptive(World *w, uint32_t n, const NbAdaptive *cfg, float *dt_log, NbAdaptiveResult *out) {
    check_adaptive_world(w, n, cfg, "UpdateWorld_GPU_Adaptive");
    NB_CHECK(w->nranks <= 1, "UpdateWorld_GPU_Adaptive of a sharded pipeline needs a collective over the ranks: not supported");
    if (out) memset(out, 0, sizeof *out);
    if (n == 0) return;
    push_if_stale(w);
    nb_hip_adaptive_steps(w->gpu, n, cfg, dt_log, out);
    w->device_is_newer = true;
}

void AdvanceWorld_GPU(World *w, double span, const NbAdaptive *cfg, uint32_t max_steps, float *dt_log, NbAdaptiveResult *out) {
    NB_CHECK(cfg != NULL, "AdvanceWorld_GPU: NULL argument");
    NbAdaptive c = *cfg;
    c.span = span;
    c.flags &= ~NB_ADAPT_CONTINUE;   /* an advance starts its own clock; its inner calls then continue it on the device */
    check_adaptive_world(w, max_steps, &c, "AdvanceWorld_GPU");
    NB_CHECK(w->nranks <= 1, "AdvanceWorld_GPU of a sharded pipeline needs a collective over the ranks: not supported");
    const uint32_t chunk = cfg->chunk ? cfg->chunk : 64u;
    NbAdaptiveResult total = {0.0, 0, 0, 0.0f, 0.0f};
    uint32_t done = 0, next = 1;
    while (done < max_steps && total.elapsed < span) {
        const uint32_t k = next < max_steps - done ? next : max_steps - done;
        UpdateWorld_GPU_Adaptive(w, k, &c, dt_log ? dt_log + done : NULL, &total);   /* cumulative: the device keeps the clock */
        c.flags = (c.flags & ~NB_ADAPT_PRIME) | NB_ADAPT_CONTINUE;
        done += k;
        const double left = total.dt_last > 0.0f ? floor((span - total.elapsed) / (double)total.dt_last) : 1.0;
        next = left < 1.0 ? 1u : left > (double)chunk ? chunk : (uint32_t)left;
    }
    if (out) *out = total;
}

/* ---- include/nbody_leapfrog.h ---------------------------------------------------------------------------------------- */

void UpdateWorld_CPU_Leapfrog(World *w, float dt, uint32_t n) {
    NB_CHECK(w != NULL, "UpdateWorld_CPU_Leapfrog: NULL argument");
    if (n == 0) return;
    pull_if_stale(w);
    if (!w->cpu_acc_current) UpdateWorld_CPU(w, 0.0f, 1);   /* unlogged, uncounted: acc becomes the state's own */
    for (uint32_t i = 0; i < n; i++) cpu_leapfrog_step(w, dt);
}

void UpdateWorld_GPU_Leapfrog(World *w, float dt, uint32_t n) {
    NB_CHECK(w != NULL, "UpdateWorld_GPU_Leapfrog: NULL argument");
    NB_CHECK(w->nranks <= 1, "UpdateWorld_GPU_Leapfrog of a sharded pipeline needs a collective over the ranks: not supported");
    if (n == 0) return;
    push_if_stale(w);
    nb_hip_leapfrog_steps(w->gpu, n, dt);
    w->device_is_newer = true;
}
