/*
 * nbody_hip.h -- C-ABI of the HIP/gfx950 simulation pipeline (libnbody_hip.so).
 *
 * This is the drop-in boundary.  Part 1 is, symbol for symbol, the seam the
 * reference's world layer calls into its Vulkan backend through
 * (reference src/lib/sim_gpu.h:8-42, called from src/lib/world.c:52,69,78,86,115):
 * a maintainer deletes src/lib/sim_gpu.c, src/lib/vulkan_ctx.c and
 * src/shader/particle_cs.glsl, links this library, and world.c is unchanged
 * (INTEGRATION.md shows it; oracle/_ref/libnbody_ref_world.so is exactly that
 * build).  Part 2 adds what a single-queue Vulkan backend had no notion of:
 * device-resident stepping, kernel timing, the N/P sharded multi-GPU
 * pipeline with its per-step all-gather of source positions over RCCL, and
 * ensembles of small worlds stepped by one launch (SimBatch).
 *
 * Plain C types only; no HIP, RCCL or torch types cross this boundary.
 * Error convention = the reference's (src/lib/util.h:17-29,47-60): any failure
 * prints "file:line [func] ..." to stderr and abort()s.  There is NO CPU
 * fallback: a call that needs the GPU aborts when no gfx950 device answers.
 */
#ifndef NBODY_AMD_NBODY_HIP_H
#define NBODY_AMD_NBODY_HIP_H

#include <stdint.h>
#include "nbody.h"
#include "nbody_diag.h" /* WorldEnergy */
#include "nbody_render.h" /* RenderView, RenderPalette */
#include "nbody_adaptive.h" /* NbAdaptive, NbAdaptiveResult */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------- */
/* Part 1: the reference seam (src/lib/sim_gpu.h)                             */
/* ------------------------------------------------------------------------- */

/* Sizes of a world and its step; replaces reference sim_gpu.h:8-12 (the uniform block). */
typedef struct WorldData {
    uint32_t total_len; /* all particles */
    uint32_t mass_len;  /* particles with mass > 0; they come first */
    float dt;           /* cached step size; PerformSimUpdate's dt wins */
} WorldData;

/* One world's device state + launch machinery; replaces reference sim_gpu.h:15. */
typedef struct SimPipeline SimPipeline;

/*
 * Replaces reference sim_gpu.h:21 (CreateSimPipeline, sim_gpu.c:34-221).
 * Allocates nothing on the GPU yet: device selection, HBM buffers and graphs are
 * made at the first SetSimulationData, so a World used only through
 * UpdateWorld_CPU never touches a GPU (SURVEY.md 8b "init side effects").
 */
SimPipeline *CreateSimPipeline(WorldData data);

/* Replaces reference sim_gpu.h:24 (sim_gpu.c:223-247). NULL is accepted. */
void DestroySimPipeline(SimPipeline *sim);

/*
 * Replaces reference sim_gpu.h:27 (sim_gpu.c:249-251): writes total_len
 * Particles (AoS, partitioned order) holding the device's latest state into ps.
 * Here this is where the D2H copy happens (the reference pays it after every
 * PerformSimUpdate, sim_gpu.c:336-341).
 */
void GetSimulationData(const SimPipeline *sim, Particle *ps);

/*
 * Replaces reference sim_gpu.h:30 (sim_gpu.c:253-256): uploads total_len
 * Particles (AoS, already partitioned: ps[i].mass > 0 exactly for i < mass_len)
 * and splits them into the SoA streams the kernels read.
 */
void SetSimulationData(SimPipeline *sim, const Particle *ps);

/*
 * Replaces reference sim_gpu.h:36 (sim_gpu.c:258-361): n > 0 steps of size dt,
 * blocking.  Simulation data must have been set.  n == 0 is a no-op here
 * (the reference documents n > 0; world.c:113 never passes 0).
 *
 * Non-finite state.  A state that has stopped being finite (a close encounter, a bad initial condition, a step size
 * too large) is ordinary data to the step kernels, on every launch shape, in a sharded group and in an ensemble:
 *   - every pos, vel and acc value has the CLASS (finite, +inf, -inf, NaN) that the reference's AVX build gives for the
 *     same input (sim_cpu.c:156-194): the pair term follows the reference through inf and NaN (dx * 0 = NaN for a source
 *     at infinity, 0 * inf = NaN for a coincident pair with no softening, dx * inf for G*m = inf), and the sums keep an
 *     infinite total infinite: the compensation of the block sums is not applied to a total that has left the finite
 *     range, so +-inf plus finite terms stays +-inf and +inf plus -inf is NaN, as in the reference's plain sums;
 *   - finite values stay within the stated tolerance.  A pair term whose factor G*m / (r * r^2)
 *     fp32 cannot hold -- r * r^2 beyond 3.4e38, or the factor below 1.2e-38 -- may come out as anything between 0 and
 *     its float64 value: the reference's form gives exactly 0 (G*m / inf), G*m * rsq * rsq^2 here gives 0 or a denormal;
 *     a pair whose dist^2 + radius is a denormal (below 1.2e-38) is outside as well: v_rsq_f32 takes no denormal input, it
 *     reads it as zero and returns +inf, so the term has the class of a coincident pair with no softening (tests/pair_cases.py
 *     draws this line: every intermediate of the statement normal and finite; inside it, DESIGN.md section 5 "The pair term");
 *   - vel = vel0 + acc * dt and pos = pos0 + vel * dt hold in fp32 wherever the result is not NaN;
 *   - a particle that is no source (mass <= 0) cannot change a bit of any other particle, whatever it holds: the launch
 *     shape depends on the counts only, and a receiver's lanes, pads and neighbours are kept apart by selects, never by
 *     a multiplication with zero;
 *   - an ensemble member's results -- its steps, its energy and potential (include/nbody_diag.h "Non-finite state" holds
 *     per member) and its rows of a traced update -- do not depend on what its neighbours hold, non-finite neighbours
 *     included.
 * Calls whose termination depends on values (the adaptive ones, include/nbody_adaptive.h) state their own edges.
 * tests/test_gpu_nonfinite.py holds every route to this; tests/nonfinite_cases.py is the case table.
 */
void PerformSimUpdate(SimPipeline *sim, uint32_t n, float dt);

/* ------------------------------------------------------------------------- */
/* Part 2: extensions (no reference counterpart)                              */
/* ------------------------------------------------------------------------- */

/* Number of visible HIP devices; 0 when there is none.  Never aborts. */
int nb_hip_device_count(void);

/* Device ordinal this process' pipelines are created on (default: 0, or LOCAL_RANK for sharded ones). */
void nb_hip_set_device(int ordinal);

/* Fills buf (NUL-terminated, at most len bytes) with "name arch CUs clockMHz pci=domain:bus:device"; aborts without a GPU. */
void nb_hip_device_info(char *buf, uint32_t len);

/* PerformSimUpdate without the final host wait: enqueue n steps and return. */
void nb_hip_step_async(SimPipeline *sim, uint32_t n, float dt);

/* Wait for everything enqueued on the pipeline's stream(s). */
void nb_hip_sync(SimPipeline *sim);

/*
 * Device time, in milliseconds, of the force+integrate kernels of the most
 * recent PerformSimUpdate / nb_hip_step_async (HIP events recorded on the
 * launch stream around the step chain; waits for them).  Needs the "timing"
 * knob (nb_hip_configure(sim, "timing", 1)); returns 0 without it.  *launches receives the
 * number of step-kernel launches those events bracket.
 */
double nb_hip_last_step_ms(SimPipeline *sim, uint32_t *launches);

/*
 * Finish-kernel launches inside the interval nb_hip_last_step_ms reports (one per step-kernel launch when the
 * launch shape splits the sources, else 0): the small O(N) kernel that adds the parts and integrates.
 */
uint32_t nb_hip_last_finish_launches(const SimPipeline *sim);

/*
 * Sharded pipelines (plain-launch chains): where the time of the most recent PerformSimUpdate went.  *kernel_ms =
 * sum over its steps of the force+integrate kernels' device time, *comm_ms = sum of the all-gathers' device time
 * (each bracketed by its own HIP event pair on the stream it ran on; in overlap mode the gather runs beside the
 * kernels, so the two do not add up to the wall time).  Returns the number of steps covered (the first 256 of a
 * call); 0 for unsharded pipelines and for chains replayed as a captured hipGraph.
 */
uint32_t nb_hip_last_step_breakdown(SimPipeline *sim, double *kernel_ms, double *comm_ms);

/*
 * What the pipeline's RCCL communicator itself reports (ncclCommCount / ncclCommUserRank / ncclCommCuDevice /
 * ncclGetVersion), the device time of the probe all-gather run at creation, and the file librccl was loaded from.
 * Returns 1 when the pipeline owns a communicator, else 0 (then nranks/rank are the creation arguments).
 * Any out pointer may be NULL.  This is the evidence that N ranks really formed one communicator.
 */
int nb_hip_comm_info(const SimPipeline *sim, int *nranks, int *rank, int *device, int *rccl_version,
                     double *first_gather_ms, char *lib_path, uint32_t len);

/*
 * Bring-up timings of the pipeline's RCCL communicator, taken once at creation: host milliseconds of ncclCommInitRank,
 * device milliseconds of the first (256-byte-per-rank, verified) all-gather including RCCL's lazy channel set-up, and
 * device microseconds of ONE warm 8-byte-per-rank all-gather (mean of 16 issued back to back in-stream): the fixed cost
 * of the per-step gather.  Returns 1 when the pipeline owns a communicator, else 0 (all three read 0 then).
 */
int nb_hip_comm_bringup(const SimPipeline *sim, double *init_ms, double *first_gather_ms, double *small_gather_us);

/*
 * Preflight probes for multi-GPU harnesses (bench.py, nbody-bench): asked BEFORE the first real contact between ranks, so
 * that a failed bring-up can say why.  Unlike the rest of this ABI they REPORT instead of aborting (they still abort when
 * this process has no gfx950 device at all).
 *   nb_hip_preflight_peers       row[q] = hipDeviceCanAccessPeer(this process' device, q): 1 / 0, 1 for the device itself,
 *                                -1 when the query failed, -2 for q >= the visible device count (returned)
 *   nb_hip_preflight_ipc_export  allocates one 4 KiB device word holding `tag` and writes its hipIpcMemHandle_t (64 bytes)
 *                                to handle64; returns the hipError_t (0 = ok)
 *   nb_hip_preflight_ipc_open    maps a PEER's exported handle (hipIpcOpenMemHandle, lazy peer access), reads the word,
 *                                unmaps; returns 0 when the word is expect_tag, the hipError_t of the failing call, or -1
 *                                when the word read is not the peer's; *ms = host milliseconds of open + read + close
 *   nb_hip_preflight_ipc_release frees the exported word (call after every peer has finished its open)
 *   nb_hip_error_string          text of a code returned by the two calls above
 */
int nb_hip_preflight_peers(int *row, int len);
int nb_hip_preflight_ipc_export(void *handle64, uint32_t tag);
int nb_hip_preflight_ipc_open(const void *handle64, uint32_t expect_tag, double *ms);
void nb_hip_preflight_ipc_release(void);
const char *nb_hip_error_string(int hip_error);

/* Cached hipGraph chains of this pipeline (at most 8, least recently used evicted); *dt_uploads = times a new step
 * size was written to device memory (the kernels read dt from there, like the reference's uniform block,
 * sim_gpu.c:268-284, so a changed dt never rebuilds or patches a cached chain). */
uint32_t nb_hip_graph_stats(const SimPipeline *sim, uint32_t *dt_uploads);

/* hipRuntimeGetVersion() of the HIP runtime this process actually bound (0 when it cannot be asked). */
int nb_hip_runtime_version(void);

/*
 * Measurement aid (no reference counterpart): the shader clock the chip holds under the step kernels' instruction mix.
 * Runs a separate probe kernel -- the interaction statement of the step kernels on scalar source operands, two
 * receivers per lane, 1024-thread workgroups filling every SIMD with 8 waves, no memory traffic in the loop -- for about
 * target_ms milliseconds; every wave stamps s_memtime (shader cycles) and s_memrealtime (constant reference clock) around
 * its loop.  *clock_ghz = d(memtime) / d(memrealtime) x the reference rate, median over the waves that spanned the whole
 * loop (a SIMD favours its oldest wave: the others finish early; min / max over all waves beside it);
 * *cycles_per_wave_interaction = the longest wave's shader cycles / 8 waves per SIMD / interactions one wave issued
 * (26 = the floor of this instruction mix: 9 plain fp32 VALU at 2 cycles + one v_rsq_f32 at 8).  The product kernels carry
 * no stamps.  Any out pointer may be NULL.  Returns the number of waves that reported.
 */
int nb_hip_probe_clock(double target_ms, double *clock_ghz, double *clock_ghz_min, double *clock_ghz_max,
                       double *cycles_per_wave_interaction, double *elapsed_ms);

/*
 * Measurement aid: the shader clock WHILE other work runs.  begin launches 8 one-wave workgroups (one per XCD) on their
 * own stream that stamp s_memtime / s_memrealtime every period_ms and sleep in between -- 8 of the chip's 8192 wave slots,
 * a few scalar instructions per period -- until end is called or max_ms has passed (every wave leaves by itself then).
 * end stops them and reports, over all sampled intervals: median / min / max clock in GHz, the median per XCD
 * (per_xcd_ghz8[8], 0 where no wave sat), the mean clock of each tenth of the sampled span as one wave saw it (profile10[10]) and
 * the span in milliseconds.  Intervals in which a counter did not move forward by a sane amount are dropped and counted
 * (*dropped_intervals).  Returns the number of intervals kept.  Any out pointer may be NULL.  One sampler per process.
 * bench.py brackets a repeat of the headline leg with it (roofline.held_clock_ghz): the probe above loads the chip with a
 * denser loop than the step kernel's and therefore reads a lower clock than the step kernel holds.
 */
#define NB_CLOCK_SAMPLER_MAX_MS 20000.0 /* period_ms below 0.05 and max_ms above this are clamped, never refused */
int nb_hip_clock_sampler_begin(double period_ms, double max_ms);
int nb_hip_clock_sampler_end(double *clock_ghz, double *clock_ghz_min, double *clock_ghz_max, double *per_xcd_ghz8,
                             double *profile10, double *span_ms, uint32_t *dropped_intervals);

/*
 * Optional: tell the pipeline which long-lived host array Set/GetSimulationData will be called with (the World's
 * particle array).  It is page-locked (hipHostRegister) when the pipeline first touches the GPU and released in
 * DestroySimPipeline, so the hand-over runs at PCIe speed instead of through pageable memory.  The array must stay
 * allocated until DestroySimPipeline or until this is called again (array = NULL forgets it).  Set/Get with any
 * other pointer keep working unchanged.  In a frame loop (every blocking update followed by a Get into this array,
 * reference src/main.c:157-163,237) the pipeline appends the read-back to the update's own submission.
 */
void nb_hip_note_host_array(SimPipeline *sim, void *array, uint64_t bytes);

/*
 * Run-time knobs a user of the reference harness needs.  key is one of:
 *   "variant"   how the wave-uniform sources reach the VALU: 1 (default) = through the scalar cache as SGPR operands,
 *               0 = wave-private LDS tiles (north star's design; bit-identical results, 8 % slower at N = 2^20: every
 *               bench.py line times both, roofline.alt_lds)
 *   "graph"     how PerformSimUpdate(n > 1) runs its chain: 0 = plain stream launches; 1 = always as a hipGraph, built on
 *               first use and cached per (length, ping-pong phase); 2 (default) = auto: calls shorter than 16 steps are
 *               plain launches; longer calls on small worlds (N x M <= 6e7) replay ONE canonical 32-step chain built when
 *               the data first reaches the device; on larger worlds a chain length runs as plain launches the first time
 *               it is asked for and as a cached hipGraph from the second time on.  The step size is never baked into a
 *               chain: kernels read it from device memory
 *   "timing"    1 = bracket every chain with a HIP event pair so that nb_hip_last_step_ms can answer, 0 (default) =
 *               do not (the two records cost a frame loop 3-7 us per call)
 *   "overlap"   sharded pipelines: 1 = split each step into own-shard / remote-shard kernels with the all-gather in
 *               between on a second stream, 0 = gather then one kernel (default)
 *   "sharded_graph"  sharded pipelines: 1 = capture the {kernel, all-gather} x n chain into a hipGraph and replay it
 *               (non-overlapped step only); 0 = plain stream launches (default)
 *               Both are opt-in by policy: per rank a step is O(N*M/P) of kernel against an O(M)
 *               gather, and every harness times all three modes from one command.
 * The same five can be preset from the environment: NB_HIP_VARIANT, NB_HIP_GRAPH, NB_HIP_OVERLAP, NB_HIP_SHARDED_GRAPH
 * (+ NB_HIP_FORCE_SHARDED = keep the RCCL path for a single rank, NB_HIP_COMM_TIMEOUT_S = bound of every wait on other
 * ranks).  Launch-shape and experiment knobs (receivers per lane, waves per workgroup, source split / passes / granule,
 * lane-split and one-workgroup chains, the fused finish, the frame loop's eager read-back) are NOT part of this ABI: every
 * one is on "auto", auto is what every published number was measured with, and the knobs that lost every measurement
 * live on only as test and tooling hooks (nbody_amd/csrc/nbody_hip_tuning.h: nb_hip_tune; their environment variables
 * exist in TUNING=1 builds only).
 * Returns the previous value; aborts on an unknown key or value.
 */
int nb_hip_configure(SimPipeline *sim, const char *key, int value);

/* What the last step launch actually used (everything is on auto unless a tuning hook moved it): k, w, variant, split, workgroups. */
void nb_hip_launch_shape(const SimPipeline *sim, int *k, int *w, int *variant, int *split, uint32_t *workgroups);

/*
 * The launch-shape arithmetic behind "auto", pure host code (usable without a GPU): for n_recv receivers and
 * n_src sources on a chip with compute_units CUs it returns receivers per lane, waves per workgroup, source
 * split and the resulting workgroup count.  Workgroups of one launch all take the same time, so the model
 * minimises rounds * work-per-workgroup, rounds = ceil(workgroups / resident slots).
 */
void nb_hip_plan_launch(uint32_t n_recv, uint32_t n_src, int compute_units, int *k, int *w, int *split, uint32_t *workgroups);

/* -- sharded (multi-GPU) pipeline: one process per GPU, N/P receivers each -- */

#define NB_HIP_UNIQUE_ID_BYTES 128

/* Rank 0 calls this and ships the 128 bytes to every rank (any transport). Wraps ncclGetUniqueId. */
void nb_hip_comm_unique_id(void *out128);

/*
 * Collective over all ranks.  Each rank passes the same WorldData and later the
 * same full particle array; rank r owns the r-th 1/P slice of the massive range
 * and the r-th 1/P slice of the massless range (nb_hip_shard_plan).
 * SetSimulationData / PerformSimUpdate / GetSimulationData keep their meaning and
 * become collectives: Get returns the FULL array on every rank.
 */
SimPipeline *CreateSimPipelineSharded(WorldData data, int rank, int nranks, const void *unique_id128);

/*
 * The same sharded pipeline over a caller-supplied transport instead of RCCL (MPI, gloo, shared memory ...): an
 * in-place all-gather over HOST memory.  buf holds nranks slots of bytes_per_rank bytes; on entry slot `rank` is
 * filled, on return every slot must hold what the owning rank put there.  The callback runs on the caller's thread,
 * inside PerformSimUpdate / GetSimulationData, once per step (source positions, Mc float2 per rank) and once per Get
 * (particle slices); every rank must reach it the same number of times.  The pipeline stages through one page-locked
 * buffer (D2H own slot, wait, callback, H2D all slots), so this route costs a host round trip per step: it exists for
 * machines without RCCL and for exercising the multi-process path with several ranks on ONE GPU (RCCL refuses two
 * ranks on a device).  Everything else -- shard plan, kernels, mirror / gather layout, overlap mode -- is the RCCL
 * path's; "sharded_graph" is ignored (a host callback cannot run inside a captured graph).
 */
/* NbAllGatherFn: include/nbody.h -- void (*)(void *ctx, void *buf, uint64_t bytes_per_rank, int rank, int nranks) */
SimPipeline *CreateSimPipelineShardedWith(WorldData data, int rank, int nranks, NbAllGatherFn allgather, void *ctx);

/*
 * The same sharded pipeline with the DIRECT exchange: no RCCL, no host staging of the data.  Every rank maps every
 * peer's gathered source array (hipIpcGetMemHandle / hipIpcOpenMemHandle, exchanged once through `control`) and, after
 * each step, copies its own slice device-to-device straight into all of them -- on xGMI, which is point-to-point, each of
 * the P - 1 copies rides its own link: the direct all-gather, where a ring would serialise P - 1 hops per link -- then
 * synchronises its stream and meets the other ranks in ONE host-side barrier per step (an 8-byte all-gather of step
 * counters through `control`; every rank must be at the same step or the call aborts).  `control` is the same in-place
 * host all-gather callback as above; it carries the IPC handles at the first SetSimulationData, a barrier at the end of
 * every SetSimulationData (no peer may push into arrays their owner is still initialising), the per-step barrier, the
 * particle slices of a collective GetSimulationData, and one barrier in DestroySimPipeline (which is therefore a
 * collective for these pipelines: nobody unmaps or frees while a peer may still write).  Costs a host round trip per
 * step like the host transport (no hipGraph capture, no overlap gain) but moves no particle data through the host:
 * a fallback for machines without a working RCCL and a way to run P processes on ONE device at device speed.
 */
SimPipeline *CreateSimPipelineShardedDirect(WorldData data, int rank, int nranks, NbAllGatherFn control, void *ctx);

/* The shard arithmetic, pure host code (usable without a GPU). */
typedef struct NbShardPlan {
    uint32_t mass_chunk;   /* Mc: massive slots per rank = all-gather count (uniform)   */
    uint32_t zero_chunk;   /* Zc: massless slots allocated per rank (uniform, >= any)   */
    uint32_t mass_begin;   /* first global massive index owned: rank * Mc, clamped      */
    uint32_t mass_count;   /* owned massive particles (<= Mc)                           */
    uint32_t zero_begin;   /* first global massless index owned (>= mass_len), clamped  */
    uint32_t zero_count;   /* owned massless particles (<= Zc), dealt to level the      */
                           /* per-rank totals mass_count + zero_count                   */
    uint32_t src_padded;   /* nranks * Mc: length of the gathered source array          */
} NbShardPlan;

NbShardPlan nb_hip_shard_plan(uint32_t total_len, uint32_t mass_len, int rank, int nranks);

/*
 * Local transport (testing aid): all nranks shards live in THIS process on the current device and
 * exchange sources by device copies instead of RCCL.  Same shard plan, same kernels, same mirror /
 * gather layout as the RCCL path, so a single-GPU box can verify the sharded arithmetic end to end.
 * out[] receives nranks pipelines; feed each the same full array with SetSimulationData, advance them
 * together with nb_hip_local_group_step (PerformSimUpdate on a member aborts), read any member with
 * GetSimulationData, destroy every member with DestroySimPipeline.
 */
int nb_hip_local_group_create(WorldData data, int nranks, SimPipeline **out);
void nb_hip_local_group_step(SimPipeline **sims, int nranks, uint32_t n, float dt);

/*
 * Conservation diagnostics of the state the pipeline holds (definitions: include/nbody_diag.h).
 *   nb_hip_energy     fills *out: the potential over the M massive receivers, kinetic energy, mass, momentum, angular
 *                     momentum and centre of mass, all reduced in a fixed order in float64 (bitwise reproducible)
 *   nb_hip_potential  writes total_len floats: Phi_i of every particle, massless ones included, in partitioned order
 * Both are enqueued on the pipeline's stream behind any nb_hip_step_async work and read the buffer that holds the latest
 * state (the one GetSimulationData merges from); they block until their own result is on the host.  They change nothing
 * observable: the state, the ping-pong phase, the cached chains (nb_hip_graph_stats), the step-size uploads, what
 * nb_hip_last_step_ms reports and the frame loop's eager read-back are as before the call.  Abort before the first
 * SetSimulationData and for sharded pipelines (their remote slices are current only inside a step: a sharded energy
 * needs a collective, not supported).
 */
void nb_hip_energy(SimPipeline *sim, WorldEnergy *out);
void nb_hip_potential(SimPipeline *sim, float *phi);

/*
 * Rendering the state the pipeline holds (definitions: include/nbody_render.h; all three results are bitwise functions of
 * the state and the view):
 *   nb_hip_bounds         bounds[4] = {min.x, min.y, max.x, max.y} over the particles with finite x and y
 *   nb_hip_render_counts  counts[3][height][width] uint32: particles of each class covering each pixel
 *   nb_hip_render_rgba    rgba[height][width][4] uint8: the count image shaded with *palette (not NULL)
 * Like the diagnostics above they are enqueued on the pipeline's stream behind any nb_hip_step_async work, read the buffer
 * that holds the latest state, block until their own result is in the caller's host buffer, and change nothing observable:
 * the state, the ping-pong phase, the cached chains (nb_hip_graph_stats), the step-size uploads, what nb_hip_last_step_ms
 * reports and the frame loop's eager read-back are as before the call.  The count image, the disc list and the frame live
 * in device buffers of the pipeline that grow on demand and are freed by DestroySimPipeline.  Abort before the first
 * SetSimulationData, for an invalid view or palette, and for sharded pipelines (a sharded render needs a collective over
 * the ranks: not supported).  Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_render_rgba").
 */
void nb_hip_bounds(SimPipeline *sim, float *bounds);
void nb_hip_render_counts(SimPipeline *sim, const RenderView *view, uint32_t *counts);
void nb_hip_render_rgba(SimPipeline *sim, const RenderView *view, const RenderPalette *palette, uint8_t *rgba);

/*
 * The potential of the state the pipeline holds away from its particles (definitions: include/nbody_field.h):
 *   nb_hip_potential_at   phi[i] = Phi(points[i]; softening) for the caller's n points ((x, y) pairs), 0 <= n <= 2^24;
 *                         n = 0 does nothing
 *   nb_hip_potential_map  phi[height][width] float32: Phi at every pixel centre of *view (only target, offset, zoom, width
 *                         and height are used).  The host computes the width column and height row coordinates; only those
 *                         width + height floats travel to the device, and the map is exactly nb_hip_potential_at of the
 *                         grid points, row-major
 * Phi at a point has the bits nb_hip_potential gives a massless particle of radius `softening` at the same place: the
 * same pair statement and the same summation order.  A point with a non-finite coordinate gives NaN.  Like the
 * diagnostics above they are enqueued on the pipeline's stream behind any nb_hip_step_async work, read the buffer that
 * holds the latest state, block until their own result is in the caller's host buffer, and change nothing observable: the
 * state, the ping-pong phase, the cached chains, the step-size uploads, what nb_hip_last_step_ms reports and the frame
 * loop's eager read-back are as before the call.  Their device buffers grow on demand and are freed by
 * DestroySimPipeline.  Abort before the first SetSimulationData, for a softening that is not finite and > 0, for an invalid
 * view, and for sharded pipelines (a collective over the ranks: not supported).  Added WITHOUT a version bump: detect them
 * by symbol (dlsym "nb_hip_potential_map").
 */
void nb_hip_potential_at(SimPipeline *sim, const float *points, uint32_t n, float softening, float *phi);
void nb_hip_potential_map(SimPipeline *sim, const RenderView *view, float softening, float *phi);

/*
 * The acceleration field of the state the pipeline holds away from its particles (definitions: include/nbody_gravity.h):
 *   nb_hip_acceleration_at   acc[2 * i], acc[2 * i + 1] = g(points[i]; softening) for the caller's n points ((x, y) pairs),
 *                            0 <= n <= 2^24; n = 0 does nothing
 *   nb_hip_acceleration_map  acc[height][width][2] float32: g at every pixel centre of *view (only target, offset, zoom,
 *                            width and height are used).  The host computes the width column and height row coordinates;
 *                            only those width + height floats travel to the device, and the map is exactly
 *                            nb_hip_acceleration_at of the grid points, row-major
 * The pair is the step kernels' statement with the softening in the place of the receiver's radius; the sums are those of
 * nb_hip_potential (fp32 over a block of 256 sources, float64 block totals in eight source slices added in order), so a
 * result is a function of the point and the state alone: not of n, the point's index or the kernel shape.  A point with a
 * non-finite coordinate gives NaN in both components.  Like the diagnostics above they are enqueued on the pipeline's stream
 * behind any nb_hip_step_async work, read the buffer that holds the latest state, block until their own result is in the
 * caller's host buffer, and change nothing observable: the state, the ping-pong phase, the cached chains, the step-size
 * uploads, what nb_hip_last_step_ms reports and the frame loop's eager read-back are as before the call.  Their device
 * buffers grow on demand and are freed by DestroySimPipeline.  Abort before the first SetSimulationData, for a softening
 * that is not finite and > 0, for an invalid view, and for sharded pipelines (a collective over the ranks: not supported).
 * Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_acceleration_map").
 */
void nb_hip_acceleration_at(SimPipeline *sim, const float *points, uint32_t n, float softening, float *acc);
void nb_hip_acceleration_map(SimPipeline *sim, const RenderView *view, float softening, float *acc);

/*
 * The tidal tensor T = dg/dp of the state the pipeline holds away from its particles (definitions: include/nbody_tidal.h;
 * kernels: nbody_amd/csrc/tidal.hip), three float32 per sample in the order (xx, xy, yy):
 *   nb_hip_tidal_at   t[3 * i .. 3 * i + 2] = T(points[i]; softening) for the caller's n points ((x, y) pairs),
 *                     0 <= n <= 2^24; n = 0 does nothing
 *   nb_hip_tidal_map  t[height][width][3]: T at every pixel centre of *view, exactly nb_hip_tidal_at of the grid points,
 *                     row-major; only the width column and height row coordinates travel to the device
 * The field sampler's third pair statement: one v_rsq_f32 per pair, four running fp32 sums per sample in the sums of
 * nb_hip_potential_at (blocks of 256 sources, float64 block totals in eight source slices added in order); the factor 3 and
 * the difference of the two parts of a diagonal component are taken in float64 and each component is rounded once.  A
 * result is a function of the point and the state alone: not of n, the point's index or the kernel shape.  No term is
 * excluded: a point on a source gets that source's finite term diag(-G*m s^(-3/2)).  A point with a non-finite coordinate
 * gives NaN in all three components; mass_len = 0 gives three +0.  Enqueued, blocking and invisible to the steps exactly as
 * nb_hip_acceleration_at / _map above, with the same buffers and the same aborts.
 * Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_tidal_map").
 */
void nb_hip_tidal_at(SimPipeline *sim, const float *points, uint32_t n, float softening, float *t);
void nb_hip_tidal_map(SimPipeline *sim, const RenderView *view, float softening, float *t);

/*
 * World ensembles: `count` independent worlds with the same particle count, stepped together.
 *
 * One world of a few hundred to a few thousand particles keeps one or a handful of the chip's 256 compute units busy;
 * a SimBatch steps many of them per launch (seeds of one galaxy set-up, a sweep over dt, training data).  Members never
 * interact.  Member b has its own source count mass_len[b] and may have its own step size.  Particles travel member-major:
 * count * total_len records, member b at [b * total_len, (b + 1) * total_len), each member partitioned "mass > 0 first".
 *
 * The contract: after any sequence of calls member b's particles are BIT-IDENTICAL to the same particles stepped alone
 * in a SimPipeline(total_len, mass_len[b]) by the same calls with its launch shape pinned to the ensemble's (below).  A
 * member's bits therefore do not depend on count, on its index, on the other members, or on how the steps are cut into
 * calls.  The launch path is a function of total_len alone:
 *   total_len <= 512          one workgroup per member runs the whole call (one launch per call of up to 65 536 steps)
 *   512 < total_len <= 3 000  one lane-split launch per step for the whole ensemble
 * Larger worlds fill the chip on their own: use one SimPipeline each.
 *
 * Same conventions as the rest of this header: create allocates nothing on the GPU (device work starts at the first
 * nb_hip_batch_set_data), failures print "file:line [func] ..." and abort() -- count = 0 or > NB_HIP_BATCH_MAX_COUNT,
 * total_len = 0 or > NB_HIP_BATCH_MAX_LEN, a mass_len[b] > total_len, an update or read-back before set_data -- there is
 * no CPU fallback, and the caller's rand() stream is left alone.  mass_len[b] = 0 (a member without sources) and n = 0
 * (no-op) are legal.  Step sizes live in device memory and are uploaded only when a value changes; a per-member upload
 * first waits for the steps already queued (they keep their step sizes).  A SimBatch shares no state with any SimPipeline.
 * These calls were added WITHOUT a version bump (nb_hip_version() stays 400): detect them by symbol
 * (dlsym "nb_hip_batch_create").
 */
#define NB_HIP_BATCH_MAX_COUNT 65535u
#define NB_HIP_BATCH_MAX_LEN 3000u

typedef struct SimBatch SimBatch;

SimBatch *nb_hip_batch_create(uint32_t count, uint32_t total_len, const uint32_t *mass_len /* [count] */);
void nb_hip_batch_destroy(SimBatch *batch); /* NULL is accepted */
void nb_hip_batch_set_data(SimBatch *batch, const Particle *ps);
void nb_hip_batch_get_data(const SimBatch *batch, Particle *ps);
void nb_hip_batch_get_member(const SimBatch *batch, uint32_t member, Particle *ps); /* total_len records */
void nb_hip_batch_update(SimBatch *batch, uint32_t n, float dt);            /* blocking, one dt for every member */
void nb_hip_batch_update_dts(SimBatch *batch, uint32_t n, const float *dt); /* blocking, dt[count] */
void nb_hip_batch_step_async(SimBatch *batch, uint32_t n, const float *dt); /* enqueue only, dt[count] */
void nb_hip_batch_sync(SimBatch *batch);
/* device milliseconds of the kernels of the last update (an event pair of the ensemble's own; 0 before the first) */
double nb_hip_batch_last_ms(SimBatch *batch);
/* how often step sizes were written to device memory */
uint32_t nb_hip_batch_dt_uploads(const SimBatch *batch);
/*
 * The launch shape, fixed at creation: path 0 = one-workgroup chain (k = 2, w = 16 / tiles waves per receiver tile,
 * lanes = 1: the per-step shape k, w, split = 1, unit = 8 it is bit-equal to), path 1 = lane-split (k = 1, w waves per
 * workgroup, `lanes` lane groups per wave); workgroups per launch.  Any pointer may be NULL.
 */
void nb_hip_batch_launch_shape(const SimBatch *batch, int *path, int *k, int *w, int *lanes, uint32_t *workgroups);

/*
 * Conservation diagnostics of every member of an ensemble, in one pass over all members (definitions:
 * include/nbody_diag.h; M_b = mass_len[b]):
 *   nb_hip_ensemble_energy     fills out[count]: member b's WorldEnergy
 *   nb_hip_ensemble_potential  writes count * total_len floats, member-major: Phi_i of every particle of every member
 * Member b's result is BIT-IDENTICAL to nb_hip_energy / nb_hip_potential of a SimPipeline holding the same particles: it
 * does not depend on count, on the member's index or on the other members (the sums run in a fixed order that both kernels
 * share).  A member with M_b = 0 gives all-zero sums and Phi = 0; M_b = 1 gives Phi_0 = 0.
 * Like nb_hip_energy for a pipeline: both are enqueued on the ensemble's stream behind any nb_hip_batch_step_async work,
 * read the buffer that holds the latest state, block until their result is on the host, and change nothing observable --
 * the state, the ping-pong phase, the step sizes on the device, nb_hip_batch_dt_uploads and nb_hip_batch_last_ms are as
 * before the call.  The particles are not read back: energy is two launches and one copy of 64 * count bytes, potential
 * one launch and one copy of 4 * count * total_len bytes, for any count.  Their scratch belongs to the SimBatch, is made
 * on first use and freed by nb_hip_batch_destroy.  Abort before nb_hip_batch_set_data.  Added WITHOUT a version bump:
 * detect them by symbol (dlsym "nb_hip_ensemble_energy").
 */
void nb_hip_ensemble_energy(SimBatch *batch, WorldEnergy *out /* [count] */);
void nb_hip_ensemble_potential(SimBatch *batch, float *phi /* [count * total_len], member-major */);

/*
 * Traced updates: the n steps of nb_hip_batch_update(_dts) with every member's WorldEnergy recorded every `every` steps,
 * in one call (what a sweep over step sizes or seeds compares is the drift of the energy over time).
 *   nb_hip_ensemble_trace_rows  host arithmetic: R = 1 + n / every, the records such a call makes
 *   nb_hip_ensemble_trace       one dt for every member
 *   nb_hip_ensemble_trace_dts   dt[count]
 * out is WorldEnergy[R][count], record-major: row 0 is the state on entry, row r the state after r * every steps; the
 * trailing n mod every steps run and are not recorded; n = 0 gives row 0 alone and changes nothing.  Exactly the n steps
 * of an untraced update run: the particles, the ping-pong phase, the step sizes on the device and nb_hip_batch_dt_uploads
 * afterwards are bit for bit what nb_hip_batch_update(_dts)(n) leaves, and nb_hip_batch_last_ms brackets the whole call.
 * Row r of member b is BIT-IDENTICAL to what nb_hip_ensemble_energy returns after the same steps made by separate update
 * calls (and so to nb_hip_energy of the same world alone).  Nothing returns to the host between records: the rows collect
 * in a device buffer of the SimBatch (made on first use, freed by nb_hip_batch_destroy) and one copy of R * count * 64
 * bytes and one stream sync end the call.  total_len <= 512: the one launch that runs the call records from the state it
 * holds (still one launch per 65 536 steps, whatever R is); above: the two launches of nb_hip_ensemble_energy are
 * enqueued behind every `every`-th step launch.  Both calls block and queue behind earlier nb_hip_batch_step_async work.
 * Abort for every = 0, a NULL argument, more than 2^24 rows (R * count; 1 GiB) and before nb_hip_batch_set_data.  Added
 * WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_ensemble_trace").
 */
uint32_t nb_hip_ensemble_trace_rows(uint32_t n, uint32_t every);
void nb_hip_ensemble_trace(SimBatch *batch, uint32_t n, float dt, uint32_t every, WorldEnergy *out /* [R][count] */);
void nb_hip_ensemble_trace_dts(SimBatch *batch, uint32_t n, const float *dt /* [count] */, uint32_t every, WorldEnergy *out);

/*
 * Rendering an ensemble: bounds, per-class count images and RGBA frames of EVERY member, without reading a particle back
 * (definitions: include/nbody_render.h; the World-level calls are include/nbody_batch_render.h).
 *   nb_hip_ensemble_bounds         bounds[count][4]: member b's {min.x, min.y, max.x, max.y}
 *   nb_hip_ensemble_render_counts  counts[count][3][height][width] under views[count], one view per member
 *   nb_hip_ensemble_render_rgba    rgba[count][height][width][4]
 * Member b's result is BIT-IDENTICAL to nb_hip_bounds / nb_hip_render_counts / nb_hip_render_rgba of a SimPipeline holding
 * the same particles under views[b]: it does not depend on count, on the member's index or on the other members.  All
 * views share width and height (a mismatch aborts, naming the first member that differs), each is within the limits of
 * include/nbody_render.h, count * width * height <= 2^24 and saturation >= 1.  While the three class planes of one image
 * fit a workgroup's share of the LDS (3 * width * height * 4 <= 48 KiB, a 64 x 64 thumbnail) one workgroup per member
 * builds the member's image on chip: ONE launch per call, for counts and for frames; larger images take a clear, a splat,
 * a disc pass and (frames) a shade over all members -- in both cases a constant number of launches, one upload of the
 * views, one copy of the images and one stream sync for any count.  The choice depends on width * height alone.  Like
 * the diagnostics: enqueued on the ensemble's stream behind any nb_hip_batch_step_async work, they read the buffer that
 * holds the latest state, block until the result is on the host and change nothing observable (the state, the ping-pong
 * phase, the step sizes, nb_hip_batch_dt_uploads and nb_hip_batch_last_ms are as before; the render has an event pair of
 * its own).  Scratch belongs to the SimBatch, is made on first use, regrown when a call needs more, and freed by
 * nb_hip_batch_destroy.  Abort before nb_hip_batch_set_data and for a NULL argument.  Added WITHOUT a version bump:
 * detect them by symbol (dlsym "nb_hip_ensemble_render_rgba").
 */
void nb_hip_ensemble_bounds(SimBatch *batch, float *bounds /* [count][4] */);
void nb_hip_ensemble_render_counts(SimBatch *batch, const RenderView *views /* [count] */, uint32_t *counts /* [count][3][h][w] */);
void nb_hip_ensemble_render_rgba(SimBatch *batch, const RenderView *views /* [count] */, const RenderPalette *palette,
                                 uint8_t *rgba /* [count][h][w][4] */);

/*
 * Ragged ensembles: members of DIFFERENT particle counts in one SimBatch (a sweep over resolution, MakeGalaxies worlds of
 * unequal size), stepped by the same launches instead of one SimBatch per size.
 *   nb_hip_ragged_create        member b has total_len[b] particles (1 .. NB_HIP_BATCH_MAX_LEN), mass_len[b] of them sources
 *   nb_hip_ragged_layout        sizes[count] and offsets[count + 1]: offsets[b] = total_len[0] + ... + total_len[b - 1]
 *   nb_hip_ragged_launch_shape  the launch groups: returns how many there are and describes group `group`
 *   nb_hip_ragged_member_shape  the group and the (k, w, lanes) of one member
 * The result is a SimBatch: every nb_hip_batch_* call, nb_hip_ensemble_energy / _potential and nb_hip_ensemble_trace(_dts)
 * work on it as documented above, with ONE change of layout: every particle array that crosses this seam (set_data,
 * get_data) and every per-particle result (potential) is PACKED, member b at offsets[b]; get_member returns total_len[b]
 * records.  A uniform ensemble is the special case in which that is today's layout, and nb_hip_ragged_layout /
 * _launch_shape / _member_shape also answer for a SimBatch made by nb_hip_batch_create (one group).
 *
 * The contract: member b is BIT-IDENTICAL -- particles after any number of steps and any cutting of the calls, energy,
 * potential, every row of a traced call -- to the same particles as the single member of nb_hip_batch_create(1,
 * total_len[b], &mass_len[b]), whatever count, its index, its neighbours, their sizes, their step sizes or the groups
 * present are.  That holds because a member's launch shape is a function of its own size alone.  Members fall into up to
 * three launch groups, reported in this order, absent when empty:
 *   total_len <= 512           chain: one workgroup per member runs the whole call, w = 16, 8 or 4 by its own size
 *   513 <= total_len <= 1581   lane-split, w = 8, lanes = 8
 *   1582 <= total_len <= 3000  lane-split, w = 16, lanes = 4
 * A call is one chain launch plus, per step, one launch per lane-split group; workgroups past a smaller member's last
 * receiver leave at once.  nb_hip_ragged_launch_shape gives a group's path, k, w (chain: of its largest member), lanes,
 * member count and workgroups per launch; any pointer may be NULL.  A traced update records inside the chain launch when
 * every member is in the chain group and interleaves the two diagnostics launches otherwise (same bits).
 *
 * Not wired yet: nb_hip_ensemble_bounds / _render_counts / _render_rgba abort on a ragged ensemble with a message that
 * says so, before they touch the device.  Create allocates nothing on the GPU; count = 0 or > NB_HIP_BATCH_MAX_COUNT, a
 * total_len[b] of 0 or > NB_HIP_BATCH_MAX_LEN and a mass_len[b] > total_len[b] print "file:line [func] ... member b ..."
 * and abort().  Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_ragged_create").
 */
SimBatch *nb_hip_ragged_create(uint32_t count, const uint32_t *total_len /* [count] */, const uint32_t *mass_len /* [count] */);
void nb_hip_ragged_layout(const SimBatch *batch, uint32_t *sizes /* [count] */, uint64_t *offsets /* [count + 1] */);
uint32_t nb_hip_ragged_launch_shape(const SimBatch *batch, uint32_t group, int *path, int *k, int *w, int *lanes, uint32_t *members,
                                    uint32_t *workgroups);
void nb_hip_ragged_member_shape(const SimBatch *batch, uint32_t member, uint32_t *group, int *k, int *w, int *lanes);

/*
 * The potential and the acceleration field of EVERY member of an ensemble away from its particles, in one launch
 * (definitions: include/nbody_field.h and include/nbody_gravity.h with M = mass_len[b]; the World-level calls are
 * include/nbody_batch_field.h; kernel: nbody_amd/csrc/batch_field.hip).  Every member has the same number of samples:
 *   nb_hip_ensemble_potential_at      phi[count][n]: Phi(points[b][i]; softening) of member b, points[count][n] (x, y) pairs
 *   nb_hip_ensemble_potential_map     phi[count][height][width]: Phi at every pixel centre of views[b], one view per member
 *   nb_hip_ensemble_acceleration_at   acc[count][n][2]: g at the same kind of points
 *   nb_hip_ensemble_acceleration_map  acc[count][height][width][2]
 * Member b's values are BIT-IDENTICAL to nb_hip_potential_at / _map / nb_hip_acceleration_at / _map of a SimPipeline holding
 * the same particles, on either of that pipeline's kernel shapes: they do not depend on count, on the member's index, on the
 * other members or on their sizes.  Uniform and ragged ensembles alike (a ragged member's sources are its mass_len[b], the
 * samples are not packed: n per member).  One softening per call, finite and > 0.  A point with a non-finite coordinate
 * gives NaN in every component, a member with mass_len[b] = 0 gives 0, n = 0 does nothing and touches no device.  All views
 * share width and height (a mismatch aborts, naming the first member that differs) and each is within the limits of
 * include/nbody_render.h; the host computes every view's width column and height row coordinates, so a map is exactly the
 * probes product at the member's pixel centres, row-major.  count * n and count * width * height are each at most 2^24.
 * Each call is one upload, one launch, one copy and one stream sync for any count.  Like the diagnostics: enqueued on the
 * ensemble's stream behind any nb_hip_batch_step_async work, they read the buffer that holds the latest state, block until
 * the result is on the host and change nothing observable (the state, the ping-pong phase, the step sizes,
 * nb_hip_batch_dt_uploads and nb_hip_batch_last_ms are as before).  Scratch belongs to the SimBatch, grows on demand and is
 * freed by nb_hip_batch_destroy.  Abort before nb_hip_batch_set_data, for a NULL argument, a softening that is not finite
 * and > 0, an invalid view and too many samples.  Added WITHOUT a version bump: detect them by symbol
 * (dlsym "nb_hip_ensemble_potential_map").
 */
void nb_hip_ensemble_potential_at(SimBatch *batch, const float *points /* [count][n][2] */, uint32_t n, float softening,
                                  float *phi /* [count][n] */);
void nb_hip_ensemble_potential_map(SimBatch *batch, const RenderView *views /* [count] */, float softening, float *phi /* [count][h][w] */);
void nb_hip_ensemble_acceleration_at(SimBatch *batch, const float *points /* [count][n][2] */, uint32_t n, float softening,
                                     float *acc /* [count][n][2] */);
void nb_hip_ensemble_acceleration_map(SimBatch *batch, const RenderView *views /* [count] */, float softening,
                                      float *acc /* [count][h][w][2] */);

/*
 * The tidal tensor of EVERY member of an ensemble, in one launch (definitions: include/nbody_tidal.h with M = mass_len[b];
 * the World-level calls are include/nbody_batch_tidal.h; kernel: nbody_amd/csrc/tidal.hip):
 *   nb_hip_ensemble_tidal_at   t[count][n][3]: (xx, xy, yy) of T(points[b][i]; softening) of member b
 *   nb_hip_ensemble_tidal_map  t[count][height][width][3]: T at every pixel centre of views[b]
 * Everything said of the four calls above holds: member b's values are BIT-IDENTICAL to nb_hip_tidal_at / _map of a
 * SimPipeline holding the same particles on either of its kernel shapes, uniform and ragged ensembles alike, the same
 * limits, edge values (three NaN, three +0) and aborts, one upload, one launch, one copy and one sync for any count.
 * Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_ensemble_tidal_map").
 */
void nb_hip_ensemble_tidal_at(SimBatch *batch, const float *points /* [count][n][2] */, uint32_t n, float softening,
                              float *t /* [count][n][3] */);
void nb_hip_ensemble_tidal_map(SimBatch *batch, const RenderView *views /* [count] */, float softening, float *t /* [count][h][w][3] */);

/*
 * Radial profiles of the state a pipeline or an ensemble holds: the six float64 annulus moments (count, S, I, L, W, K) of
 * every row about a centre (definitions, row rule and summation order: include/nbody_profile.h; kernels:
 * nbody_amd/csrc/profile.hip).  edges: bins + 1 float32 radii, 1 <= bins <= 254; centre: (cx, cy, ux, uy); weights:
 * NB_PROFILE_BY_MASS = 0 (particles i < mass_len, weight m_i; a massless particle is never read) or NB_PROFILE_BY_NUMBER = 1
 * (all total_len particles, weight 1); out: [bins + 2][6] doubles; unplaced (nullable): the particles whose squared radius is NaN.
 *   nb_hip_profile            one workgroup per chunk of 1024 particles stores the chunk's rows to a slab the pipeline owns, one
 *                             thread per (row, column) then adds the chunks in order.  Upload bins + 1 + 4 floats, download
 *                             rows * 48 + 4 bytes, one sync.  Enqueued, blocking and invisible to the steps like nb_hip_energy;
 *                             sharded pipelines abort like it.  Nothing to read (total_len = 0, or mass mode with mass_len = 0)
 *                             gives +0 everywhere and touches no device.
 *   nb_hip_ensemble_profile   every member of an ensemble, uniform or ragged, in ONE launch: one workgroup per member walks its
 *                             three chunks or fewer.  The edges are shared, the centre is per member: centres[count][4].
 *                             out[count][bins + 2][6], unplaced[count].  Member b's values are BIT-IDENTICAL to nb_hip_profile
 *                             of a SimPipeline holding the same particles.
 * No float atomics: a result is a function of the state and the arguments alone.  Every check -- NULL arguments, bins of 0 or
 * above 254, non-finite, negative or non-increasing edges, a non-finite centre, an unknown weights, a call before the data is
 * set -- runs before any device touch and ends in "file:line [func] ..." + abort().
 * Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_profile", dlsym "nb_hip_ensemble_profile").
 */
void nb_hip_profile(SimPipeline *sim, const float *edges, uint32_t bins, const float centre[4], int weights, double *out,
                    uint32_t *unplaced);
void nb_hip_ensemble_profile(SimBatch *batch, const float *edges, uint32_t bins, const float *centres /* [count][4] */, int weights,
                             double *out /* [count][bins + 2][6] */, uint32_t *unplaced /* [count] */);

/*
 * Pair-separation counts of the state a pipeline or an ensemble holds: how many pairs of particles lie in every row of the
 * caller's radii, per class of pair (definitions, row rule and columns: include/nbody_paircount.h; kernel:
 * nbody_amd/csrc/paircount.hip).  edges: bins + 1 float32 radii, 1 <= bins <= 254; classes: a non-empty mask of NB_PAIRS_MM = 1,
 * NB_PAIRS_MT = 2, NB_PAIRS_TT = 4 (a class not asked for is zeros, and a particle only it would read is never read); out:
 * [bins + 2][3] uint64, every count exact; unplaced (nullable): [3], the pairs whose q is NaN.
 *   nb_hip_pair_counts            one launch: a workgroup per (class, tile of 128 receivers, span of sources) counts in LDS and
 *                                 adds its rows to a table the pipeline owns with 64-bit integer atomics.  No upload (the
 *                                 thresholds travel with the launch), download (rows + 1) * 24 bytes, one sync.  Enqueued,
 *                                 blocking and invisible to the steps like nb_hip_profile; sharded pipelines abort like it.
 *                                 Nothing to count (N < 2, or every requested class without a pair) gives zeros and touches no
 *                                 device.
 *   nb_hip_ensemble_pair_counts   every member of an ensemble, uniform or ragged, in ONE launch of the same kernel; one edge set
 *                                 and one mask for all.  out[count][bins + 2][3], unplaced[count][3].  Member b's counts are
 *                                 those of nb_hip_pair_counts of a SimPipeline holding the same particles.
 * Integers add exactly in any order: a result is a function of the state and the arguments alone, and there is no float
 * atomic.  Every check -- NULL arguments, bins of 0 or above 254, non-finite, negative or non-increasing edges, an empty or
 * unknown classes, a call before the data is set -- runs before any device touch and ends in "file:line [func] ..." + abort().
 * Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_pair_counts", dlsym "nb_hip_ensemble_pair_counts").
 */
void nb_hip_pair_counts(SimPipeline *sim, const float *edges, uint32_t bins, uint32_t classes, uint64_t *out /* [bins + 2][3] */,
                        uint64_t *unplaced /* [3] */);
void nb_hip_ensemble_pair_counts(SimBatch *batch, const float *edges, uint32_t bins, uint32_t classes,
                                 uint64_t *out /* [count][bins + 2][3] */, uint64_t *unplaced /* [count][3] */);

/*
 * The nearest neighbour and the neighbour count of every particle of the state a pipeline or an ensemble holds: which other
 * particle is closest, its squared distance, and how many lie within a radius (definitions, candidates, ties and the order-free
 * key: include/nbody_neighbour.h; kernel: nbody_amd/csrc/neighbour.hip).  receivers, sources: each a non-empty mask of
 * NB_NEIGH_MASSIVE = 1, NB_NEIGH_MASSLESS = 2 (a class that is neither is never read; a particle that is no receiver gets
 * (+inf, NB_NEIGH_NONE, 0)); radius: finite and >= 0, read only when count is given; q, index: [total_len]; count (nullable):
 * [total_len], and without it no count is evaluated.
 *   nb_hip_neighbours             one launch: a workgroup per (tile of 128 receivers, span of sources) merges in LDS and meets the
 *                                 other spans in a table of the call's scratch through one 64-bit integer atomic minimum and one
 *                                 32-bit integer atomic add per receiver.  No upload, download 8 bytes per particle without the
 *                                 count and 12 with it, one sync.  Enqueued, blocking and invisible to the steps like
 *                                 nb_hip_pair_counts; sharded pipelines abort like it.  Nothing to evaluate (no receiver or no
 *                                 source) fills the defaults and touches no device.
 *   nb_hip_ensemble_neighbours    every member of an ensemble, uniform or ragged, in ONE launch of the same kernel; one pair of
 *                                 masks and one radius for all.  The arrays are packed, member b at offsets[b] of
 *                                 nb_hip_ragged_layout; an index counts within its member.  Member b's entries are those of
 *                                 nb_hip_neighbours of a SimPipeline holding the same particles.
 * A minimum of keys and a sum of integers do not depend on order: a result is a function of the state and the arguments alone,
 * and there is no float atomic.  Every check -- NULL arguments, an empty or unknown mask, a non-finite or negative radius when
 * count is given, a call before the data is set -- runs before any device touch and ends in "file:line [func] ..." + abort().
 * Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_neighbours", dlsym "nb_hip_ensemble_neighbours").
 */
void nb_hip_neighbours(SimPipeline *sim, uint32_t receivers, uint32_t sources, float radius, float *q /* [total_len] */,
                       uint32_t *index /* [total_len] */, uint32_t *count /* nullable */);
void nb_hip_ensemble_neighbours(SimBatch *batch, uint32_t receivers, uint32_t sources, float radius, float *q, uint32_t *index,
                                uint32_t *count /* packed, member b at offsets[b] */);

/*
 * The friends-of-friends groups of the state a pipeline or an ensemble holds: every particle labelled with the smallest index of
 * the structure it is connected to under a linking length (definitions, what links and what follows: include/nbody_group.h; the
 * union-find and the argument for it: nbody_amd/csrc/group_common.h; kernels: nbody_amd/csrc/group.hip).  members: a non-empty
 * mask of NB_NEIGH_MASSIVE = 1, NB_NEIGH_MASSLESS = 2 (a class that is not of it is never read and gets NB_GROUP_NONE);
 * linking_length: finite and >= 0; group: [total_len]; n_groups (nullable): the number of groups, counted on the host from the
 * copied labels.
 *   nb_hip_groups             three launches in the stream: the table of the call's scratch set to the identity, the pair scan
 *                             over j < i whose links meet in that table through agent-scope relaxed integer atomics (load,
 *                             compare-and-swap, minimum) on global addresses, and the pass that reads the labels off.  No upload,
 *                             download 4 bytes per particle, one sync.  Enqueued, blocking and invisible to the steps like
 *                             nb_hip_neighbours; sharded pipelines abort like it.  Nothing to link (linking_length == 0, fewer than
 *                             two particles of the mask) fills every particle of the mask with its own index and launches nothing.
 *   nb_hip_ensemble_groups    every member of an ensemble, uniform or ragged, in the same three launches; one mask and one
 *                             linking length for all.  The labels are packed, member b at offsets[b] of nb_hip_ragged_layout, and
 *                             count within their member: no group crosses members.  n_groups: [count].  Member b's entries are
 *                             those of nb_hip_groups of a SimPipeline holding the same particles.
 * The smallest index of a connected component does not depend on the order the links are met in: a result is a function of the
 * state and the arguments alone, and there is no float atomic.  Every check -- NULL arguments, an empty or unknown mask, a
 * non-finite or negative linking length, a call before the data is set -- runs before any device touch and ends in
 * "file:line [func] ..." + abort().
 * Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_groups", dlsym "nb_hip_ensemble_groups").
 */
void nb_hip_groups(SimPipeline *sim, uint32_t members, float linking_length, uint32_t *group /* [total_len] */, uint32_t *n_groups /* nullable */);
void nb_hip_ensemble_groups(SimBatch *batch, uint32_t members, float linking_length, uint32_t *group /* packed, member b at offsets[b] */,
                            uint32_t *n_groups /* [count], nullable */);

/*
 * Adaptive time steps chosen on the device (definitions: include/nbody_adaptive.h; kernels: nbody_amd/csrc/timestep.hip).
 *   nb_hip_adaptive_steps         n steps, each of the size the criterion gives for the state before it; blocking
 *   nb_hip_adaptive_steps_async   the same, enqueue only
 *   nb_hip_adaptive_collect       waits for the last adaptive call and copies its log (n floats, may be NULL) and result
 *   nb_hip_timestep               the criterion alone (no span clip) for the latest state; changes nothing observable
 *   nb_hip_ensemble_adaptive_steps   the same for every member of a SimBatch: dt_log[n][count], out[count], either may be NULL
 * For every step the call enqueues the criterion launch -- a small reduction over acc and radius that writes the step size
 * where the step kernels read it (the pipeline's device dt, an ensemble's dt[count]), advances a float64 time on the device,
 * counts and logs -- and then exactly the launches a one-step PerformSimUpdate / nb_hip_batch_update makes, without its
 * step-size upload.  There is no host synchronisation inside the call; one copy at the end brings the log and the result.
 * The contract: dt_log[i] is, bit for bit, the host criterion of include/nbody_adaptive.h applied to the state before step i,
 * and the state afterwards is bit for bit that of PerformSimUpdate(sim, 1, dt_log[i]) for i = 0 .. n - 1 (for an ensemble:
 * nb_hip_batch_update_dts(batch, 1, dt_log[i])); a member's row does not depend on count, its index or the other members.
 * NB_ADAPT_PRIME first runs one dt = 0 step (equal to PerformSimUpdate(sim, 1, 0)), not logged and not counted.  The step
 * size cached on the host is dropped, so the next fixed-step call uploads its own.  Chains of adaptive steps are plain
 * launches: they are not captured into hipGraphs, and the one-workgroup n-step chain is not used (a one-step call never is).
 * Abort, before any device is touched, for a NULL argument, a configuration include/nbody_adaptive.h rejects and n > 2^20;
 * for sharded pipelines and ragged ensembles; and before the first SetSimulationData / nb_hip_batch_set_data.  n = 0 does
 * nothing.  Added WITHOUT a version bump: detect them by symbol (dlsym "nb_hip_adaptive_steps").
 */
void nb_hip_adaptive_steps(SimPipeline *sim, uint32_t n, const NbAdaptive *cfg, float *dt_log /* n or NULL */, NbAdaptiveResult *out);
void nb_hip_adaptive_steps_async(SimPipeline *sim, uint32_t n, const NbAdaptive *cfg);
void nb_hip_adaptive_collect(SimPipeline *sim, float *dt_log /* n or NULL */, NbAdaptiveResult *out);
void nb_hip_timestep(SimPipeline *sim, const NbAdaptive *cfg, float *dt);
void nb_hip_ensemble_adaptive_steps(SimBatch *batch, uint32_t n, const NbAdaptive *cfg, float *dt_log /* [n][count] */,
                                 NbAdaptiveResult *out /* [count] */);

/*
 * Leapfrog (kick-drift-kick) steps (definitions: include/nbody_leapfrog.h; the statement: nbody_amd/csrc/leapfrog_common.h;
 * kernels: nbody_amd/csrc/leapfrog.hip).
 *   nb_hip_leapfrog_steps         n steps of size dt; blocking
 *   nb_hip_leapfrog_steps_async   the same, enqueue only (nb_hip_sync waits)
 *   nb_hip_ensemble_leapfrog         n steps of every member of a SimBatch, one dt for all; blocking
 *   nb_hip_ensemble_leapfrog_dts     the same with dt[count], one step size per member
 * A step is open(dt), exactly the launches of a one-step PerformSimUpdate(sim, 1, 0) / nb_hip_batch_update(batch, 1, 0), and
 * close(dt); between two force launches one pass closes the step behind it and opens the next.  The step kernels' own step
 * size holds 0 during the call and the step size cached on the host is dropped, so the next fixed-step call uploads its own.
 * The object remembers whether acc is the acceleration of the state it holds: true after a leapfrog call (an adaptive call
 * with NB_ADAPT_LEAPFROG included), false after SetSimulationData / nb_hip_batch_set_data, any Euler update, traced update or
 * Euler adaptive call.  A call that finds it false first runs one one-step dt = 0 update, so the first call of a sequence
 * costs n + 1 force evaluations and every following one n.  The contract: the state afterwards is, bit for bit, what the
 * caller gets from GetSimulationData -> open in float32 -> SetSimulationData -> PerformSimUpdate(sim, 1, 0) ->
 * GetSimulationData -> close -> SetSimulationData per step, on every launch route, and n steps in one call have the bits of
 * the same steps in any split into calls.  The adaptive calls above honour NB_ADAPT_LEAPFROG: per step the criterion on the
 * current acc, the span clip, open(dt_i), force, close(dt_i); dt_log[i] is the host criterion of the state before step i
 * and the state that of nb_hip_leapfrog_steps(sim, 1, dt_log[i]) for i = 0 .. n - 1.
 * Chains of leapfrog steps are plain launches: no hipGraph, no one-workgroup chain.  Abort, before any device is touched,
 * for a NULL argument, for sharded pipelines and ragged ensembles, and before the first SetSimulationData /
 * nb_hip_batch_set_data.  n = 0 does nothing.  Added WITHOUT a version bump: detect them by symbol (dlsym
 * "nb_hip_leapfrog_steps").
 */
void nb_hip_leapfrog_steps(SimPipeline *sim, uint32_t n, float dt);
void nb_hip_leapfrog_steps_async(SimPipeline *sim, uint32_t n, float dt);
void nb_hip_ensemble_leapfrog(SimBatch *batch, uint32_t n, float dt);
void nb_hip_ensemble_leapfrog_dts(SimBatch *batch, uint32_t n, const float *dt /* [count] */);

/* Library/ABI version: major*10000 + minor*100 + patch. */
int nb_hip_version(void);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_HIP_H */
