/*
 * nbody_hip_tuning.h -- test and tooling hooks of libnbody_hip.so.  NOT part of the C-ABI (include/nbody_hip.h is):
 * nothing here is stable, nothing here is needed to use the library, and every knob below is on "auto" in every
 * published number.  They exist so that the GPU suite can pin a launch shape (bit-equality tests across shardings need
 * one wave per workgroup), so that tools/ can scan shapes, and so that nbody-bench can price its "floor" column.
 *
 * History of why each one is not public (the measurements are under profiles/):
 *   k, w, split, unit, passes   launch shape; "auto" is within 1.2 % of the best explicit neighbour at every size the
 *                               GPU suite asks the hardware about (test_auto_launch_shape_is_near_the_best_...)
 *   lanes, fused_chain          small-world kernels; auto-selected below N ~ 4 000 / N <= 256, frozen since round 3
 *   deal, deal_extra            large launches dealt by ticket so that faster XCDs take more; auto from 32 rounds: -1.2 % per
 *                               launch at N = 2^20 (profiles/r23_deal_probe.json)
 *   fused_finish                the last workgroup of a receiver tile finishes it; auto from N x M >= 4e7, -0.4 ... -2.3 us
 *   readback, zero_copy_upload  the GUI frame loop's eager read-back / zero-copy upload heuristics, frozen since round 2
 */
#ifndef NBODY_AMD_NBODY_HIP_TUNING_H
#define NBODY_AMD_NBODY_HIP_TUNING_H

#include "nbody_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * key is one of (0 = auto unless stated):
 *   "k"         receivers per lane: 1 or 2 (4 only in TUNING=1 builds)
 *   "w"         waves (source slices) per workgroup: 1, 4, 8 or 16 (2 only in TUNING=1 builds); w = 1 makes the summation
 *               order independent of the launch geometry
 *   "split"     workgroups per receiver tile, each over 1/split of the sources (a finish kernel adds the parts): 1..16
 *   "unit"      granule of the source slicing: 8, 16, 32 or 64 sources (the LDS route always uses 64)
 *   "passes"    launches per step over consecutive source sub-ranges, chained through acc[]: 1..64 (auto: each pass's
 *               sources fit one XCD's L2)
 *   "lanes"     lane groups per wave over the same 64 / lanes receivers (lane_split_kernel): 2, 4 or 8; 1 = never
 *   "fused_chain"   one-workgroup worlds run a whole n-step call inside one launch: 2 (default) = auto (N <= 256 and
 *               N x M <= 3.6e4, calls of 2+ steps), 1 = whenever the world fits (N <= 512), 0 = never
 *   "fused_finish"  split shapes without their second kernel (the tile's last workgroup adds the parts and integrates):
 *               2 (default) = auto (unsharded, scalar-cache route, N x M >= 4e7, <= 200 000 receivers), 1 = whenever the
 *               shape has a split, 0 = never
 *   "deal"      large step launches whose workgroups draw their (receiver tile, source part) from a ticket counter, over a
 *               grid a little larger than the item count, so that XCDs holding a higher clock take more of a launch
 *               (kernels.hip dealt_kernel): 2 (default) = auto (unsharded, scalar-cache route, k = 1 or 2, w = 16, no fused
 *               finish, at least 32 resident rounds of workgroups), 1 = whenever the shape allows, 0 = never; same bits
 *   "deal_extra"    workgroups a dealt launch holds on top of its items: 0 (default) = max(8, items / 32)
 *   "readback"  when the device state reaches the array named by nb_hip_note_host_array: 0 = only when GetSimulationData
 *               asks, 1 = at the end of every blocking PerformSimUpdate, 2 (default) = auto (eager once two updates in a
 *               row were each followed by a Get into the noted array)
 *   "render_merge"  how splat_kernel adds points to the count image: 1 (default) = lanes of a wave that hit the same word
 *               are merged first (one add per distinct word while merging pays), 0 = one atomic add per lane (the A/B of
 *               tools/render_probe.py; same bits)
 *   "render_detail" 1 = nb_hip_last_render_ms can split the last render into splat / disc / shade (three more event
 *               records per call), 0 (default) = the whole render only
 *   "field_shape"   which kernel nb_hip_potential_at / nb_hip_potential_map run: 0 (default) = auto (one wave per tile when
 *               the world has at most 2 blocks of 256 sources and the call at least 4 096 tiles of 128 samples, else the
 *               source split; profiles/r12_field_probe.json), 1 = the source split (8 waves share
 *               a tile of samples, 1/8 of the sources each), 2 = one wave per tile; same bits (tests/test_gpu_field.py)
 *   "gravity_shape" which kernel nb_hip_acceleration_at / nb_hip_acceleration_map run: 0 (default) = auto (the rule of
 *               "field_shape": field.hip has one pick_wave_shape and one pair of thresholds; the sweep for this pair body,
 *               profiles/r13_gravity_probe.json, puts its crossover in the same place), 1 = the source split, 2 = one wave
 *               per tile; same bits (tests/test_gpu_gravity.py)
 *   "tidal_shape"   which kernel nb_hip_tidal_at / nb_hip_tidal_map run: 0 (default) = auto (the same pick_wave_shape and
 *               thresholds, inherited, not retuned: tools/tidal_probe.py reports where this pair body's crossover lies), 1 = the
 *               source split, 2 = one wave per tile; same bits (tests/test_gpu_tidal.py)
 *   "zero_copy_upload"  1 (default) = SetSimulationData from the noted, page-locked array lets the split kernel read the
 *               records over PCIe itself; 0 = DMA copy into device staging, then the kernel
 * Returns the previous value; aborts on an unknown key or value.
 */
int nb_hip_tune(SimPipeline *sim, const char *key, int value);

/* 1 when the library was built with make TUNING=1: the launch shapes the cost model never picks (K = 4, W = 2) and the
 * NB_HIP_* environment presets of the hooks above exist in such builds only. */
int nb_hip_tuning_build(void);

/* Steps of the last update that ran inside one-workgroup chain launches ("fused_chain"). */
uint32_t nb_hip_last_fused_steps(const SimPipeline *sim);

/* Lane groups per wave (1, 2, 4 or 8) and source-slice granule of the last step launch. */
int nb_hip_launch_lanes(const SimPipeline *sim);
int nb_hip_launch_unit(const SimPipeline *sim);

/* What "auto" picks for an unsharded step of that size, pure host code: lane groups per wave (1 = the classic shape
 * nb_hip_plan_launch describes; through w the waves per workgroup), whether the source split runs without the finish
 * kernel, and the source-slice granule. */
int nb_hip_plan_launch_lanes(uint32_t n_recv, uint32_t n_src, int *w);
int nb_hip_plan_fused_finish(uint32_t n_recv, uint32_t n_src, int compute_units);
int nb_hip_plan_launch_unit(uint32_t n_recv, uint32_t n_src, int compute_units);

/* Dealt launches ("deal" hook).  nb_hip_last_deal: 1 when the step launches of the last update were dealt, with their item
 * count and the workgroups launched on top (either pointer may be NULL).  nb_hip_plan_deal: what "deal" = 2 decides for an
 * unsharded step of that size on the auto shape, pure host code.  nb_hip_deal_item: the (receiver tile, source part) ticket
 * `ticket` stands for in a launch of tiles x split items -- the function the kernel calls; returns 0 and writes nothing for
 * a ticket past the last item.  nb_hip_deal_counter: the pipeline's ticket counter, read back after a sync (0 between
 * launches; 0 for a pipeline that has none). */
int nb_hip_last_deal(const SimPipeline *sim, uint32_t *items, uint32_t *extra);
int nb_hip_plan_deal(uint32_t n_recv, uint32_t n_src, int compute_units);
int nb_hip_deal_item(uint32_t ticket, uint32_t tiles, uint32_t split, uint32_t *tile, uint32_t *part);
uint32_t nb_hip_deal_counter(SimPipeline *sim);

/* Device milliseconds of the kernels of the last nb_hip_energy / nb_hip_potential / nb_hip_potential_at /
 * nb_hip_potential_map / nb_hip_acceleration_at / nb_hip_acceleration_map / nb_hip_tidal_at / nb_hip_tidal_map /
 * nb_hip_profile / nb_hip_pair_counts / nb_hip_neighbours / nb_hip_groups (their own event pair, not the step's); 0 before the first call. */
double nb_hip_last_diag_ms(SimPipeline *sim);

/* The float32 thresholds nb_hip_pair_counts compares q against for these edges (nbody_amd/csrc/paircount_common.h): table
 * receives 255 floats, c[0 .. bins] and NaN behind them; returns the first step of the device's search.  Host code only. */
uint32_t nb_hip_pair_thresholds(const float *edges, uint32_t bins, float *table);

/* The span of nb_hip_neighbours / nb_hip_ensemble_neighbours (nbody_amd/csrc/neighbour.hip): the source blocks of 256 one
 * workgroup walks, for every later call of the process; 0 (default) = auto, the host's policy.  The result is the same for every
 * value: the GPU suite uses it to cross span boundaries at N ~ 1 000.  Returns the previous value.  Host code only. */
uint32_t nb_hip_neighbour_span(uint32_t blocks);

/* The span of nb_hip_groups / nb_hip_ensemble_groups (nbody_amd/csrc/group.hip): the source blocks of 256 one workgroup of the
 * pair launch walks, for every later call of the process; 0 (default) = auto, the host's policy.  The result is the same for
 * every value.  Returns the previous value.  Host code only. */
uint32_t nb_hip_group_span(uint32_t blocks);

/* The same for an ensemble: device milliseconds of the kernels of the last nb_hip_ensemble_energy /
 * nb_hip_ensemble_potential (an event pair of their own, not the update's); 0 before the first call. */
double nb_hip_ensemble_last_diag_ms(SimBatch *batch);

/* Traced ensemble updates (nb_hip_ensemble_trace): mode 0 = auto, 1 = always interleave the diagnostics launches with the
 * step launches, also where the one-workgroup chain could record by itself (total_len <= 512); and what the last traced
 * call did: fused = 1 when the chain recorded, and the kernel launches it made.  Either pointer may be NULL. */
void nb_hip_ensemble_trace_mode(SimBatch *batch, int mode);
void nb_hip_ensemble_last_trace_info(const SimBatch *batch, int *fused, uint32_t *launches);

/* Device milliseconds of the kernels of the last nb_hip_bounds / nb_hip_render_counts / nb_hip_render_rgba (an event pair
 * of their own); 0 before the first call.  parts (may be NULL) receives {bounds, clear + splat, disc, shade}: the last
 * bounds call in parts[0]; the other three need the "render_detail" hook and read 0 without it. */
double nb_hip_last_render_ms(SimPipeline *sim, double *parts);

/* Ensemble renders (nb_hip_ensemble_render_counts / _rgba): mode 0 = auto, 1 = the global path (clear, splat, disc pass,
 * shade) also where the image fits the one-workgroup tile path; what the last render did: tile_path = 1 when the tile
 * kernel ran, and the launches it enqueued (the clear counts as one), both 0 before the first render and left alone by
 * nb_hip_ensemble_bounds; and the device milliseconds of the kernels alone (not of the upload of the views or the copy
 * back) of the last render or bounds call (an event pair of their own, 0 before the first call).  Either pointer may be
 * NULL. */
void nb_hip_ensemble_render_mode(SimBatch *batch, int mode);
void nb_hip_ensemble_last_render_info(const SimBatch *batch, int *tile_path, uint32_t *launches);
double nb_hip_ensemble_last_render_ms(SimBatch *batch);

/* The last leapfrog call (nb_hip_leapfrog_steps, an adaptive call with NB_ADAPT_LEAPFROG; nb_hip_ensemble_leapfrog and the
 * ensemble's adaptive call for a SimBatch): the force evaluations it enqueued -- steps, plus one when it primed -- and
 * whether it primed, i.e. acc was not known to be the state's own.  Both 0 before the first call; either pointer may be NULL. */
void nb_hip_last_leapfrog_info(const SimPipeline *sim, uint32_t *force_launches, int *primed);
void nb_hip_ensemble_last_leapfrog_info(const SimBatch *batch, uint32_t *force_launches, int *primed);

/* Device allocations and events the library holds at this moment, process-wide: every allocation goes through one seam
 * (device_ctx.hip dev_alloc_bytes / dev_free) and every event through one owner type (pipeline_internal.h), and both count
 * there.  Plain host counters: no HIP call, works without a GPU.  An object that is destroyed gives back exactly what it
 * took (the GPU suite holds each kind of object to that).  Either pointer may be NULL. */
void nb_hip_live_resources(uint32_t *buffers, uint32_t *events);

#ifdef __cplusplus
}
#endif

#endif /* NBODY_AMD_NBODY_HIP_TUNING_H */
