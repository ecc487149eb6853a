// kernels.h -- internal (C++) interface between the pipeline and the gfx950 force kernels (kernels.hip): their parameter
// blocks, entry points and the two launches that have no shape to choose.  Which shape a launch gets is launch_shape.h,
// the AoS <-> SoA converters are convert.h.  Not part of the C-ABI; include/nbody_hip.h is.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nb {

enum : uint32_t {
    STEP_ACC_IN = 1u,       // start each receiver's sum from acc[] instead of zero
    STEP_NO_FINALIZE = 2u,  // store the sums into acc[] and skip the integrator
};
// (experiment, knob "fused_finish") split steps without the finish kernel: the last-arriving workgroup of a receiver tile
// adds the parts itself -- parts as agent-scope (sc1) stores / loads, one ticket per tile; see step_kernel<..., FUSED>

enum : int {
    VARIANT_LDS = 0,   // wave-private LDS tiles (coalesced float2 loads -> ds_write -> broadcast ds_read_b128)
    VARIANT_SMEM = 1,  // wave-uniform source loads through the scalar cache (s_load_dwordx8/16)
};

// Everything one force(+integrate) launch needs.  Passed by value as the single kernel argument,
// so a hipGraph kernel node is re-pointed by rewriting one struct.
struct StepParams {
    // sources = snapshot of the previous step (Jacobi): positions and premultiplied G*m
    const float2 *src_pos;
    const float *src_gm;
    uint32_t src_begin[2];  // two half-open source ranges, walked back to back;
    uint32_t src_end[2];    // the second is empty except in the overlapped sharded step
    // receivers owned by this launch
    const float2 *pos_in;
    float2 *pos_out;
    float2 *vel;
    float2 *acc;
    const float *radius;
    uint32_t n_recv;      // receivers this launch computes (logical indices 0 .. n_recv)
    // logical receiver i lives in slot i + (i >= recv_split ? recv_gap : 0): a shard's massive slice is padded
    // to the uniform all-gather chunk, and the pad slots must not cost workgroups (one extra workgroup on a
    // 2-round grid is +50 %, profiles/r01_shard_overhead_before_fix.txt).  Unsharded: recv_split = n_recv.
    uint32_t recv_split;
    uint32_t recv_gap;
    // new positions of the receivers in slots [0, n_mirror) are also written here (the shard's slice of
    // the next gathered source array); n_mirror == 0 disables it
    float2 *mirror;
    uint32_t n_mirror;
    // step size, read from device memory -- where the reference keeps it too (the uniform block, sim_gpu.h:8-12,
    // re-uploaded when dt changes, sim_gpu.c:268-284).  A hipGraph chain therefore never needs re-patching for a new dt.
    const float *dt;
    uint32_t flags;
    // source split: gridDim.y = split workgroups share one receiver tile, each over 1/split of the source
    // chunks; with split > 1 the step kernel only stores its sums to parts[part][receiver] and finish_kernel
    // adds the parts in order and integrates.  Fills the chip when there are few receiver tiles and lands the
    // workgroup count near a round boundary (see choose_shape).
    float2 *parts;
    uint32_t split;
    uint32_t *tickets;    // fused finish only: one arrival counter per receiver tile, zero between launches
    // granule of the source slicing: a wave's slice is a whole number of `unit` sources (64, or 32 / 16 / 8 for
    // latency-bound launches whose parts hold fewer 64-source chunks than the workgroup has waves -- with 64 only, a
    // part of 6 chunks keeps 6 of 16 waves busy).  Slices stay 8-aligned, so the scalar loads keep their alignment.
    // Scalar-cache route only: the LDS route stages whole 64-source tiles and always runs with 64 -- the two routes
    // give the same bits whenever the granule is 64.  Two-range (overlapped) steps always use 64.
    uint32_t unit;
    // dealt launches only (dealt_kernel): the ticket counter of the pipeline, zero between launches, and the number of
    // (receiver tile, source part) items = tiles x split; null / 0 in every other launch
    uint32_t *deal;
    uint32_t deal_items;
};

// Ticket t of a dealt launch is receiver tile t % tiles of source part t / tiles: the order in which a 2-D grid of
// (tiles, split) workgroups is linearised, so a dealt launch touches memory in the order the classic one does.  Tickets
// from tiles x split on stand for nothing (live = false).  The kernel and the host (nb_hip_deal_item) call this one copy.
struct DealItem {
    uint32_t tile, part;
    bool live;
};
__host__ __device__ inline DealItem deal_item(uint32_t ticket, uint32_t tiles, uint32_t split) {
    if (tiles == 0 || ticket / tiles >= split) return DealItem{0, 0, false};
    return DealItem{ticket % tiles, ticket / tiles, true};
}

// The parameters of a plain step: one source range [0, n_src), receivers without a gap or a mirror, sums from zero,
// integrated, unsplit.  The one-world pipeline starts from it (step_chain.hip whole_step), an ensemble member's
// lane-split step is exactly it (kernels.hip batch_lane_split_kernel).
__host__ __device__ inline StepParams plain_step(const float2 *src_pos, const float *src_gm, uint32_t n_src, const float2 *pos_in,
                                                 float2 *pos_out, float2 *vel, float2 *acc, const float *radius, uint32_t n_recv,
                                                 const float *dt, uint32_t unit) {
    return StepParams{.src_pos = src_pos, .src_gm = src_gm, .src_begin = {0, 0}, .src_end = {n_src, 0}, .pos_in = pos_in,
                      .pos_out = pos_out, .vel = vel, .acc = acc, .radius = radius, .n_recv = n_recv, .recv_split = n_recv,
                      .dt = dt, .split = 1, .unit = unit};   // every field not named is zero / null
}

// A whole n-step chain of a world that fits ONE workgroup, run inside one launch (chain_kernel): positions ping-pong in
// LDS, velocities and radii stay in registers, two workgroup barriers per step and no kernel boundary (1.6-1.8 us each
// on this chip, more than such a step's arithmetic).  Sixteen waves: `tiles` receiver tiles of 64 * K receivers, 16 / tiles
// waves per tile, each over a 1/W slice of the sources in 8-source granules -- the summation order of the per-step
// kernel launched with k = K, w = 16 / tiles, split = 1, unit = 8, so the two paths give the same bits.
struct ChainParams {
    float2 *pos;          // in: state before the chain; out: state after it (updated in place)
    float2 *vel;          // in / out
    float2 *acc;          // out: the last step's sums (Particle.acc is observable)
    const float *radius;
    const float *src_gm;  // G*m of the sources = the first n_src receivers (massive-first order)
    uint32_t n_recv;      // receivers, <= 128 * tiles
    uint32_t n_src;       // sources, <= n_recv
    uint32_t steps;       // steps to run, >= 1
    uint32_t tiles;       // 1, 2 or 4
    const float *dt;      // step size in device memory, as for the per-step kernels
};

constexpr uint32_t CHAIN_K = 2;            // receivers per lane of the chain
constexpr uint32_t CHAIN_MAX_RECV = 512;   // 4 tiles of 128 receivers (K = 2)

// An ensemble of `count` independent worlds stepped by one launch (batch_chain_kernel: one workgroup per member runs the
// whole chain; batch_lane_split_kernel: gridDim.y = members, one launch per step).  Member-major SoA: every array is
// [count][stride], stride >= the largest member and a multiple of 64, so each member's rows stay 256-byte aligned.
// Member b's sources are its first mass_len[b] particles; its step size is dt[b].  Both are read from device memory.
//
// A launch finds its member in one of two ways, and the parameter type says which (kernels.hip member_of):
//   BatchParams    by block index: workgroup g steps member g, every member has n_recv particles;
//   RaggedParams   by list: workgroup g steps member members[g] of n_len[members[g]] particles -- a ragged ensemble, whose
//                  launch covers one GROUP of members that share a launch shape.  n_recv and tiles are not read: both
//                  come from n_len, so a member's shape is a function of its own size alone.
// Each ensemble kernel is one template over the two; nothing else of a kernel depends on the addressing.
struct BatchParams {
    float2 *pos_in;       // state before the step (chain: before the call, updated in place)
    float2 *pos_out;      // lane-split: state after the step; chain: unused
    float2 *vel;
    float2 *acc;
    const float *radius;
    const float *gm;      // G*m, 0 in rows that are not sources
    const uint32_t *mass_len;   // [count]
    const float *dt;            // [count]
    uint32_t n_recv;      // particles per member
    uint32_t stride;      // rows per member
    uint32_t steps;       // chain only: steps of this launch, >= 1
    uint32_t tiles;       // chain only: chain_tiles(n_recv)
};

struct RaggedParams : BatchParams {
    const uint32_t *n_len;     // [count] particles per member
    const uint32_t *members;   // [workgroups of the group] member indices
};

// What a traced ensemble chain (batch_trace_chain_kernel) takes besides its steps: every `every`-th step of the CALL the
// member's eight float64 energy sums (diag_sums.h order, the bits of ensemble_phi_kernel + ensemble_reduce_kernel for that
// state) go to rows[record][member][8], whichever way the launch finds its members.  A call longer than one launch carries
// its record index across launches through `done`; the launch with done = 0 also records the state on entry (record 0), and
// may have steps = 0.
struct TraceParams {
    const float *mass;    // [count][stride], like gm
    double *rows;         // [records][count][8]
    uint32_t count;       // members of the ensemble (the row pitch)
    uint32_t every;       // >= 1
    uint32_t done;        // steps of this call that earlier launches ran
};

constexpr int MAX_SPLIT = 16;

struct LaunchShape;   // launch_shape.h

// Kernel entry point for a shape; used both for direct launches and for graph nodes.
const void *step_kernel_fn(LaunchShape s);
const void *step_kernel_fused_fn(LaunchShape s);   // nullptr when the shape has no fused-finish instantiation
const void *dealt_kernel_fn(LaunchShape s);        // nullptr when the shape has no dealt instantiation (1-D grid, StepParams::deal)
// second kernel of a split step (split > 1): adds the parts and finishes like the step kernel's epilogue
const void *finish_kernel_fn();

// the one-workgroup chain: 1024 threads, one block; tiles from chain_tiles(n_recv)
void launch_chain(hipStream_t st, const ChainParams &p);

// ensembles: the kernel of a lane-split shape (nullptr when not instantiated; `listed`: the RaggedParams instantiation), and
// the chain launches of `workgroups` members.  Both take the full block and pick the instantiation themselves: by list
// when p.members is set, else by block index (a kernel argument that points at a RaggedParams serves either way: the
// BatchParams is its head).
const void *batch_lane_split_fn(int w, int lanes, bool listed);
void launch_batch_chain(hipStream_t st, const RaggedParams &p, uint32_t workgroups);
void launch_batch_trace_chain(hipStream_t st, const RaggedParams &p, const TraceParams &t, uint32_t workgroups);

}  // namespace nb
