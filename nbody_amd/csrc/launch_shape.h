// launch_shape.h -- which shape a force launch gets: the host-side launch policy (launch_shape.hip).  Plain host
// arithmetic with fitted constants; no device code, and not part of the kernel-source hash bench.py ties PMC figures to.
#pragma once

#include "kernels.h"

namespace nb {

constexpr uint32_t BATCH_MAX_RECV = 3000;   // lane_split_rule's own cut-off at n_src = n_recv (N x N <= 9e6)

// A launch shape; 0 = "auto" in a request to choose_shape.  Write one with named fields ({.k = 2, .w = 16}): the
// defaults are the all-auto request.
struct LaunchShape {
    int k = 0;                    // receivers per lane: 1, 2 (4 in tuning builds)
    int w = 0;                    // waves per workgroup = source slices: 1, 4, 8, 16 (2 in tuning builds)
    int variant = VARIANT_SMEM;   // VARIANT_*
    int split = 0;                // workgroups per receiver tile (source parts): 1 .. MAX_SPLIT
    int unit = 0;                 // sources per slice granule: 64 (default), 32, 16, 8
    // lane groups per wave (0 / 1: a wave's 64 lanes are 64 * k receivers).  2 or 4: the lanes of a wave split into that
    // many groups over the SAME 64 / lanes receivers, each group walking its own slice of the sources (lane_split_kernel):
    // w * lanes source slices per receiver inside ONE workgroup -- the parallelism a source split buys, without its
    // second kernel.  Latency-bound launches only (k = 1, split = 1, sources staged once in LDS).
    int lanes = 0;
};

inline bool operator==(const LaunchShape &a, const LaunchShape &b) {
    return a.k == b.k && a.w == b.w && a.variant == b.variant && a.split == b.split && a.unit == b.unit && a.lanes == b.lanes;
}

// Every field of a request left to choose_shape: only then may it pick the lane-split kernel, and the pipeline the
// one-workgroup chain (an explicit shape or LDS-tile route asks for the classic per-step kernel).
inline bool shape_on_auto(const LaunchShape &want) { return want == LaunchShape{}; }

constexpr uint32_t LANE_SPLIT_MAX_SRC = 1u << 18;   // sources a lane-split launch walks (one launch = one source pass)

// The auto rule for lane-split shapes: lanes (1 = use the classic kernel) and waves per workgroup.
int lane_split_rule(uint32_t n_recv, uint32_t n_src, int *w);

// Resolve "auto" (0) entries of `want` for a launch over n_recv receivers and n_src sources.
LaunchShape choose_shape(LaunchShape want, uint32_t n_recv, uint32_t n_src, int compute_units);

// the auto rule of the "fused_finish" knob: split steps of this size run without the finish kernel
bool fused_finish_rule(uint32_t n_recv, uint32_t n_src);

// Dealt launches ("deal" knob; kernels.hip dealt_kernel): the (receiver tile, source part) items of a shape, the workgroups
// launched on top of them, and the auto rule -- launches of at least DEAL_MIN_ROUNDS resident rounds.
uint32_t deal_items(LaunchShape s, uint32_t n_recv);
uint32_t deal_extra(uint32_t items);
bool deal_pays(uint32_t items, int compute_units);
// ... and for a step of that size on the auto shape: whether it deals at all
bool deal_rule(uint32_t n_recv, uint32_t n_src, int compute_units);

// Grid, block and dynamic LDS of a shape's step kernel (kernels.h step_kernel_fn), and of the finish kernel.
dim3 step_grid(LaunchShape s, uint32_t n_recv);
dim3 step_block(LaunchShape s);
size_t step_lds_bytes(LaunchShape s, uint32_t n_src);   // dynamic LDS of the launch (0 except for lane-split shapes)
dim3 finish_grid(uint32_t n_recv);
dim3 finish_block();

// the one-workgroup chain: tiles for n_recv receivers (0: the world does not fit)
uint32_t chain_tiles(uint32_t n_recv);

// ensembles: the lane-split shape for members of n_recv particles (lanes; 1 = none: N > BATCH_MAX_RECV)
int batch_lane_shape(uint32_t n_recv, int *w);

}  // namespace nb
