// launch_shape.hip -- the host-side launch policy of the force kernels: which (K, W, split, unit, lanes) a launch gets,
// its grid / block / LDS geometry, and the auto rules of the lane-split, chain, ensemble and fused-finish paths.
// Plain host arithmetic with constants fitted to scans (the tables and derivations sit beside each rule).  This file
// emits no device code: the kernels are kernels.hip, and only they are part of the kernel-source hash bench.py ties PMC
// figures to (tests/test_isa.py holds this file to "no kernel").
#include "launch_shape.h"

namespace nb {
namespace {

constexpr int WAVE = 64;    // lanes per wave
constexpr int CHUNK = 64;   // sources per staged tile = the default slice granule (kernels.hip)

// Launches that do not even fill the chip once with K = 2 / W = 16 workgroups (fewer than 65 536 receivers on 256
// CUs) are priced in microseconds by a model fitted to exhaustive (K, W, split, unit) scans at N = 250 ... 50 000
// (tools/sweep_shapes.py; profiles/r02_sweep_shapes_units.txt holds the latest scan, 3 360 timed shapes).  There a wave is
// latency-bound, not issue-bound: alone on its SIMD it needs LAT us per 64-source chunk and receiver set (a serial
// dependency chain), and only beyond ~2 waves per SIMD does the chunk time grow with occupancy -- at THR us per wave,
// worse (factor A) the emptier the SIMD, and worse again for K = 1 (K1A).  Every wave also costs UFIX chunks of fixed
// work (launch, receiver loads, the LDS reduction), which is what stops the split from growing without bound, and a
// split adds the finish kernel.  Cutting the sources into more parts and finer granules shortens every wave's chain, so
// small launches want shapes the big-launch model would never pay for: N = 250 runs 3.2 us per step with 16 waves of 8
// sources instead of 4.6 us with two waves of 64, N = 2 000 5.4 instead of 6.7, N = 4 000 6.8 with 8 parts of 256-thread
// workgroups.  Mean regret of the model's pick against the scan's best: 1.7 % (worst 4.4 %).
double small_launch_cost_us(uint32_t n_recv, uint32_t n_src, int k, int w, int sp, int unit, int cus) {
    constexpr double LAT = 1.575, THR = 0.7545, K1 = 0.987, K1A = 0.178, A = 0.179, MIX = 0.874;
    constexpr double FINISH = 2.08, W4 = 1.035, UFIX = 0.15, BASE = 2.27;
    // the longest wave slice of a workgroup, in 64-source chunks (a fraction of one when the slice granule is finer)
    const uint32_t granules = (n_src + unit - 1) / unit;
    const uint64_t groups = ((uint64_t)n_recv + WAVE * k - 1) / (WAVE * k) * (uint64_t)sp;
    const uint64_t capacity = (uint64_t)cus * (32 / w);
    const uint64_t full = groups / capacity, left = groups % capacity;
    const uint32_t part_granules = (granules + sp - 1) / sp;
    const uint32_t wave_granules = (part_granules + w - 1) / w;
    const double units = (double)k * (wave_granules ? wave_granules : 1) * (double)unit / (double)CHUNK + UFIX;
    auto chunk_time = [&](double occ) {  // us per chunk and receiver set with `occ` waves on every SIMD
        const double f = k == 1 ? K1 + K1A * (8.0 - occ) / 8.0 : 1.0;
        const double busy = occ * THR * f * (1.0 + A * (8.0 - occ) / 8.0);
        return LAT > busy ? LAT : busy;
    };
    double t = (double)full * units * chunk_time(8.0);
    if (left) {
        // the busiest CU holds ceil(left / CUs) workgroups of w waves on its 4 SIMDs
        double occ = (w / 4.0) * (double)((left + cus - 1) / cus);
        if (occ > 8.0) occ = 8.0;
        const double lock = units * chunk_time(occ);                                    // runs after the full rounds
        const double fluid = units * chunk_time(8.0) * (double)left / (double)capacity;  // packs in behind them
        t += full ? MIX * lock + (1.0 - MIX) * fluid : lock;
    }
    if (sp > 1) t += FINISH;
    if (w == 4) t *= W4;
    return t + BASE;  // what every step pays whatever its shape (dispatch, kernel boundary): keeps ties ties
}

}  // namespace

// Lane-split shapes ("lanes" = 0, auto), from a scan of lanes x w over N = 300 ... 10 000 (tools/lane_probe.py,
// profiles/r03_lane_split_scan.txt; us per step, best lane-split shape vs the best classic shape the model above picks):
//   N = 500: 3.11 vs 3.86   800: 3.25 vs 4.25   1 200: 3.70 vs 4.98   2 000: 3.93 vs 5.41   4 000: 5.88 vs 6.93
//   5 000: 8.62 vs 8.42     8 000: 13.3 vs 12.7   10 000: 20.6 vs 15.8
// i.e. 15-28 % faster while a step is latency (N x M <~ 9e6), slower once it is throughput: every workgroup stages ALL
// the sources in LDS and the per-lane LDS reads cost issue slots a wave-uniform scalar operand does not.  Which (lanes, w)
// wins moves with the size; neighbours are within 2-3 % of each other.
int lane_split_rule(uint32_t n_recv, uint32_t n_src, int *w) {
    const double pairs = (double)n_recv * (double)n_src;
    *w = 16;
    if (n_src == 0 || n_recv == 0 || n_src > LANE_SPLIT_MAX_SRC || pairs > 9.0e6) return 1;
    if (pairs <= 1.5e5) {
        *w = 8;
        return 4;
    }
    if (pairs <= 2.5e6) {
        *w = 8;
        return 8;
    }
    return 4;
}

LaunchShape choose_shape(LaunchShape want, uint32_t n_recv, uint32_t n_src, int compute_units) {
    // Workgroups of one launch all take the same time, so a launch costs
    //     (rounds + tail) * (work per workgroup),   rounds = ceil(workgroups / resident capacity),
    // and one workgroup past a round boundary costs a whole round (1025 workgroups on 512 slots run 1.5x as
    // long as 1024; profiles/r01_shard_overhead_before_fix.txt).  Work per workgroup = K receivers per lane x
    // the 64-source chunks one wave walks.  Pick the cheapest (K, W, split); ties go to the larger K, larger W,
    // smaller split.  More, shorter workgroups also shrink the launch's ramp-up/ragged-end share.  K = 4 is left out: 71 VGPRs, lower
    // occupancy, never faster (profiles/r01_sweep4_shapes_by_n.txt).
    if (compute_units <= 0) compute_units = 256;
    if (shape_on_auto(want)) {   // an explicit LDS-tile route or shape knob asks for the classic kernel
        int w = 16;
        const int lanes = lane_split_rule(n_recv, n_src, &w);
        if (lanes > 1) {
            want.lanes = lanes;
            want.w = w;
        }
    }
    if (want.lanes > 1) {
        // one receiver per lane, no source split, 8-source granules, LDS-staged sources
        LaunchShape sh = want;
        sh.k = 1;
        sh.w = (want.w == 4 || want.w == 8 || want.w == 16) ? want.w : 16;
        if (sh.lanes == 8 && sh.w == 4) sh.w = 8;   // eight groups: instantiated for 8 and 16 waves
        if (sh.lanes != 2 && sh.lanes != 4 && sh.lanes != 8) sh.lanes = 4;
        sh.split = 1;
        sh.unit = 8;
        sh.variant = VARIANT_LDS;
        return sh;
    }
    if (want.variant == VARIANT_LDS) want.unit = CHUNK;  // the LDS route stages whole 64-source tiles, whatever was asked
    const uint32_t chunks = (n_src + CHUNK - 1) / CHUNK;
    const bool small = ((uint64_t)n_recv + 2 * WAVE - 1) / (2 * WAVE) < (uint64_t)compute_units * 2;
    LaunchShape best = want;
    best.lanes = 1;
    double best_cost = -1.0;
    for (int k = 2; k >= 1; k--) {
        if (want.k != 0 && want.k != k) continue;
        for (int w = 16; w >= 4; w /= 2) {
            if (want.w != 0 && want.w != w) continue;
            for (int sp = 1; sp <= MAX_SPLIT; sp++) {
                if (want.split != 0 && want.split != sp) continue;
                // small launches: 1024-thread workgroups exactly while the whole launch is a handful of unsplit tiles
                // (16 waves per tile beat 8 there: 4.2 vs 4.6 us at N = 800); beyond that 256- and 512-thread
                // workgroups pack better, and the model overrates W = 16
                const bool few_unsplit_tiles = sp == 1 && ((uint64_t)n_recv + WAVE * k - 1) / (WAVE * k) <= 24;
                // ... with at least ~16 sources for every wave: 8 waves when there are no more than 128 sources
                // (N = 250: 2.9 us with 8 waves of 16 sources, 3.2 with 16 waves of 8)
                const int tiny_w = n_src <= 128 ? 8 : 16;
                if (small && want.w == 0 && (few_unsplit_tiles ? w != tiny_w : w == 16)) continue;
                // slice granule: 64 unless the launch is latency-bound; a finer one only has to win where a part holds
                // fewer chunks than the workgroup has waves, and ties keep the coarser granule (64 first)
                for (int unit = CHUNK; unit >= 8; unit /= 2) {
                    if (want.unit != 0 && want.unit != unit) continue;
                    if (!small && want.unit == 0 && unit != CHUNK) continue;
                    double cost;
                    if (small) {
                        cost = small_launch_cost_us(n_recv, n_src, k, w, sp, unit, compute_units);
                    } else {
                        const uint64_t groups = ((uint64_t)n_recv + WAVE * k - 1) / (WAVE * k) * (uint64_t)sp;
                        const uint64_t capacity = (uint64_t)compute_units * (32 / w);  // 8 waves per SIMD at <= 64 VGPRs
                        const uint64_t rounds = (groups + capacity - 1) / capacity;
                        const uint32_t part_chunks = (chunks + sp - 1) / sp;
                        const uint32_t wave_chunks = (part_chunks + w - 1) / w;
                        // + 1 chunk-equivalent per workgroup for prologue/epilogue; + TAIL rounds per launch for ramp-up
                        // and the ragged end (measured: 2-round launches run 4.5 % over, 16-round ones 0.1 % over:
                        // profiles/r01_shard_overhead_split.txt); a split adds the finish kernel and the parts traffic
                        constexpr double TAIL = 0.13;
                        cost = ((double)rounds + TAIL) * ((double)k * (wave_chunks ? wave_chunks : 1) + 1.0);
                        if (sp > 1) cost += 3.0 + 0.02 * sp;
                        if (w < 16) cost *= 1.01;
                        // K = 1 per interaction at large N: 1.6 % slower than K = 2 with the plain body (48.6 vs 47.8 ms
                        // per launch at N = 2^20; it was 25 % with the packed body, whose single statement ran alone)
                        if (k == 1) cost *= 1.02;
                    }
                    if (best_cost < 0.0 || cost < best_cost * 0.999) {
                        best_cost = cost;
                        best.k = k;
                        best.w = w;
                        best.split = sp;
                        best.unit = unit;
                    }
                }
            }
        }
    }
    if (best_cost < 0.0) {  // explicit w = 1 (or a tuning-build shape): honour the request as given
        best.k = want.k ? want.k : 2;
        best.w = want.w ? want.w : 16;
        best.split = want.split ? want.split : 1;
        best.unit = want.unit ? want.unit : CHUNK;
    }
    return best;
}

dim3 step_grid(LaunchShape s, uint32_t n_recv) {
    if (s.lanes > 1) return dim3((n_recv + WAVE / s.lanes - 1) / (WAVE / s.lanes), 1);
    return dim3((n_recv + WAVE * s.k - 1) / (WAVE * s.k), s.split > 1 ? s.split : 1);
}

size_t step_lds_bytes(LaunchShape s, uint32_t n_src) {
    if (s.lanes <= 1) return 0;
    (void)n_src;   // the sources pass through one tile of 2 * 64 * w entries, whatever their number
    return (size_t)2 * WAVE * s.w * 12 + ((size_t)s.w + 1) * WAVE * sizeof(float2);   // tile (x, y, G*m) + [w * lanes][64 / lanes] partial sums + 64 second-level sums
}
dim3 finish_grid(uint32_t n_recv) { return dim3((n_recv + 255u) / 256u); }
dim3 finish_block() { return dim3(256); }
dim3 step_block(LaunchShape s) { return dim3(WAVE * s.w); }

uint32_t chain_tiles(uint32_t n_recv) {
    for (uint32_t t = 1; t <= 4; t *= 2)
        if (n_recv <= t * WAVE * CHAIN_K) return t;
    return 0;
}

// ---- ensembles ------------------------------------------------------------------------------------------------------
// The lane-split shape of an ensemble is a function of N alone (members differ in their source counts, and a member's bits
// must not depend on them): the auto rule at n_src = n_recv, whose cut-off N x N <= 9e6 is N <= 3 000.
int batch_lane_shape(uint32_t n_recv, int *w) { return lane_split_rule(n_recv, n_recv, w); }

// ---- fused finish ("fused_finish" knob, auto) ------------------------------------------------------------------------
// What a split step WITHOUT its second, dependent kernel (step_chain.hip fused_finish_applies, kernels.hip
// step_kernel<..., FUSED>) buys is the finish kernel's boundary minus the ticket's round trip
// (profiles/r04_fused_finish.txt, us per step, cached graph replays | plain launches):
//   N = 5 000 +0.6 | -0.6    8 000 0.0 | -0.5    10 000 -0.4 | -1.0    14 000 -1.2 | -0.8    20 000 -0.7 | -0.9
//   50 000 -1.5 | -1.6    100 000 -2.3 | -2.3
// Auto (2, default): unsharded steps on the scalar-cache route with N x M >= 4e7 (N >~ 9 000: from where it also wins
// inside a hipGraph) and at most 200 000 receivers (beyond that the finish kernel is < 0.3 % of a step, and the kernels
// of the BASELINE sizes stay the ones the PMC profiles describe).  Sharded steps keep the two-kernel form.
constexpr double FUSED_FINISH_MIN_PAIRS = 4.0e7;
constexpr uint32_t FUSED_FINISH_MAX_RECV = 200000;

bool fused_finish_rule(uint32_t n_recv, uint32_t n_src) {
    return (double)n_recv * (double)n_src >= FUSED_FINISH_MIN_PAIRS && n_recv <= FUSED_FINISH_MAX_RECV;
}

// ---- dealt launches ("deal" knob, auto) -------------------------------------------------------------------------------
// The grid of a dealt launch is the item count plus `extra` workgroups (kernels.hip dealt_kernel): what a fast XCD takes
// over from a slow one comes out of the extra ones, so extra bounds the speed difference the scheme can absorb -- items / 32
// is 3 %, three times what the clocks ask for (the odd XCDs hold 1-2 % less) -- and every extra workgroup that finds the
// counter spent costs one atomic and leaves.  Eight at least, one per XCD.
uint32_t deal_items(LaunchShape s, uint32_t n_recv) {
    const dim3 g = step_grid(s, n_recv);
    return g.x * g.y;
}

uint32_t deal_extra(uint32_t items) { return items / 32 > 8 ? items / 32 : 8; }

// What dealing can win is the slow XCDs' lag at the end of a launch, a fixed FRACTION of it; what it costs is fixed per
// launch (the draws of the first resident round arrive together; the drain of the extra workgroups).  Auto therefore deals
// only launches of at least DEAL_MIN_ROUNDS rounds of resident workgroups (two 1 024-thread workgroups per CU).  Same-box
// A/B, kernel ms per launch, classic | dealt, gain against the classic repeats' own spread (profiles/r23_deal_probe.json):
//   N = 262 144,  8 rounds:  6.107 |  6.132  -0.40 %  (spread 0.58 %)      N = 524 288, 24 rounds: 12.261 | 12.220  +0.33 % (0.22 %)
//   N = 2^20,    32 rounds: 48.930 | 48.342  +1.20 %  (spread 0.14 %)      (N = 131 072, 10 rounds, runs the fused finish: never dealt)
// 24 rounds is a gain of 1.5 spreads, 32 rounds one of 8.9: the rule starts where the gain is beyond doubt.
constexpr uint32_t DEAL_MIN_ROUNDS = 32;

bool deal_pays(uint32_t items, int compute_units) {
    if (compute_units <= 0) compute_units = 256;
    return (uint64_t)items >= (uint64_t)DEAL_MIN_ROUNDS * 2u * (uint64_t)compute_units;
}

bool deal_rule(uint32_t n_recv, uint32_t n_src, int compute_units) {
    const LaunchShape sh = choose_shape({.lanes = 1}, n_recv, n_src, compute_units);
    if (dealt_kernel_fn(sh) == nullptr) return false;
    if (sh.split > 1 && fused_finish_rule(n_recv, n_src)) return false;
    return deal_pays(deal_items(sh, n_recv), compute_units);
}

}  // namespace nb
