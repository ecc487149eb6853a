// step_chain.hip -- n fixed Euler steps of one device as device work: the launches of one step, cached hipGraph chains.
//
// Stands where the reference records its command buffer (src/lib/sim_gpu.c:258-361: copy -> barrier -> dispatch x n ->
// copy, re-recorded on every call).  Differences by design:
//   * ping-pong position buffers instead of a full device-to-device copy per step (sim_gpu.c:316-324);
//   * n-step chains are cached hipGraphs of kernel nodes, keyed on (length, passes, shape, ping-pong phase); the step
//     size sits in device memory like the reference's uniform (sim_gpu.c:268-284), so a new dt never rebuilds a chain;
//   * worlds that fit ONE workgroup run their chain inside one launch (nb::launch_chain), positions in LDS.
// The sharded step and its all-gather: shard_exchange.hip.  Device-chosen and leapfrog steps: step_schedule.hip.
#include "pipeline_internal.h"

namespace nbi {

constexpr size_t GRAPH_CACHE_MAX = 8;     // cached chains per pipeline; the least recently used one is evicted
// graph = 2 (auto): chains shorter than this stay plain launches.  A hipGraphLaunch costs the host ~12 us more than
// a few plain launches and a replayed node saves 1-2 us, so a graph pays from a dozen steps on
// (profiles/r02_frame_loop_latency.txt: 2-step frames 33 -> 44 us with a graph, 8-step frames still 98 -> 102 us).
constexpr uint32_t GRAPH_AUTO_MIN_CHAIN = 16;

// Make room for one more cached chain: the least recently used one goes (a frame loop with a varying chain length
// or dt must not grow device-side graph execs without bound).
void evict_for_one_more(SimPipeline *s) {
    while (s->graphs.size() >= GRAPH_CACHE_MAX) {
        size_t victim = 0;
        for (size_t i = 1; i < s->graphs.size(); i++)
            if (s->graphs[i].last_use < s->graphs[victim].last_use) victim = i;
        ASSERT_HIP(hipStreamSynchronize(s->stream), "sync before evicting a cached chain");
        destroy_graph(s->graphs[victim]);
        s->graphs.erase(s->graphs.begin() + (long)victim);
    }
}

void destroy_graph(StepGraph &g) {
    if (g.exec) ASSERT_HIP(hipGraphExecDestroy(g.exec), "hipGraphExecDestroy");
    if (g.graph) ASSERT_HIP(hipGraphDestroy(g.graph), "hipGraphDestroy");
    g.exec = nullptr;
    g.graph = nullptr;
    g.nodes.clear();
    g.params.clear();
}

uint32_t dealt_extra(const SimPipeline *s, uint32_t items);

nb::LaunchShape resolve_shape(SimPipeline *s) {
    nb::LaunchShape want = s->want;
    // the model sees one launch: with source passes that is 1/passes of the sources
    nb::StepParams probe;
    memset(&probe, 0, sizeof probe);
    probe.src_end[0] = s->n_src;
    const uint32_t passes = (s->sharded && s->overlap) ? 1 : passes_for(s, probe);
    // lane-split launches walk ONE source range of an unsharded pipeline (one launch = the whole step)
    if (s->sharded || passes != 1 || s->n_src > nb::LANE_SPLIT_MAX_SRC || s->n_src == 0) want.lanes = 1;   // never, not "auto"
    nb::LaunchShape sh = nb::choose_shape(want, s->n_real, (s->n_src + passes - 1) / passes, g_dev.compute_units);
    NB_ASSERT(nb::step_kernel_fn(sh) != nullptr, "no step kernel for k=%d w=%d variant=%d", sh.k, sh.w, sh.variant);
    if (sh.split > 1 && s->n_real > 0 && s->parts.grown(s->stream, (size_t)sh.split * s->n_real)) {
        if (!s->tickets) {
            s->tickets.alloc((size_t)s->n_real / 64 + 2);
            zero_tickets(s);
            ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after zeroing the tickets");
        }
        for (auto &g : s->graphs) destroy_graph(g);  // cached nodes point at the old buffer
        s->graphs.clear();
    }
    s->last_shape = sh;
    s->last_groups = nb::step_grid(sh, s->n_real).x * nb::step_grid(sh, s->n_real).y;
    s->last_deal_items = deal_applies(s, sh) ? nb::deal_items(sh, s->n_real) : 0u;
    s->last_deal_extra = s->last_deal_items ? dealt_extra(s, s->last_deal_items) : 0u;
    return sh;
}

// Parameters of the single-kernel step that reads phase `in` and writes phase `in ^ 1`.
nb::StepParams whole_step(const SimPipeline *s, int in, float dt) {
    (void)dt;  // the value travels through device memory (upload_dt), the parameter block only points at it
    nb::StepParams p = nb::plain_step(s->src_pos[in], s->src_gm, s->n_src, s->pos[in], s->pos[in ^ 1], s->vel, s->acc, s->radius,
                                      s->n_real, s->dt_dev, 64);
    if (s->sharded) {
        // slots [0, mass_count) massive, [mass_count, Mc) pads (never computed), [Mc, Mc + zero_count) massless
        p.recv_split = s->plan.mass_count;
        p.recv_gap = s->plan.mass_chunk - s->plan.mass_count;
        p.mirror = s->src_pos[in ^ 1] + (size_t)s->rank * s->plan.mass_chunk;
        p.n_mirror = s->plan.mass_count;
    }
    return p;
}

// Fused finish ("fused_finish" knob): a split step WITHOUT its second, dependent kernel.  The parts of a receiver tile
// are written with agent-scope (sc1) stores; every workgroup then takes a ticket of its tile, and the one that arrives
// last -- all other parts are complete by then: each workgroup waits for its own stores (vmcnt(0)) before it draws --
// reads the parts back with the same scope, adds them in part order exactly like finish_kernel and integrates.  Same
// bits as the two-kernel form (the GPU suite runs green with it forced on; tools/fused_finish_soak.py: 20 000 steps at
// N = 10 000 + 300 random shapes, 0 differences).  What it buys, and from which size on it is the default:
// launch_shape.hip fused_finish_rule.
bool fused_finish_applies(const SimPipeline *s, nb::LaunchShape sh) {
    if (s->fused_finish == 0 || s->sharded || sh.split <= 1 || sh.lanes > 1 || !s->tickets) return false;
    if (nb::step_kernel_fused_fn(sh) == nullptr) return false;   // scalar-cache route, W >= 4
    return s->fused_finish == 1 || nb::fused_finish_rule(s->n_real, s->n_src);
}

// Dealt launches ("deal" knob): the step kernel's workgroups draw their (receiver tile, source part) from one ticket
// counter, and the grid holds a few more workgroups than items, so an XCD that holds a higher clock takes more of a launch
// (kernels.hip dealt_kernel; why and what it buys: DESIGN.md section 3 "Dealt launches").  Same items, same code, same
// finish kernel: the bits of a step do not depend on the knob.  Unsharded steps on the scalar-cache route with sixteen
// waves per workgroup and no fused finish; 1 = whenever the shape allows, 2 = launches of enough rounds
// (launch_shape.hip deal_pays).
bool deal_applies(const SimPipeline *s, nb::LaunchShape sh) {
    if (s->deal == 0 || s->sharded || !s->deal_counter || s->n_real == 0) return false;
    if (sh.variant != nb::VARIANT_SMEM || sh.lanes > 1 || sh.w != 16 || (sh.k != 1 && sh.k != 2)) return false;
    if (nb::dealt_kernel_fn(sh) == nullptr || fused_finish_applies(s, sh)) return false;
    return s->deal == 1 || nb::deal_pays(nb::deal_items(sh, s->n_real), g_dev.compute_units);
}

// workgroups a dealt launch holds on top of its items ("deal_extra" hook: 0 = launch_shape.hip deal_extra)
uint32_t dealt_extra(const SimPipeline *s, uint32_t items) { return s->want_deal_extra > 0 ? (uint32_t)s->want_deal_extra : nb::deal_extra(items); }

dim3 launch_grid(const SimPipeline *s, nb::LaunchShape sh, bool dealt) {
    if (!dealt) return nb::step_grid(sh, s->n_real);
    const uint32_t items = nb::deal_items(sh, s->n_real);
    return dim3(items + dealt_extra(s, items));
}

const void *launch_fn(nb::LaunchShape sh, bool fused, bool dealt) {
    return dealt ? nb::dealt_kernel_fn(sh) : fused ? nb::step_kernel_fused_fn(sh) : nb::step_kernel_fn(sh);
}

nb::StepParams shaped(const SimPipeline *s, nb::StepParams p, nb::LaunchShape sh) {
    p.split = sh.split > 1 ? (uint32_t)sh.split : 1u;
    p.parts = p.split > 1 ? s->parts : nullptr;
    p.tickets = s->tickets;
    if (deal_applies(s, sh)) {
        p.deal = s->deal_counter;
        p.deal_items = nb::deal_items(sh, s->n_real);
    }
    // finer slice granules only for single-range steps (the overlapped sharded step walks two ranges: 64 there)
    p.unit = (sh.unit >= 8 && sh.unit <= 64 && p.src_end[1] == p.src_begin[1]) ? (uint32_t)sh.unit : 64u;
    return p;
}

// Source passes: a step over sources [0, n) can run as P launches over consecutive sub-ranges chained through
// acc[] (STEP_NO_FINALIZE / STEP_ACC_IN).  All workgroups of a pass then stream the same <= ~3 MB of sources, which
// stay resident in each XCD's 4 MiB L2 across the pass's rounds instead of being re-fetched every round.
constexpr size_t L2_SOURCE_BUDGET = 3u << 20;  // bytes of (x, y, G*m) per pass

uint32_t passes_for(const SimPipeline *s, const nb::StepParams &p) {
    if (p.flags != 0 || p.src_end[1] != p.src_begin[1]) return 1;  // only whole, unchained steps are cut up
    const uint32_t n = p.src_end[0] - p.src_begin[0];
    uint32_t want = (uint32_t)s->want_passes;
    if (want == 0) want = (uint32_t)(((size_t)n * 12 + L2_SOURCE_BUDGET - 1) / L2_SOURCE_BUDGET);
    const uint32_t chunks = (n + 63) / 64;
    if (want > chunks) want = chunks;
    return want ? want : 1;
}

// The launches of one step: P passes, each = step kernel (+ finish kernel when the shape is split).
std::vector<nb::StepParams> step_passes(const SimPipeline *s, const nb::StepParams &whole, nb::LaunchShape sh) {
    std::vector<nb::StepParams> out;
    const uint32_t P = passes_for(s, whole);
    const uint32_t lo = whole.src_begin[0], n = whole.src_end[0] - lo;
    const uint32_t per = ((n + 63) / 64 + P - 1) / P * 64;  // whole 64-source chunks per pass
    for (uint32_t q = 0; q < P; q++) {
        nb::StepParams p = shaped(s, whole, sh);
        if (P > 1) {
            p.src_begin[0] = lo + (q * per < n ? q * per : n);
            p.src_end[0] = lo + ((q + 1) * per < n ? (q + 1) * per : n);
            p.flags = (q > 0 ? nb::STEP_ACC_IN : 0u) | (q + 1 < P ? nb::STEP_NO_FINALIZE : 0u);
        }
        out.push_back(p);
    }
    return out;
}

void launch_step(SimPipeline *s, nb::LaunchShape sh, const nb::StepParams &p, hipStream_t st) {
    if (s->n_real == 0) return;  // a rank without receivers still takes part in the gathers
    const bool fused = fused_finish_applies(s, sh), dealt = deal_applies(s, sh);
    for (nb::StepParams &copy : step_passes(s, p, sh)) {
        void *args[] = {&copy};
        ASSERT_HIP(hipLaunchKernel(launch_fn(sh, fused, dealt), launch_grid(s, sh, dealt), nb::step_block(sh), args,
                                   nb::step_lds_bytes(sh, copy.src_end[0] - copy.src_begin[0]), st),
                   "step kernel launch (k=%d w=%d variant=%d split=%d dealt=%d, %u receivers)", sh.k, sh.w, sh.variant, sh.split,
                   (int)dealt, s->n_real);
        if (copy.split > 1 && !fused)
            ASSERT_HIP(hipLaunchKernel(nb::finish_kernel_fn(), nb::finish_grid(s->n_real), nb::finish_block(), args, 0, st),
                       "finish kernel launch (%u receivers, %u parts)", s->n_real, copy.split);
    }
}

// The fused finish counts arrivals per receiver tile and its last arriver puts the ticket back to zero -- which only holds
// while every launch runs to its end.  A launch that ended part-way (a failed graph replay, a device error the caller
// survived) would leave non-zero tickets, and every later step would silently skip that tile's integration: so the tickets
// are re-zeroed, in stream order, whenever a new state is uploaded and before a chain is built.
// The counter of the dealt launches lives by the same rule (its last draw puts it back to zero) and is zeroed with them.
void zero_tickets(SimPipeline *s) {
    if (s->tickets) ASSERT_HIP(hipMemsetAsync(s->tickets, 0, s->tickets.count() * sizeof(uint32_t), s->stream), "zero the tile tickets");
    if (s->deal_counter) ASSERT_HIP(hipMemsetAsync(s->deal_counter, 0, sizeof(uint32_t), s->stream), "zero the deal counter");
}

// The step size of everything enqueued from here on.  Written in stream order, so steps already queued keep theirs.
void upload_dt(SimPipeline *s, float dt) {
    if (s->dt_valid && memcmp(&dt, &s->dt_enqueued, sizeof dt) == 0) return;
    nb::launch_set_scalar(s->stream, s->dt_dev, dt);
    s->dt_enqueued = dt;
    s->dt_valid = true;
    s->dt_uploads++;
}

// ---- single-device chains ------------------------------------------------------------------------------------

void fill_node(hipKernelNodeParams &kp, void **args, const void *fn, dim3 grid, dim3 block, size_t lds_bytes = 0) {
    memset(&kp, 0, sizeof kp);
    kp.func = const_cast<void *>(fn);
    kp.gridDim = grid;
    kp.blockDim = block;
    kp.sharedMemBytes = (unsigned int)lds_bytes;
    kp.kernelParams = args;
    kp.extra = nullptr;
}

// A cached chain, single-device or sharded, is keyed on (length, passes, shape, PHASE): an odd chain length flips the
// ping-pong phase, so a frame loop that asks for the same odd n alternates between two phases -- with the phase in the
// key it gets two instantiated graphs and replays them untouched, instead of re-patching every node of one graph on
// every call.  dt is not part of the key and never forces a rebuild or a patch: the nodes read it from device memory
// (upload_dt).
// Whether the chain's step launches are dealt, and over how many workgroups, is part of the key as well: flipping the "deal"
// knob builds a new chain (other kernel, other grid) and never re-patches one.
StepGraph *find_graph(SimPipeline *s, uint32_t n, uint32_t passes, nb::LaunchShape sh, int phase) {
    const uint32_t dealt_groups = deal_applies(s, sh) ? launch_grid(s, sh, true).x : 0u;
    for (auto &c : s->graphs)
        if (c.n == n && c.passes == passes && c.phase == phase && c.shape == sh && c.dealt_groups == dealt_groups) return &c;
    return nullptr;
}

StepGraph *find_or_build_graph(SimPipeline *s, uint32_t n, float dt, nb::LaunchShape sh) {
    const uint32_t passes = passes_for(s, whole_step(s, s->cur, dt));
    StepGraph *g = find_graph(s, n, passes, sh, s->cur);
    const bool fused = fused_finish_applies(s, sh), dealt = deal_applies(s, sh);
    const uint32_t per_pass = sh.split > 1 && !fused ? 2 : 1;  // step kernel (+ finish kernel)
    const uint32_t per_step = passes * per_pass;
    const bool fresh = g == nullptr;
    if (fresh) {
        evict_for_one_more(s);
        s->graphs.emplace_back();
        g = &s->graphs.back();
        g->n = n;
        g->passes = passes;
        g->shape = sh;
        g->dealt_groups = dealt ? launch_grid(s, sh, true).x : 0u;
        ASSERT_HIP(hipGraphCreate(&g->graph, 0), "hipGraphCreate");
        g->nodes.resize((size_t)n * per_step);
        g->params.resize((size_t)n * passes);
    }
    g->last_use = ++s->use_clock;
    if (!fresh) return g;
    if (fused || dealt) zero_tickets(s);
    hipGraphNode_t prev = nullptr;
    for (uint32_t i = 0; i < n; i++) {
        const std::vector<nb::StepParams> launches = step_passes(s, whole_step(s, (s->cur + i) & 1, dt), sh);
        for (uint32_t q = 0; q < passes; q++) {
            g->params[(size_t)i * passes + q] = launches[q];
            void *args[] = {&g->params[(size_t)i * passes + q]};
            for (uint32_t j = 0; j < per_pass; j++) {
                hipKernelNodeParams kp;
                if (j == 0)
                    fill_node(kp, args, launch_fn(sh, fused, dealt), launch_grid(s, sh, dealt), nb::step_block(sh),
                              nb::step_lds_bytes(sh, launches[q].src_end[0] - launches[q].src_begin[0]));
                else
                    fill_node(kp, args, nb::finish_kernel_fn(), nb::finish_grid(s->n_real), nb::finish_block());
                hipGraphNode_t &node = g->nodes[(size_t)i * per_step + q * per_pass + j];
                ASSERT_HIP(hipGraphAddKernelNode(&node, g->graph, prev ? &prev : nullptr, prev ? 1 : 0, &kp),
                           "hipGraphAddKernelNode step %u/%u", i, n);
                prev = node;
            }
        }
    }
    ASSERT_HIP(hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0), "hipGraphInstantiate (%u steps)", n);
    g->phase = s->cur;
    return g;
}

// graph = 2 (auto) on small worlds: ONE canonical chain of CANON_STEPS steps starting at phase 0, built when the data
// first reaches the device (outside any step call) and replayed by every call of 32+ steps: one plain step if needed
// to reach phase 0, whole replays (even length: the phase stays 0), the remainder as plain launches.  A replayed node
// is a little cheaper than a plain launch while steps are short -- the first 100-step call of a fresh pipeline runs
// 4.56 vs 4.71 us per step at N = 250, 5.00 vs 5.11 at 1 000, 7.29 vs 7.53 at 4 000, 20.7 vs 20.9 at 10 000, and
// slightly SLOWER at 20 000 (50.0 vs 48.4): profiles/r02_first_call_probe.txt -- and building the 32-step chain costs
// 95-150 us once (profiles/r02_graph_chunk_probe.txt), which a one-off call could never win back.  Prebuilt, the
// reference's nbody-bench -- ONE 100-step call per world (bench.c:30-33) -- runs 96 of its 100 steps at the replay rate.
constexpr double CANON_MAX_PAIRS = 6.0e7;  // N x M up to which a replay still pays (N ~ 11 000 with galaxy.h ICs)

// A world that fits one workgroup runs its chains inside ONE launch (kernels.hip chain_kernel).  "fused_chain" = 2
// (auto): only while a step is cheaper on one compute unit than the kernel boundary it saves -- N <= 256 (two receiver
// tiles of eight waves each; with four tiles a wave's source slice is 2.5x longer) and N x M <= 3.6e4.  Measured
// (profiles/r03_fused_chain.txt): 2.25 us per step at N = 200 / 250 against 3.1 as per-step launches, but 4.95 against
// 3.4 at N = 300 and 7.6 against 3.7 at N = 512 -- one CU runs the interaction body at ~63 % of its issue rate with four
// latency-bound waves per SIMD.  For calls of two steps or more, and only with the launch shape left on auto (an explicit k / w / split / unit / passes asks for the
// per-step kernel).  1 = whenever the world fits (N <= 512), whatever the other knobs say; 0 = never.
constexpr double CHAIN_MAX_PAIRS = 3.6e4;
constexpr uint32_t CHAIN_AUTO_MAX_RECV = 256;

bool wants_fused_chain(const SimPipeline *s) {
    if (s->sharded || s->fused_chain == 0 || s->n_real == 0 || nb::chain_tiles(s->n_real) == 0) return false;
    if (s->fused_chain == 1) return true;
    // an explicit shape, route or passes asks for the per-step kernel
    return nb::shape_on_auto(s->want) && s->want_passes == 0 && s->n_real <= CHAIN_AUTO_MAX_RECV &&
           (double)s->n_real * (double)(s->n_src ? s->n_src : 1) <= CHAIN_MAX_PAIRS;
}

void enqueue_fused(SimPipeline *s, uint32_t n) {
    nb::ChainParams p;
    memset(&p, 0, sizeof p);
    p.pos = s->pos[s->cur];   // updated in place: the ping-pong phase does not move
    p.vel = s->vel;
    p.acc = s->acc;
    p.radius = s->radius;
    p.src_gm = s->src_gm;
    p.n_recv = s->n_real;
    p.n_src = s->n_src;
    p.tiles = nb::chain_tiles(s->n_real);
    p.dt = s->dt_dev;
    for (uint32_t left = n; left > 0;) {
        p.steps = left > CHAIN_MAX_STEPS_PER_LAUNCH ? CHAIN_MAX_STEPS_PER_LAUNCH : left;
        nb::launch_chain(s->stream, p);
        left -= p.steps;
    }
    s->fused_steps = n;
    // the per-step shape it is bit-equal to
    s->last_shape = {.k = 2, .w = (int)(16u / p.tiles), .variant = nb::VARIANT_LDS, .split = 1, .unit = 8, .lanes = 1};
    s->last_groups = 1;
}

bool wants_canonical(const SimPipeline *s) {
    if (s->fused_chain == 2 && wants_fused_chain(s)) return false;   // its chains never reach the graph path
    return !s->sharded && s->use_graph == 2 && s->n_real > 0 &&
           (double)s->n_real * (double)(s->n_src ? s->n_src : 1) <= CANON_MAX_PAIRS;
}

void enqueue_single(SimPipeline *s, uint32_t n, float dt) {
    if (n >= 2 && wants_fused_chain(s)) {
        enqueue_fused(s, n);
        return;
    }
    const nb::LaunchShape sh = resolve_shape(s);
    if (!s->use_graph || n == 1 || (s->use_graph == 2 && n < GRAPH_AUTO_MIN_CHAIN)) {
        for (uint32_t i = 0; i < n; i++) {
            launch_step(s, sh, whole_step(s, s->cur, dt), s->stream);
            s->cur ^= 1;
        }
        return;
    }
    uint32_t left = n;
    if (wants_canonical(s)) {
        if (s->cur == 1 && left > 0) {  // reach phase 0
            launch_step(s, sh, whole_step(s, s->cur, dt), s->stream);
            s->cur ^= 1;
            left--;
        }
        while (left >= CANON_STEPS) {
            StepGraph *g = find_or_build_graph(s, CANON_STEPS, dt, sh);  // prebuilt at SetSimulationData unless a knob moved
            ASSERT_HIP(hipGraphLaunch(g->exec, s->stream), "hipGraphLaunch (canonical %u steps)", CANON_STEPS);
            left -= CANON_STEPS;
        }
        for (; left > 0; left--) {
            launch_step(s, sh, whole_step(s, s->cur, dt), s->stream);
            s->cur ^= 1;
        }
        return;
    }
    while (left > 0) {
        // full chains have even length so that replaying them keeps the ping-pong phase
        const uint32_t chunk = left > GRAPH_CHAIN_MAX ? GRAPH_CHAIN_MAX : left;
        if (s->use_graph == 2 && !find_graph(s, chunk, passes_for(s, whole_step(s, s->cur, dt)), sh, s->cur)) {
            // Building and instantiating a chain costs ~3 us per node, more than it saves in one run (a graph
            // replay saves 1-2 us per step below N ~ 10 000 and nothing above: profiles/r01_graph_build_vs_replay.txt).
            // A caller that steps the same n again and again -- a frame loop -- gets the graph from its second
            // call; a one-off call (the reference's nbody-bench times exactly one) never pays for it.
            bool seen = false;
            for (uint32_t c : s->seen_chains) seen = seen || c == chunk;
            if (!seen) {
                if (s->seen_chains.size() >= 64) s->seen_chains.clear();
                s->seen_chains.push_back(chunk);
                for (uint32_t i = 0; i < chunk; i++) {
                    launch_step(s, sh, whole_step(s, s->cur, dt), s->stream);
                    s->cur ^= 1;
                }
                left -= chunk;
                continue;
            }
        }
        StepGraph *g = find_or_build_graph(s, chunk, dt, sh);
        ASSERT_HIP(hipGraphLaunch(g->exec, s->stream), "hipGraphLaunch (%u steps)", chunk);
        if (chunk & 1) s->cur ^= 1;
        left -= chunk;
    }
}

// ---- what every step call starts and ends with ---------------------------------------------------------------------

void begin_call(SimPipeline *s) {
    s->pool.used = 0;
    s->kernel_iv.clear();
    s->comm_iv.clear();
    s->detail_steps = 0;
    s->fused_steps = 0;
    s->host_current = false;
}

void end_call(SimPipeline *s, uint32_t launches) {
    if (s->timing)
        s->step_iv.end(s->stream);
    else
        s->step_iv.clear();
    s->timed_launches = launches;
    s->timed_finish_launches = s->last_shape.split > 1 && !fused_finish_applies(s, s->last_shape) ? s->timed_launches : 0;
}

void enqueue_steps(SimPipeline *s, uint32_t n, float dt) {
    NB_ASSERT(s->on_device, "PerformSimUpdate before SetSimulationData");
    if (s->slots == 0 || n == 0) return;
    use_device();
    begin_call(s);
    s->acc_current = false;   // an Euler step leaves the acc of the state before it
    upload_dt(s, dt);
    if (s->timing) s->step_iv.begin(s->stream);
    if (!s->sharded)
        enqueue_single(s, n, dt);
    else
        enqueue_sharded(s, n, dt);
    uint32_t launches = (s->sharded && s->overlap) ? 2 * n : n * passes_for(s, whole_step(s, s->cur, dt));
    if (s->fused_steps) launches = (n + CHAIN_MAX_STEPS_PER_LAUNCH - 1) / CHAIN_MAX_STEPS_PER_LAUNCH;
    end_call(s, launches);
    s->data.dt = dt;
}

}  // namespace nbi
