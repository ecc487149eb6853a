// batch.hip -- SimBatch: an ensemble of B independent worlds with the same particle count, stepped together
// (include/nbody_hip.h "World ensembles").
//
// One small world cannot use the chip: below N ~ 4 000 a step is the kernel boundary plus one wave's dependency chain, and
// the one-workgroup chain sits on ONE of 256 compute units.  The other CUs can only be used by more
// worlds, so this file steps B of them per launch:
//   N <= 512          batch_chain_kernel: workgroup b runs member b's whole n-step call (positions ping-pong in LDS), one
//                     launch per call, for every call length and every B;
//   512 < N <= 3 000  batch_lane_split_kernel<W, H>: gridDim.y = B, one launch per step, positions ping-pong between two
//                     device arrays; (W, H) = lane_split_rule(N, N), a function of N alone.
// A traced update (nb_hip_ensemble_trace) records every member's energy sums every k steps without returning to the host:
// on the chain path batch_trace_chain_kernel records from the state it holds in LDS (still one launch per call), on the
// lane-split path the two diagnostics launches are interleaved with the step launches; one copy and one sync at the end.
// Adaptive and leapfrog updates run step_schedule.h's one launch schedule with every member as its target.  The read-only
// calls (energy, potential, bounds, renders) are batch_observe.hip.
// The path is chosen by N alone -- never by B or by the members' source counts -- and the kernels run the very bodies of
// chain_kernel / lane_split_kernel, so member b's bits are those of the same particles alone in a SimPipeline pinned to
// that shape (tests/test_gpu_batch.py).  Members share nothing with each other and a SimBatch shares nothing with any
// SimPipeline: own stream, own buffers, own events.
//
// A RAGGED ensemble (nb_hip_ragged_create) is the same SimBatch with a particle count per member.  The SoA arrays keep one
// stride (the largest member rounded up to 64 rows), the AoS side of the seam is packed (member b at offsets[b]), and the
// members fall into up to three launch GROUPS by their own size alone -- chain (N <= 512), lane-split (8, 8), lane-split
// (16, 4) -- each with a device list of its member indices: one chain launch per call and one lane-split launch per group
// and step (the same kernels instantiated for RaggedParams: the receiver count read per member).  Member b's bits are
// those of the same particles as the only member of a uniform SimBatch of its size.
// The host has ONE representation and ONE launch walk for both: create() below makes every SimBatch with its groups -- a
// uniform one has exactly one, of all members, without a device list -- and every fixed Euler step goes through
// ensemble_walk.h's walk_ensemble with StepTarget as its target, so a uniform SimBatch launches exactly what it launched
// before ragged ones existed.  How a launch finds its members (by block index, or through n_len and the lists) is decided
// on the device side of the seam (kernels.h, convert.h, batch_diag.h): every launch here hands over the tables, which a
// uniform ensemble does not have.  `ragged` itself is read by materialize's upload of those tables, by create()'s lookup of
// the lane-split kernel, by StepTarget::copy's assertion, and by the calls that are not wired for ragged ensembles.
#include "batch_internal.h"
#include "diag_sums.h"
#include "ensemble_walk.h"
#include "leapfrog.h"
#include "nbody_hip_tuning.h"
#include "step_schedule.h"
#include "timestep.h"

using namespace nbi;

namespace {

void materialize(SimBatch *s) {
    use_device();
    if (s->on_device) return;
    ASSERT_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "stream");
    const size_t rows = (size_t)s->count * s->stride;
    for (int b = 0; b < 2; b++) {
        if (b == 1 && !s->lane_split()) break;   // the chain updates positions in place
        s->pos[b].alloc(rows);
        ASSERT_HIP(hipMemsetAsync(s->pos[b], 0, rows * sizeof(float2), s->stream), "clear positions");
    }
    s->vel.alloc(rows);
    s->acc.alloc(rows);
    s->radius.alloc(rows);
    s->mass.alloc(rows);
    s->gm.alloc(rows);
    s->mass_len_dev.alloc(s->count);
    s->dt_dev.alloc(s->count);
    s->aos.alloc((size_t)s->offsets[s->count]);
    if (s->ragged) {
        // pad rows stay zero for the life of the ensemble: no kernel writes a row at or beyond n_len[b]
        ASSERT_HIP(hipMemsetAsync(s->vel, 0, rows * sizeof(float2), s->stream), "clear velocities");
        ASSERT_HIP(hipMemsetAsync(s->acc, 0, rows * sizeof(float2), s->stream), "clear accelerations");
        ASSERT_HIP(hipMemsetAsync(s->radius, 0, rows * sizeof(float), s->stream), "clear radii");
        ASSERT_HIP(hipMemsetAsync(s->mass, 0, rows * sizeof(float), s->stream), "clear masses");
        ASSERT_HIP(hipMemsetAsync(s->gm, 0, rows * sizeof(float), s->stream), "clear G*m");
        s->n_len_dev.alloc(s->count);
        s->offsets_dev.alloc((size_t)s->count + 1);
        ASSERT_HIP(hipMemcpyAsync(s->n_len_dev, s->n_len.data(), (size_t)s->count * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream),
                   "H2D of %u member sizes", s->count);
        ASSERT_HIP(hipMemcpyAsync(s->offsets_dev, s->offsets.data(), ((size_t)s->count + 1) * sizeof(uint64_t), hipMemcpyHostToDevice,
                                  s->stream),
                   "H2D of %u member offsets", s->count);
        for (auto &g : s->groups) {
            g.list.alloc(g.members.size());
            ASSERT_HIP(hipMemcpyAsync(g.list, g.members.data(), g.members.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream),
                       "H2D of a launch group's %zu members", g.members.size());
        }
    }
    ASSERT_HIP(hipMemcpyAsync(s->mass_len_dev, s->mass_len.data(), (size_t)s->count * sizeof(uint32_t), hipMemcpyHostToDevice,
                              s->stream),
               "H2D of %u source counts", s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after the first device set-up");
    s->on_device = true;
}

// The step sizes of everything enqueued from here on; uploaded only when a value changed.  One dt for all: a fill
// launch in stream order.  Per-member values: the stream is drained first, so steps already queued keep theirs.
void upload_dts(SimBatch *s, const float *dt, bool uniform) {
    bool same = s->dt_valid;
    for (uint32_t b = 0; same && b < s->count; b++) {
        const float v = uniform ? dt[0] : dt[b];
        same = memcmp(&v, &s->dt_host[b], sizeof v) == 0;
    }
    if (same) return;
    for (uint32_t b = 0; b < s->count; b++) s->dt_host[b] = uniform ? dt[0] : dt[b];
    if (uniform) {
        nb::launch_batch_fill(s->stream, s->dt_dev, s->count, dt[0]);
    } else {
        ASSERT_HIP(hipStreamSynchronize(s->stream), "sync before a per-member step-size upload");
        ASSERT_HIP(hipMemcpy(s->dt_dev, s->dt_host.data(), (size_t)s->count * sizeof(float), hipMemcpyHostToDevice),
                   "H2D of %u step sizes", s->count);
    }
    s->dt_valid = true;
    s->dt_uploads++;
}

nb::BatchParams step_params(const SimBatch *s) {
    nb::BatchParams p;
    memset(&p, 0, sizeof p);
    p.vel = s->vel;
    p.acc = s->acc;
    p.radius = s->radius;
    p.gm = s->gm;
    p.mass_len = s->mass_len_dev;
    p.dt = s->dt_dev;
    p.n_recv = s->n;
    p.stride = s->stride;
    return p;
}

// What the launches of walk_ensemble are.  Every launch gets the full block: the BatchParams, the member sizes and the
// group's list -- the last two null in a uniform ensemble, whose kernels read only the BatchParams at its head.
struct StepTarget {
    SimBatch *s;
    nb::BatchParams p;   // step_params(s)

    nb::RaggedParams params(const SimBatch::Group &g, int in, int out, uint32_t steps) const {
        nb::RaggedParams rp = {p, s->n_len_dev, g.list};
        rp.pos_in = s->pos[in];
        rp.pos_out = s->pos[out];
        rp.steps = steps;
        rp.tiles = g.tiles;
        return rp;
    }
    void lanes(const SimBatch::Group &g, int in) {
        nb::RaggedParams rp = params(g, in, in ^ 1, 0);
        void *args[] = {&rp};   // g.fn takes the whole of it or its head
        ASSERT_HIP(hipLaunchKernel(g.fn, g.grid, g.block, args, g.lds, s->stream),
                   "ensemble lane-split launch (w=%d lanes=%d, %zu members of up to %u)", g.w, g.lanes, g.members.size(), g.max_n);
    }
    void chain(const SimBatch::Group &g, int buf, uint32_t steps) {
        nb::launch_batch_chain(s->stream, params(g, buf, buf, steps), (uint32_t)g.members.size());
    }
    void copy(const SimBatch::Group &g, int from, int to) {
        NB_ASSERT(s->ragged, "a uniform ensemble is one group: its chain never meets a phase that moved");
        nb::launch_ragged_copy_rows(s->stream, g.list, s->n_len_dev, (uint32_t)g.members.size(), g.max_n, s->stride, s->pos[from],
                                    s->pos[to]);
    }
};

// The chain that records from the state it holds in LDS: t.done carries the record index across the launches of a call.
struct TraceTarget : StepTarget {
    nb::TraceParams t;

    void chain(const SimBatch::Group &g, int buf, uint32_t steps) {
        nb::launch_batch_trace_chain(s->stream, params(g, buf, buf, steps), t, (uint32_t)g.members.size());
        t.done += steps;
    }
};

// n steps, no record; returns the launches made
uint32_t launch_steps(SimBatch *s, const nb::BatchParams &p, uint32_t n) {
    StepTarget target = {s, p};
    return walk_ensemble(target, s->groups, s->cur, n, CHAIN_MAX_STEPS_PER_LAUNCH);
}

// the seam's converters: staged AoS records -> SoA rows of buffer 0 and G*m; the latest rows -> AoS records (the offsets
// and member sizes on the device are null in a uniform ensemble, like the lists)
void split_members(SimBatch *s) {
    nb::launch_batch_split(s->stream, s->aos, s->offsets_dev, s->n_len_dev, s->mass_len_dev, s->count, s->n, s->stride, s->pos[0], s->vel,
                           s->acc, s->radius, s->mass, s->gm, NB_G);
}

void merge_members(SimBatch *s, uint32_t first, uint32_t members) {
    nb::launch_batch_merge(s->stream, s->aos, s->offsets_dev, s->n_len_dev, first, members, s->n, s->stride, s->pos[s->cur], s->vel, s->acc,
                           s->radius, s->mass);
}

void enqueue(SimBatch *s, uint32_t n, const float *dt, bool uniform) {
    NB_ASSERT(s != nullptr && dt != nullptr, "NULL argument");
    NB_ASSERT(s->has_data, "ensemble update before nb_hip_batch_set_data");
    if (n == 0) return;
    use_device();
    s->acc_current = false;   // an Euler step leaves the acc of the state before it
    upload_dts(s, dt, uniform);
    nb::BatchParams p = step_params(s);
    s->step_iv.begin(s->stream);
    launch_steps(s, p, n);
    ASSERT_HIP(hipGetLastError(), "ensemble launch (%u members of %u particles, %u steps)", s->count, s->n, n);
    s->step_iv.end(s->stream);
}

// ---- device-chosen and leapfrog steps: every member as the target of step_schedule.h's schedule --------------------------

// the step sizes of the kick / drift passes, [2][count]
float *kick_words(SimBatch *s) {
    if (!s->lf_dt) s->lf_dt.alloc(2 * (size_t)s->count);
    return s->lf_dt;
}

// The step words are dt_dev[count], read by the launches of a one-step update; the kick words are the two rows of lf_dt.
struct BatchTarget {
    SimBatch *s;
    nb::BatchParams p;
    nb::TimestepParams t;   // adaptive calls only
    float *log;             // [n][count] on the device, or null
    uint32_t forces = 0;

    bool acc_current() const { return s->acc_current; }
    void zero_step_word() {
        const float zero = 0.0f;
        upload_dts(s, &zero, true);
    }
    void force() {
        launch_steps(s, p, 1);
        forces++;
    }
    void criterion(uint32_t i, int row) {   // one workgroup per member writes dt[b]
        t.log = log ? log + (size_t)i * s->count : nullptr;
        t.dt_out = row < 0 ? s->dt_dev : s->lf_dt + (size_t)row * s->count;
        nb::launch_ensemble_timestep(s->stream, t, s->count);
    }
    // one pass over every member: close with row `close_row` of lf_dt, open (kick + drift of the latest positions) with `open_row`
    void kicks(bool close, bool open, uint32_t close_row, uint32_t open_row) {
        nb::LeapfrogParams lf;
        memset(&lf, 0, sizeof lf);
        lf.pos = s->pos[s->cur];
        lf.vel = s->vel;
        lf.acc = s->acc;
        lf.dt_close = s->lf_dt + (size_t)close_row * s->count;
        lf.dt_open = s->lf_dt + (size_t)open_row * s->count;
        lf.n = s->n;
        lf.stride = s->stride;
        nb::launch_leapfrog(s->stream, lf, close, open, s->count);
    }
    void begin_mark() { s->step_iv.begin(s->stream); }
    void end_mark() {
        ASSERT_HIP(hipGetLastError(), "ensemble step launches (%u members of %u particles)", s->count, s->n);
        s->step_iv.end(s->stream);
    }
};

// One call of the schedule and every record it leaves: the only place these fields are set for a device-chosen or leapfrog call.
void run_call(SimBatch *s, Schedule c, const nb::TimestepParams &t, float *log) {
    BatchTarget target = {s, step_params(s), t, log};
    if (c.leapfrog) {
        kick_words(s);
        s->lf_primed = !s->acc_current;
    }
    run_schedule(target, c);
    if (c.leapfrog) s->lf_force_launches = target.forces;
    s->dt_valid = false;            // dt_dev holds 0 or the device's choices: the next fixed-step update uploads its own afresh
    s->acc_current = c.leapfrog;    // Euler steps leave the acc of the state before them
}

// n kick-drift-kick steps, every member with its own step size
void enqueue_leapfrog(SimBatch *s, uint32_t n, const float *dt, bool uniform, const char *what) {
    NB_ASSERT(s != nullptr && dt != nullptr, "%s: NULL argument", what);
    NB_ASSERT(!s->ragged, "%s: leapfrog steps of ragged ensembles (members of different sizes) are not supported", what);
    if (n == 0) return;
    NB_ASSERT(s->has_data, "%s before nb_hip_batch_set_data", what);
    use_device();
    if (uniform) {
        nb::launch_batch_fill(s->stream, kick_words(s), s->count, dt[0]);
    } else {   // before anything of this call is queued: the blocking copy drains what earlier calls left, not this one
        ASSERT_HIP(hipStreamSynchronize(s->stream), "sync before a per-member step-size upload");
        ASSERT_HIP(hipMemcpy(kick_words(s), dt, (size_t)s->count * sizeof(float), hipMemcpyHostToDevice), "H2D of %u step sizes", s->count);
    }
    run_call(s, {n, true, false, false}, nb::TimestepParams{}, nullptr);
}

void read_back(SimBatch *s, uint32_t first, uint32_t members, Particle *ps) {
    NB_ASSERT(s != nullptr && ps != nullptr, "NULL argument");
    NB_ASSERT(s->has_data, "ensemble read-back before nb_hip_batch_set_data");
    use_device();
    merge_members(s, first, members);
    ASSERT_HIP(hipMemcpyAsync(ps, s->aos + s->offsets[first],
                              (size_t)(s->offsets[first + members] - s->offsets[first]) * sizeof(Particle), hipMemcpyDeviceToHost,
                              s->stream),
               "D2H of %u members", members);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after an ensemble read-back");
}

constexpr uint64_t TRACE_MAX_ROWS = 1ull << 24;   // rows of 64 bytes: 1 GiB

// nb_hip_ensemble_trace / _dts: the n steps of enqueue() with a record of every member's sums before the first and after
// every `every`-th, all in stream order; then one copy, one sync.
void trace(SimBatch *s, uint32_t n, const float *dt, bool uniform, uint32_t every, WorldEnergy *out) {
    NB_ASSERT(s != nullptr && dt != nullptr && out != nullptr, "NULL argument");
    NB_ASSERT(every > 0, "every = 0: a traced update records every k >= 1 steps");
    NB_ASSERT((1ull + n / every) * s->count <= TRACE_MAX_ROWS, "%llu records x %u members > %llu rows (1 GiB of energy rows)",
              1ull + n / every, s->count, (unsigned long long)TRACE_MAX_ROWS);
    const uint32_t records = nb_hip_ensemble_trace_rows(n, every);
    NB_ASSERT(s->has_data, "traced ensemble update before nb_hip_batch_set_data");
    use_device();
    if (n > 0) {
        upload_dts(s, dt, uniform);
        s->acc_current = false;   // Euler steps leave the acc of the state before them
    }
    constexpr size_t Q = NB_DIAG_SUMS;
    const size_t pitch = (size_t)s->count * Q;
    s->trace.grown(s->stream, (size_t)records * pitch);
    double *rows = s->trace;
    const bool fused = !s->lane_split() && s->trace_mode == 0;   // every member is in the one chain group
    if (!fused) energy_slab(s);
    const nb::BatchParams p = step_params(s);
    uint32_t launches = 0;
    s->step_iv.begin(s->stream);
    if (fused) {
        TraceTarget target = {{s, p}, {.mass = s->mass, .rows = rows, .count = s->count, .every = every}};
        if (n == 0) target.chain(s->groups[0], s->cur, 0);   // one launch of no steps: the record on entry
        launches = n == 0 ? 1 : walk_ensemble(target, s->groups, s->cur, n, CHAIN_MAX_STEPS_PER_LAUNCH);
    } else {
        launch_energy_sums(s, rows);
        launches += 2;
        for (uint32_t r = 1; r < records; r++) {
            launches += launch_steps(s, p, every);
            launch_energy_sums(s, rows + r * pitch);
            launches += 2;
        }
        launches += launch_steps(s, p, n % every);
    }
    ASSERT_HIP(hipGetLastError(), "traced ensemble launch (%u members of %u particles, %u steps, a record every %u)", s->count, s->n,
               n, every);
    s->step_iv.end(s->stream);
    s->trace_fused = fused;
    s->trace_launches = launches;
    s->trace_host.resize((size_t)records * pitch);
    ASSERT_HIP(hipMemcpyAsync(s->trace_host.data(), rows, (size_t)records * pitch * sizeof(double), hipMemcpyDeviceToHost, s->stream),
               "D2H of %u x %u energy rows", records, s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after a traced ensemble update");
    for (size_t i = 0; i < (size_t)records * s->count; i++) nb_energy_from_sums(s->trace_host.data() + i * Q, out + i);
}

// The launch shape of a member of n particles, a function of n alone: the chain while it fits (k = 2, 16 waves over its
// tiles), the lane-split shape above that.  slot: 0 chain, 1 lane-split (8, 8), 2 lane-split (16, 4).
struct MemberShape { int slot, k, w, lanes; };
MemberShape member_shape(uint32_t n) {
    if (const uint32_t tiles = nb::chain_tiles(n)) return {0, 2, (int)(16u / tiles), 1};
    int w = 16;
    const int lanes = nb::batch_lane_shape(n, &w);
    return {lanes == 8 ? 1 : 2, 1, w, lanes};
}

// Every SimBatch is made here, from the checked sizes its entry point put into n_len: offsets, stride, and the groups with
// all that their launches need.
SimBatch *create(SimBatch *s, const uint32_t *mass_len, bool ragged) {
    const uint32_t count = (uint32_t)s->n_len.size();
    s->ragged = ragged;
    s->count = count;
    s->mass_len.assign(mass_len, mass_len + count);
    s->dt_host.assign(count, 0.0f);
    s->offsets.resize((size_t)count + 1);   // offsets[0] = 0
    SimBatch::Group slot[3];
    for (uint32_t b = 0; b < count; b++) {
        const uint32_t n = s->n_len[b];
        s->offsets[b + 1] = s->offsets[b] + n;
        s->n = n > s->n ? n : s->n;
        const MemberShape m = member_shape(n);
        SimBatch::Group &g = slot[m.slot];
        g.path = m.slot != 0;
        g.k = m.k;
        g.lanes = m.lanes;
        if (n > g.max_n) {   // chain: w of the group's largest member
            g.max_n = n;
            g.w = m.w;
        }
        g.members.push_back(b);
    }
    s->stride = round_up(s->n, 64);
    for (auto &g : slot) {
        if (g.members.empty()) continue;
        g.tiles = nb::chain_tiles(g.max_n);
        g.workgroups = (uint32_t)g.members.size();
        if (g.path) {
            const nb::LaunchShape sh = {.k = 1, .w = g.w, .variant = nb::VARIANT_LDS, .split = 1, .unit = 8, .lanes = g.lanes};
            g.fn = nb::batch_lane_split_fn(g.w, g.lanes, ragged);
            NB_ASSERT(g.lanes > 1 && g.fn != nullptr, "no ensemble kernel for w=%d lanes=%d", g.w, g.lanes);
            g.grid = nb::step_grid(sh, g.max_n);
            g.workgroups *= g.grid.x;
            g.grid.y = (uint32_t)g.members.size();
            g.block = nb::step_block(sh);
            g.lds = nb::step_lds_bytes(sh, g.max_n);
        }
        s->groups.push_back(std::move(g));
    }
    return s;
}

}  // namespace

extern "C" {

SimBatch *nb_hip_batch_create(uint32_t count, uint32_t total_len, const uint32_t *mass_len) {
    NB_ASSERT(count > 0, "an ensemble needs at least one member (count = 0)");
    NB_ASSERT(count <= NB_HIP_BATCH_MAX_COUNT, "count %u > %u members (the grid's y extent)", count, NB_HIP_BATCH_MAX_COUNT);
    NB_ASSERT(total_len > 0, "total_len = 0: an ensemble of empty worlds");
    NB_ASSERT(total_len <= nb::BATCH_MAX_RECV, "total_len %u > %u: ensembles step worlds of at most %u particles", total_len,
              nb::BATCH_MAX_RECV, nb::BATCH_MAX_RECV);
    NB_ASSERT(mass_len != nullptr, "NULL mass_len array");
    for (uint32_t b = 0; b < count; b++)
        NB_ASSERT(mass_len[b] <= total_len, "member %u: mass_len %u > total_len %u", b, mass_len[b], total_len);
    SimBatch *s = new SimBatch();
    s->n_len.assign(count, total_len);
    return create(s, mass_len, false);
}

SimBatch *nb_hip_ragged_create(uint32_t count, const uint32_t *total_len, const uint32_t *mass_len) {
    NB_ASSERT(count > 0, "an ensemble needs at least one member (count = 0)");
    NB_ASSERT(count <= NB_HIP_BATCH_MAX_COUNT, "count %u > %u members (the grid's y extent)", count, NB_HIP_BATCH_MAX_COUNT);
    NB_ASSERT(total_len != nullptr && mass_len != nullptr, "NULL total_len or mass_len array");
    for (uint32_t b = 0; b < count; b++) {
        NB_ASSERT(total_len[b] > 0, "member %u: total_len = 0: an empty world", b);
        NB_ASSERT(total_len[b] <= nb::BATCH_MAX_RECV, "member %u: total_len %u > %u: ensembles step worlds of at most %u particles", b,
                  total_len[b], nb::BATCH_MAX_RECV, nb::BATCH_MAX_RECV);
        NB_ASSERT(mass_len[b] <= total_len[b], "member %u: mass_len %u > total_len %u", b, mass_len[b], total_len[b]);
    }
    SimBatch *s = new SimBatch();
    s->n_len.assign(total_len, total_len + count);
    return create(s, mass_len, true);
}

void nb_hip_ragged_layout(const SimBatch *s, uint32_t *sizes, uint64_t *offsets) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (sizes) memcpy(sizes, s->n_len.data(), (size_t)s->count * sizeof(uint32_t));
    if (offsets) memcpy(offsets, s->offsets.data(), ((size_t)s->count + 1) * sizeof(uint64_t));
}

uint32_t nb_hip_ragged_launch_shape(const SimBatch *s, uint32_t group, int *path, int *k, int *w, int *lanes, uint32_t *members,
                                    uint32_t *workgroups) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    const uint32_t groups = (uint32_t)s->groups.size();
    NB_ASSERT(group < groups, "launch group %u of %u", group, groups);
    const SimBatch::Group &g = s->groups[group];
    if (path) *path = g.path;
    if (k) *k = g.k;
    if (w) *w = g.w;
    if (lanes) *lanes = g.lanes;
    if (members) *members = (uint32_t)g.members.size();
    if (workgroups) *workgroups = g.workgroups;
    return groups;
}

void nb_hip_ragged_member_shape(const SimBatch *s, uint32_t member, uint32_t *group, int *k, int *w, int *lanes) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    NB_ASSERT(member < s->count, "member %u of %u", member, s->count);
    const MemberShape m = member_shape(s->n_len[member]);
    uint32_t gi = 0;   // the lanes tell the groups apart: 1, 8, 4
    for (uint32_t i = 0; i < s->groups.size(); i++)
        if (s->groups[i].lanes == m.lanes) gi = i;
    if (group) *group = gi;
    if (k) *k = m.k;
    if (w) *w = m.w;
    if (lanes) *lanes = m.lanes;
}

void nb_hip_batch_destroy(SimBatch *s) {
    if (s == nullptr) return;
    if (s->on_device) {
        use_device();
        ASSERT_HIP(hipStreamSynchronize(s->stream), "sync before destroying an ensemble");
        ASSERT_HIP(hipStreamDestroy(s->stream), "stream");
    }
    delete s;   // its device arrays and events go with their owners
}

void nb_hip_batch_set_data(SimBatch *s, const Particle *ps) {
    NB_ASSERT(s != nullptr && ps != nullptr, "NULL argument");
    if (!s->on_device) {
        // first touch: stream, HBM, code objects -- none of it may move the caller's rand() stream
        RandGuard keep_callers_rand_stream;
        materialize(s);
    }
    use_device();
    s->cur = 0;
    s->acc_current = false;   // the uploaded acc is the caller's: a leapfrog call evaluates its own first
    ASSERT_HIP(hipMemcpyAsync(s->aos, ps, (size_t)s->offsets[s->count] * sizeof(Particle), hipMemcpyHostToDevice, s->stream),
               "H2D of %u members' particles (up to %u each)", s->count, s->n);
    split_members(s);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_batch_set_data");
    s->has_data = true;
}

void nb_hip_batch_get_data(const SimBatch *s, Particle *ps) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    read_back(const_cast<SimBatch *>(s), 0, s->count, ps);
}

void nb_hip_batch_get_member(const SimBatch *s, uint32_t b, Particle *ps) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    NB_ASSERT(b < s->count, "member %u of %u", b, s->count);
    read_back(const_cast<SimBatch *>(s), b, 1, ps);
}

void nb_hip_batch_step_async(SimBatch *s, uint32_t n, const float *dt) { enqueue(s, n, dt, false); }

void nb_hip_batch_sync(SimBatch *s) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (!s->on_device) return;
    use_device();
    ASSERT_HIP(hipStreamSynchronize(s->stream), "stream sync");
}

void nb_hip_batch_update(SimBatch *s, uint32_t n, float dt) {
    enqueue(s, n, &dt, true);
    nb_hip_batch_sync(s);
}

void nb_hip_batch_update_dts(SimBatch *s, uint32_t n, const float *dt) {
    enqueue(s, n, dt, false);
    nb_hip_batch_sync(s);
}

void nb_hip_ensemble_leapfrog(SimBatch *s, uint32_t n, float dt) {
    enqueue_leapfrog(s, n, &dt, true, "nb_hip_ensemble_leapfrog");
    if (n > 0) nb_hip_batch_sync(s);
}

void nb_hip_ensemble_leapfrog_dts(SimBatch *s, uint32_t n, const float *dt) {
    enqueue_leapfrog(s, n, dt, false, "nb_hip_ensemble_leapfrog_dts");
    if (n > 0) nb_hip_batch_sync(s);
}

void nb_hip_ensemble_last_leapfrog_info(const SimBatch *s, uint32_t *force_launches, int *primed) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (force_launches) *force_launches = s->lf_force_launches;
    if (primed) *primed = s->lf_primed ? 1 : 0;
}

// n adaptive steps of every member; nothing returns to the host until the one copy at the end.
void nb_hip_ensemble_adaptive_steps(SimBatch *s, uint32_t n, const NbAdaptive *cfg, float *dt_log, NbAdaptiveResult *out) {
    const char *what = "nb_hip_ensemble_adaptive_steps";
    check_adaptive_cfg(s, n, cfg, what);
    NB_ASSERT(!s->ragged, "%s: adaptive steps of ragged ensembles (members of different sizes) are not supported", what);
    if (n == 0) {
        if (out) memset(out, 0, (size_t)s->count * sizeof *out);
        return;
    }
    NB_ASSERT(s->has_data, "%s before nb_hip_batch_set_data", what);
    use_device();
    const size_t head = (size_t)s->count * sizeof(nb::AdaptState);
    const size_t log_bytes = dt_log ? (size_t)n * s->count * sizeof(float) : 0;
    s->adapt.grown_carrying(s->stream, head + log_bytes, head);
    nb::TimestepParams t = nb::timestep_params(s->acc, s->radius, s->n, s->stride, *cfg);
    char *records = s->adapt;
    t.state = reinterpret_cast<nb::AdaptState *>(records);
    t.commit = 1;
    if (!(cfg->flags & NB_ADAPT_CONTINUE) || !s->adapt_armed) nb::launch_arm(s->stream, t.state, s->count);
    s->adapt_armed = true;
    const bool leapfrog = (cfg->flags & NB_ADAPT_LEAPFROG) != 0;
    run_call(s, {n, leapfrog, true, !leapfrog && (cfg->flags & NB_ADAPT_PRIME) != 0}, t,
             dt_log ? reinterpret_cast<float *>(records + head) : nullptr);
    s->adapt_host.resize(head + log_bytes);
    ASSERT_HIP(hipMemcpyAsync(s->adapt_host.data(), s->adapt, head + log_bytes, hipMemcpyDeviceToHost, s->stream),
               "D2H of %u x %u step sizes and the results", n, s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after an adaptive ensemble update");
    for (uint32_t b = 0; out && b < s->count; b++) out[b] = nb::adaptive_result(s->adapt_host.data() + (size_t)b * sizeof(nb::AdaptState));
    if (dt_log) memcpy(dt_log, s->adapt_host.data() + head, log_bytes);
}

double nb_hip_batch_last_ms(SimBatch *s) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (!s->step_iv.valid()) return 0.0;
    use_device();
    return s->step_iv.ms();
}

uint32_t nb_hip_batch_dt_uploads(const SimBatch *s) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    return s->dt_uploads;
}

uint32_t nb_hip_ensemble_trace_rows(uint32_t n, uint32_t every) {
    NB_ASSERT(every > 0, "every = 0: a traced update records every k >= 1 steps");
    return 1u + n / every;
}

void nb_hip_ensemble_trace(SimBatch *s, uint32_t n, float dt, uint32_t every, WorldEnergy *out) { trace(s, n, &dt, true, every, out); }

void nb_hip_ensemble_trace_dts(SimBatch *s, uint32_t n, const float *dt, uint32_t every, WorldEnergy *out) {
    trace(s, n, dt, false, every, out);
}

// tuning hooks (nbody_hip_tuning.h)
void nb_hip_ensemble_trace_mode(SimBatch *s, int mode) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    NB_ASSERT(mode == 0 || mode == 1, "trace mode %d (0 = auto, 1 = interleaved)", mode);
    s->trace_mode = mode;
}

void nb_hip_ensemble_last_trace_info(const SimBatch *s, int *fused, uint32_t *launches) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (fused) *fused = s->trace_fused;
    if (launches) *launches = s->trace_launches;
}

void nb_hip_batch_launch_shape(const SimBatch *s, int *path, int *k, int *w, int *lanes, uint32_t *workgroups) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    const SimBatch::Group &first = s->groups[0];
    uint32_t total = 0;
    for (const auto &g : s->groups) total += g.workgroups;
    if (path) *path = s->lane_split() ? 1 : 0;
    if (k) *k = first.k;
    if (w) *w = first.w;
    if (lanes) *lanes = first.lanes;
    if (workgroups) *workgroups = total;
}

}  // extern "C"
