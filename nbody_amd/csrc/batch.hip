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
// nb_hip_ensemble_bounds / _render_counts / _render_rgba look at every member without reading it back (kernels:
// batch_render.hip): a constant number of launches, one copy of the images and one sync for any B.
// The path is chosen by N alone -- never by B or by the members' source counts -- and the kernels run the very bodies of
// chain_kernel / lane_split_kernel, so member b's bits are those of the same particles alone in a SimPipeline pinned to
// that shape (tests/test_gpu_batch.py).  Members share nothing with each other and a SimBatch shares nothing with any
// SimPipeline: own stream, own buffers, own events.
//
// A RAGGED ensemble (nb_hip_ragged_create) is the same SimBatch with a particle count per member.  The SoA arrays keep one
// stride (the largest member rounded up to 64 rows), the AoS side of the seam is packed (member b at offsets[b]), and the
// members fall into up to three launch GROUPS by their own size alone -- chain (N <= 512), lane-split (8, 8), lane-split
// (16, 4) -- each with a device list of its member indices: one chain launch per call and one lane-split launch per group
// and step (kernels.hip ragged_*_kernel, the same bodies with the receiver count read per member).  Member b's bits are
// those of the same particles as the only member of a uniform SimBatch of its size.  A uniform SimBatch launches exactly
// what it launched before ragged ones existed.
#include "pipeline_internal.h"
#include "batch_diag.h"
#include "batch_render.h"
#include "diag_sums.h"
#include "leapfrog.h"
#include "nbody_hip_tuning.h"
#include "render_common.h"
#include "timestep.h"
#include "timestep_common.h"

using namespace nbi;

struct SimBatch {
    uint32_t count = 0;     // members
    uint32_t n = 0;         // particles per member; ragged: of the largest member
    uint32_t stride = 0;    // rows per member in the SoA arrays: n rounded up to 64 (256-byte aligned float rows)
    std::vector<uint32_t> n_len;      // [count] particles of each member
    std::vector<uint64_t> offsets;    // [count + 1] member b's first record in the packed AoS arrays of the seam
    bool ragged = false;              // made by nb_hip_ragged_create
    std::vector<uint32_t> mass_len;   // [count]
    std::vector<float> dt_host;       // [count]: what dt_dev holds (valid once dt_valid)
    bool dt_valid = false;
    uint32_t dt_uploads = 0;

    bool on_device = false;
    bool has_data = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool timed = false;
    float2 *pos[2] = {nullptr, nullptr};
    float2 *vel = nullptr, *acc = nullptr;
    float *radius = nullptr, *mass = nullptr, *gm = nullptr;
    uint32_t *mass_len_dev = nullptr;
    float *dt_dev = nullptr;
    void *aos = nullptr;   // device staging of Set / Get: [count][n] Particle
    int cur = 0;           // pos[cur] is the latest state (the chain path never moves it)

    // the launch shape, fixed at creation
    int path = 0;          // 0 chain, 1 lane-split
    int k = 2, w = 16, lanes = 1;
    uint32_t tiles = 0;
    uint32_t workgroups = 0;

    // ragged only: the launch groups, in the order chain, lane-split (8, 8), lane-split (16, 4); those without members are
    // absent.  path = 1 as soon as one member is lane-split (both position buffers exist, traces interleave).
    struct Group {
        int path = 0, k = 2, w = 16, lanes = 1;   // chain: w of the group's largest member
        uint32_t max_n = 0;                       // its largest member
        uint32_t workgroups = 0;                  // per launch
        std::vector<uint32_t> members;            // ascending member indices
        uint32_t *list = nullptr;                 // the same on the device
    };
    std::vector<Group> groups;
    uint32_t *n_len_dev = nullptr;
    uint64_t *offsets_dev = nullptr;

    // nb_hip_ensemble_energy / nb_hip_ensemble_potential (kernels: batch_diag.hip): scratch made on first use, an event
    // pair of their own (ev[] keeps bracketing the last update)
    double *diag = nullptr;      // float64 slab: [count][tiles of 128][NB_DIAG_SUMS] + the [count][NB_DIAG_SUMS] results
    size_t diag_cap = 0;         // doubles allocated in diag
    float *diag_phi = nullptr;   // the potentials on the device: [count][n]
    size_t diag_phi_cap = 0;
    std::vector<double> diag_host;   // the results on the host before they become WorldEnergy
    hipEvent_t ev_diag[2] = {nullptr, nullptr};
    bool diag_timed = false;

    // nb_hip_ensemble_trace: the rows of the last traced call, on the device and on their way to WorldEnergy
    double *trace = nullptr;     // [records][count][NB_DIAG_SUMS]
    size_t trace_cap = 0;
    std::vector<double> trace_host;
    int trace_mode = 0;          // tuning hook: 1 = interleaved diagnostics launches also where the chain could record
    int trace_fused = 0;         // what the last traced call did
    uint32_t trace_launches = 0;

    // nb_hip_ensemble_bounds / _render_counts / _render_rgba (kernels: batch_render.hip): scratch made on first use, an
    // event pair of their own
    RenderView *render_views = nullptr;      // [count]: the views of the last call
    uint32_t *render_keys = nullptr;         // [count][4]
    uint32_t *render_counts = nullptr;       // tile path: [count][3][h][w]; global path: the disc cursor behind them
    size_t render_counts_cap = 0;
    uint32_t *render_rgba = nullptr;         // [count][h][w]
    size_t render_rgba_cap = 0;
    nbr::EnsembleDisc *render_discs = nullptr;   // global path: [count * n]
    hipEvent_t ev_render[2] = {nullptr, nullptr};
    bool render_timed = false;
    int render_mode = 0;                     // tuning hook: 1 = the global path also where the tile path applies
    int render_tile = 0;                     // what the last render did (a bounds call leaves both alone)
    uint32_t render_launches = 0;

    // nb_hip_ensemble_adaptive_steps (kernels: timestep.hip): [count] AdaptState, then the call's log [n][count]; grown on demand
    void *adapt = nullptr;
    size_t adapt_bytes = 0;
    bool adapt_armed = false;   // the records hold a call to continue (NB_ADAPT_CONTINUE)
    std::vector<char> adapt_host;

    // leapfrog steps (kernels: leapfrog.hip): the step sizes of the kick / drift passes, [2][count] -- a fixed-step call uses
    // the first row, an adaptive one alternates so that one launch can close step i - 1 and open step i
    float *lf_dt = nullptr;
    bool acc_current = false;        // acc = F(x) of the state held: true after a leapfrog call, false after anything else that moves it
    uint32_t lf_force_launches = 0;  // force evaluations of the last leapfrog call (nb_hip_ensemble_last_leapfrog_info)
    bool lf_primed = false;          // ... and whether it had to run one first
};

namespace {

void materialize(SimBatch *s) {
    use_device();
    if (s->on_device) return;
    ASSERT_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking), "stream");
    for (auto &e : s->ev) ASSERT_HIP(hipEventCreate(&e), "event");
    const size_t rows = (size_t)s->count * s->stride;
    for (int b = 0; b < 2; b++) {
        if (b == 1 && s->path == 0) break;   // the chain updates positions in place
        s->pos[b] = dev_alloc<float2>(rows);
        ASSERT_HIP(hipMemsetAsync(s->pos[b], 0, rows * sizeof(float2), s->stream), "clear positions");
    }
    s->vel = dev_alloc<float2>(rows);
    s->acc = dev_alloc<float2>(rows);
    s->radius = dev_alloc<float>(rows);
    s->mass = dev_alloc<float>(rows);
    s->gm = dev_alloc<float>(rows);
    s->mass_len_dev = dev_alloc<uint32_t>(s->count);
    s->dt_dev = dev_alloc<float>(s->count);
    s->aos = dev_alloc<Particle>((size_t)s->offsets[s->count]);
    if (s->ragged) {
        // pad rows stay zero for the life of the ensemble: no kernel writes a row at or beyond n_len[b]
        ASSERT_HIP(hipMemsetAsync(s->vel, 0, rows * sizeof(float2), s->stream), "clear velocities");
        ASSERT_HIP(hipMemsetAsync(s->acc, 0, rows * sizeof(float2), s->stream), "clear accelerations");
        ASSERT_HIP(hipMemsetAsync(s->radius, 0, rows * sizeof(float), s->stream), "clear radii");
        ASSERT_HIP(hipMemsetAsync(s->mass, 0, rows * sizeof(float), s->stream), "clear masses");
        ASSERT_HIP(hipMemsetAsync(s->gm, 0, rows * sizeof(float), s->stream), "clear G*m");
        s->n_len_dev = dev_alloc<uint32_t>(s->count);
        s->offsets_dev = dev_alloc<uint64_t>((size_t)s->count + 1);
        ASSERT_HIP(hipMemcpyAsync(s->n_len_dev, s->n_len.data(), (size_t)s->count * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream),
                   "H2D of %u member sizes", s->count);
        ASSERT_HIP(hipMemcpyAsync(s->offsets_dev, s->offsets.data(), ((size_t)s->count + 1) * sizeof(uint64_t), hipMemcpyHostToDevice,
                                  s->stream),
                   "H2D of %u member offsets", s->count);
        for (auto &g : s->groups) {
            g.list = dev_alloc<uint32_t>(g.members.size());
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
    p.tiles = s->tiles;
    return p;
}

// n lane-split steps, one launch each
void launch_lane_steps(SimBatch *s, nb::BatchParams &p, uint32_t n) {
    const void *fn = nb::batch_lane_split_fn(s->w, s->lanes);
    const nb::LaunchShape sh = {.k = 1, .w = s->w, .variant = nb::VARIANT_LDS, .split = 1, .unit = 8, .lanes = s->lanes};
    dim3 grid = nb::step_grid(sh, s->n);
    grid.y = s->count;
    for (uint32_t i = 0; i < n; i++) {
        p.pos_in = s->pos[s->cur];
        p.pos_out = s->pos[s->cur ^ 1];
        void *args[] = {&p};
        ASSERT_HIP(hipLaunchKernel(fn, grid, nb::step_block(sh), args, nb::step_lds_bytes(sh, s->n), s->stream),
                   "ensemble lane-split launch (w=%d lanes=%d, %u members of %u)", s->w, s->lanes, s->count, s->n);
        s->cur ^= 1;
    }
}

// n steps of a ragged ensemble: per step one launch for every lane-split group (all of them flip the ping-pong phase
// together), then the chain group's whole call in place in the buffer it started from -- and, when the phase moved, one
// copy of the chain members' position rows into the buffer that is now the latest, so that every reader (read-back,
// diagnostics, the next call) finds all members in pos[cur].  Returns the launches made.
uint32_t launch_ragged_steps(SimBatch *s, const nb::BatchParams &p0, uint32_t n) {
    uint32_t launches = 0;
    const int cur0 = s->cur;
    for (uint32_t i = 0; i < n && s->path != 0; i++) {
        for (const auto &g : s->groups) {
            if (g.path == 0) continue;
            nb::RaggedParams rp = {p0, s->n_len_dev, g.list};
            rp.b.pos_in = s->pos[s->cur];
            rp.b.pos_out = s->pos[s->cur ^ 1];
            const nb::LaunchShape sh = {.k = 1, .w = g.w, .variant = nb::VARIANT_LDS, .split = 1, .unit = 8, .lanes = g.lanes};
            dim3 grid = nb::step_grid(sh, g.max_n);
            grid.y = (uint32_t)g.members.size();
            void *args[] = {&rp};
            ASSERT_HIP(hipLaunchKernel(nb::ragged_lane_split_fn(g.w, g.lanes), grid, nb::step_block(sh), args,
                                       nb::step_lds_bytes(sh, g.max_n), s->stream),
                       "ragged lane-split launch (w=%d lanes=%d, %zu members of up to %u)", g.w, g.lanes, g.members.size(), g.max_n);
            launches++;
        }
        s->cur ^= 1;
    }
    for (const auto &g : s->groups) {
        if (g.path != 0) continue;
        nb::RaggedParams rp = {p0, s->n_len_dev, g.list};
        rp.b.pos_in = rp.b.pos_out = s->pos[cur0];
        for (uint32_t left = n; left > 0; left -= rp.b.steps, launches++) {
            rp.b.steps = left > CHAIN_MAX_STEPS_PER_LAUNCH ? CHAIN_MAX_STEPS_PER_LAUNCH : left;
            nb::launch_ragged_chain(s->stream, rp, (uint32_t)g.members.size());
        }
        if (s->cur != cur0 && n > 0) {
            nb::launch_ragged_copy_rows(s->stream, g.list, s->n_len_dev, (uint32_t)g.members.size(), g.max_n, s->stride, s->pos[cur0],
                                        s->pos[s->cur]);
            launches++;
        }
    }
    return launches;
}

// n steps, no record: whole chain launches or lane-split launches; returns the launches made
uint32_t launch_steps(SimBatch *s, nb::BatchParams &p, uint32_t n) {
    if (s->ragged) return launch_ragged_steps(s, p, n);
    if (s->path != 0) {
        launch_lane_steps(s, p, n);
        return n;
    }
    uint32_t launches = 0;
    p.pos_in = p.pos_out = s->pos[s->cur];
    for (uint32_t left = n; left > 0; left -= p.steps, launches++) {
        p.steps = left > CHAIN_MAX_STEPS_PER_LAUNCH ? CHAIN_MAX_STEPS_PER_LAUNCH : left;
        nb::launch_batch_chain(s->stream, p, s->count);
    }
    return launches;
}

void enqueue(SimBatch *s, uint32_t n, const float *dt, bool uniform) {
    NB_ASSERT(s != nullptr && dt != nullptr, "NULL argument");
    NB_ASSERT(s->has_data, "ensemble update before nb_hip_batch_set_data");
    if (n == 0) return;
    use_device();
    s->acc_current = false;   // an Euler step leaves the acc of the state before it
    upload_dts(s, dt, uniform);
    nb::BatchParams p = step_params(s);
    ASSERT_HIP(hipEventRecord(s->ev[0], s->stream), "event record");
    launch_steps(s, p, n);
    ASSERT_HIP(hipGetLastError(), "ensemble launch (%u members of %u particles, %u steps)", s->count, s->n, n);
    ASSERT_HIP(hipEventRecord(s->ev[1], s->stream), "event record");
    s->timed = true;
}

// ---- leapfrog steps: the passes of leapfrog.hip around the launches of a one-step dt = 0 update ----------------------------

// one pass over every member: close with row `close_row` of lf_dt, open (kick + drift of the latest positions) with `open_row`
void launch_kicks(SimBatch *s, bool close, bool open, uint32_t close_row, uint32_t open_row) {
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

void launch_force(SimBatch *s, nb::BatchParams &p) {
    launch_steps(s, p, 1);
    s->lf_force_launches++;
}

// the step kernels' dt[count] holds 0 for the whole call; one unlogged, uncounted force evaluation first when acc is not
// known to be the members' own
void begin_leapfrog(SimBatch *s, nb::BatchParams &p) {
    if (!s->lf_dt) s->lf_dt = dev_alloc<float>(2 * (size_t)s->count);
    const float zero = 0.0f;
    upload_dts(s, &zero, true);
    s->lf_force_launches = 0;
    s->lf_primed = !s->acc_current;
    if (s->lf_primed) launch_force(s, p);
}

// n kick-drift-kick steps, every member with its own step size: open, force, one close + open pass and a force launch per
// further step, close
void enqueue_leapfrog(SimBatch *s, uint32_t n, const float *dt, bool uniform, const char *what) {
    NB_ASSERT(s != nullptr && dt != nullptr, "%s: NULL argument", what);
    NB_ASSERT(!s->ragged, "%s: leapfrog steps of ragged ensembles (members of different sizes) are not supported", what);
    if (n == 0) return;
    NB_ASSERT(s->has_data, "%s before nb_hip_batch_set_data", what);
    use_device();
    nb::BatchParams p = step_params(s);
    begin_leapfrog(s, p);
    if (uniform) {
        nb::launch_batch_fill(s->stream, s->lf_dt, s->count, dt[0]);
    } else {
        ASSERT_HIP(hipStreamSynchronize(s->stream), "sync before a per-member step-size upload");
        ASSERT_HIP(hipMemcpy(s->lf_dt, dt, (size_t)s->count * sizeof(float), hipMemcpyHostToDevice), "H2D of %u step sizes", s->count);
    }
    ASSERT_HIP(hipEventRecord(s->ev[0], s->stream), "event record");
    for (uint32_t i = 0; i < n; i++) {
        launch_kicks(s, i > 0, true, 0, 0);
        launch_force(s, p);
    }
    launch_kicks(s, true, false, 0, 0);
    ASSERT_HIP(hipGetLastError(), "leapfrog ensemble launches (%u members of %u particles, %u steps)", s->count, s->n, n);
    ASSERT_HIP(hipEventRecord(s->ev[1], s->stream), "event record");
    s->timed = true;
    s->dt_valid = false;   // the next fixed-step update uploads its own step sizes afresh
    s->acc_current = true;
}

void read_back(SimBatch *s, uint32_t first, uint32_t members, Particle *ps) {
    NB_ASSERT(s != nullptr && ps != nullptr, "NULL argument");
    NB_ASSERT(s->has_data, "ensemble read-back before nb_hip_batch_set_data");
    use_device();
    if (s->ragged)
        nb::launch_ragged_merge(s->stream, s->aos, s->offsets_dev, s->n_len_dev, first, members, s->n, s->stride, s->pos[s->cur], s->vel,
                                s->acc, s->radius, s->mass);
    else
        nb::launch_batch_merge(s->stream, s->aos, first, members, s->n, s->stride, s->pos[s->cur], s->vel, s->acc, s->radius, s->mass);
    ASSERT_HIP(hipMemcpyAsync(ps, static_cast<const Particle *>(s->aos) + s->offsets[first],
                              (size_t)(s->offsets[first + members] - s->offsets[first]) * sizeof(Particle), hipMemcpyDeviceToHost,
                              s->stream),
               "D2H of %u members", members);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after an ensemble read-back");
}

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

nbd::EnsembleDiagParams begin_diag(SimBatch *s) {
    use_device();
    if (!s->ev_diag[0]) {
        for (auto &e : s->ev_diag) ASSERT_HIP(hipEventCreate(&e), "event");
    }
    ASSERT_HIP(hipEventRecord(s->ev_diag[0], s->stream), "record diagnostics begin");
    return diag_params(s);
}

void end_diag(SimBatch *s) {
    ASSERT_HIP(hipEventRecord(s->ev_diag[1], s->stream), "record diagnostics end");
    s->diag_timed = true;
}

template <typename T>
T *grown(SimBatch *s, T *&buf, size_t &cap, size_t need) {
    if (cap < need) {
        if (buf) {
            ASSERT_HIP(hipStreamSynchronize(s->stream), "sync before regrowing a diagnostics buffer");
            dev_free(buf);
        }
        buf = dev_alloc<T>(need);
        cap = need;
    }
    return buf;
}

// The two launches of an energy diagnostic of the latest state: every member's eight sums -> res[count][NB_DIAG_SUMS].
void launch_energy_sums(SimBatch *s, double *res) {
    const uint32_t tiles = nbd::ensemble_tiles(s->n);
    nbd::EnsembleDiagParams p = diag_params(s);
    p.slab = s->diag;
    nbd::launch_ensemble_potential(s->stream, p, s->count);
    ASSERT_HIP(hipGetLastError(), "ensemble_phi_kernel launch (energy, %u members of %u)", s->count, s->n);
    nbd::launch_ensemble_reduce(s->stream, s->diag, s->mass_len_dev, tiles, s->count, res);
    ASSERT_HIP(hipGetLastError(), "ensemble_reduce_kernel launch (%u members)", s->count);
}

// The slab of per-tile rows, with room for one call's results behind it.
double *energy_slab(SimBatch *s) {
    return grown(s, s->diag, s->diag_cap, (size_t)s->count * (nbd::ensemble_tiles(s->n) + 1) * NB_DIAG_SUMS);
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
    double *rows = grown(s, s->trace, s->trace_cap, (size_t)records * pitch);
    const bool fused = s->path == 0 && s->trace_mode == 0;
    if (!fused) energy_slab(s);
    nb::BatchParams p = step_params(s);
    uint32_t launches = 0;
    ASSERT_HIP(hipEventRecord(s->ev[0], s->stream), "event record");
    if (fused) {
        nb::BatchTraceParams t;
        memset(&t, 0, sizeof t);
        t.mass = s->mass;
        t.rows = rows;
        t.count = s->count;
        t.every = every;
        p.pos_in = p.pos_out = s->pos[s->cur];
        do {   // n = 0 is one launch of no steps: the record on entry
            const uint32_t left = n - t.done;
            p.steps = left > CHAIN_MAX_STEPS_PER_LAUNCH ? CHAIN_MAX_STEPS_PER_LAUNCH : left;
            t.b = p;
            if (s->ragged)   // fused means every member is in the chain group: its list is 0 .. count - 1
                nb::launch_ragged_trace_chain(s->stream, nb::RaggedTraceParams{t, s->n_len_dev, s->groups[0].list}, s->count);
            else
                nb::launch_batch_trace_chain(s->stream, t);
            t.done += p.steps;
            launches++;
        } while (t.done < n);
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
    ASSERT_HIP(hipEventRecord(s->ev[1], s->stream), "event record");
    s->timed = true;
    s->trace_fused = fused;
    s->trace_launches = launches;
    s->trace_host.resize((size_t)records * pitch);
    ASSERT_HIP(hipMemcpyAsync(s->trace_host.data(), rows, (size_t)records * pitch * sizeof(double), hipMemcpyDeviceToHost, s->stream),
               "D2H of %u x %u energy rows", records, s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after a traced ensemble update");
    for (size_t i = 0; i < (size_t)records * s->count; i++) nb_energy_from_sums(s->trace_host.data() + i * Q, out + i);
}

// ---- rendering: bounds, count tiles and frames of every member, without reading the particles back ------------------

void begin_render(SimBatch *s) {
    use_device();
    if (!s->ev_render[0]) {
        for (auto &e : s->ev_render) ASSERT_HIP(hipEventCreate(&e), "event");
    }
    ASSERT_HIP(hipEventRecord(s->ev_render[0], s->stream), "record render begin");
}

void end_render(SimBatch *s) {
    ASSERT_HIP(hipEventRecord(s->ev_render[1], s->stream), "record render end");
    s->render_timed = true;
}

void check_views(const SimBatch *s, const RenderView *views, const char *what) {
    NB_ASSERT(views != nullptr, "%s: NULL RenderView array", what);
    uint32_t member = 0;
    const char *fault = nb_render_views_fault(views, s->count, &member);
    NB_ASSERT(fault == nullptr, "%s: invalid RenderView of member %u of %u (%u x %u, zoom %g): %s", what, member, s->count,
              views[member].width, views[member].height, (double)views[member].zoom, fault);
}

// The count images of the latest state on the stream: the tile kernel (straight to the frame when a palette is given) or
// clear + splat + disc pass (+ shade); *launches = what was enqueued.
void enqueue_render(SimBatch *s, const RenderView *views, const RenderPalette *palette, uint32_t *launches) {
    const uint32_t width = views[0].width, height = views[0].height;
    const size_t plane = (size_t)width * height;
    const bool tile = nbr::tile_fits(width, height) && s->render_mode == 0;
    if (!s->render_views) s->render_views = dev_alloc<RenderView>(s->count);
    if (palette) grown(s, s->render_rgba, s->render_rgba_cap, (size_t)s->count * plane);
    if (!tile || !palette) grown(s, s->render_counts, s->render_counts_cap, nbr::global_count_words(s->count, width, height));
    if (!tile && !s->render_discs) s->render_discs = dev_alloc<nbr::EnsembleDisc>((size_t)s->count * s->n);
    ASSERT_HIP(hipMemcpyAsync(s->render_views, views, (size_t)s->count * sizeof(RenderView), hipMemcpyHostToDevice, s->stream),
               "H2D of %u views", s->count);
    begin_render(s);
    nbr::EnsembleRenderParams p{};
    p.pos = s->pos[s->cur];
    p.mass = s->mass;
    p.radius = s->radius;
    p.n = s->n;
    p.stride = s->stride;
    p.count = s->count;
    p.width = width;
    p.height = height;
    p.views = s->render_views;
    if (tile) {
        nbr::launch_ensemble_tile(s->stream, p, s->render_counts, palette, s->render_rgba);
        *launches = 1;
    } else {
        ASSERT_HIP(hipMemsetAsync(s->render_counts, 0, nbr::global_count_words(s->count, width, height) * sizeof(uint32_t), s->stream),
                   "clear %u count images and the disc cursor", s->count);
        nbr::launch_ensemble_global(s->stream, p, s->render_counts, s->render_discs);
        *launches = 3;
        if (palette) {
            nbr::launch_ensemble_shade(s->stream, s->render_counts, s->count, (uint32_t)plane, *palette, s->render_rgba);
            *launches = 4;
        }
    }
    ASSERT_HIP(hipGetLastError(), "ensemble render launch (%u members of %u particles, %u x %u, %s path)", s->count, s->n, width, height,
               tile ? "tile" : "global");
    end_render(s);
    s->render_tile = tile;
    s->render_launches = *launches;
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
    s->count = count;
    s->n = total_len;
    s->stride = round_up(total_len, 64);
    s->mass_len.assign(mass_len, mass_len + count);
    s->dt_host.assign(count, 0.0f);
    s->n_len.assign(count, total_len);
    s->offsets.resize((size_t)count + 1);
    for (uint32_t b = 0; b <= count; b++) s->offsets[b] = (uint64_t)b * total_len;
    s->tiles = nb::chain_tiles(total_len);
    if (s->tiles) {
        s->path = 0;
        s->k = 2;
        s->w = (int)(16u / s->tiles);
        s->lanes = 1;
        s->workgroups = count;
    } else {
        s->path = 1;
        s->k = 1;
        s->lanes = nb::batch_lane_shape(total_len, &s->w);
        NB_ASSERT(s->lanes > 1 && nb::batch_lane_split_fn(s->w, s->lanes) != nullptr, "no ensemble kernel for w=%d lanes=%d", s->w,
                  s->lanes);
        s->workgroups = count * ((total_len + 64u / (uint32_t)s->lanes - 1) / (64u / (uint32_t)s->lanes));
    }
    return s;
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
    s->ragged = true;
    s->count = count;
    s->mass_len.assign(mass_len, mass_len + count);
    s->n_len.assign(total_len, total_len + count);
    s->dt_host.assign(count, 0.0f);
    s->offsets.resize((size_t)count + 1);
    s->offsets[0] = 0;
    SimBatch::Group slot[3];   // chain, lane-split (8, 8), lane-split (16, 4)
    for (uint32_t b = 0; b < count; b++) {
        const uint32_t n = total_len[b];
        s->offsets[b + 1] = s->offsets[b] + n;
        s->n = n > s->n ? n : s->n;
        int which = 0, w = 16, lanes = 1;
        if (nb::chain_tiles(n) == 0) {
            lanes = nb::batch_lane_shape(n, &w);
            NB_ASSERT(lanes > 1 && nb::ragged_lane_split_fn(w, lanes) != nullptr, "member %u: no ensemble kernel for w=%d lanes=%d", b, w,
                      lanes);
            which = lanes == 8 ? 1 : 2;
        }
        SimBatch::Group &g = slot[which];
        g.path = which != 0;
        g.k = which ? 1 : 2;
        g.lanes = lanes;
        g.max_n = n > g.max_n ? n : g.max_n;
        g.w = which ? w : (int)(16u / nb::chain_tiles(g.max_n));
        g.members.push_back(b);
    }
    s->stride = round_up(s->n, 64);
    for (auto &g : slot) {
        if (g.members.empty()) continue;
        const uint32_t per = g.path ? (g.max_n + 64u / (uint32_t)g.lanes - 1) / (64u / (uint32_t)g.lanes) : 1u;
        g.workgroups = (uint32_t)g.members.size() * per;
        s->workgroups += g.workgroups;
        if (g.path) s->path = 1;
        s->groups.push_back(g);
    }
    s->k = s->groups[0].k;
    s->w = s->groups[0].w;
    s->lanes = s->groups[0].lanes;
    return s;
}

void nb_hip_ragged_layout(const SimBatch *s, uint32_t *sizes, uint64_t *offsets) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (sizes) memcpy(sizes, s->n_len.data(), (size_t)s->count * sizeof(uint32_t));
    if (offsets) memcpy(offsets, s->offsets.data(), ((size_t)s->count + 1) * sizeof(uint64_t));
}

uint32_t nb_hip_ragged_launch_shape(const SimBatch *s, uint32_t group, int *path, int *k, int *w, int *lanes, uint32_t *members,
                                    uint32_t *workgroups) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    const uint32_t groups = s->ragged ? (uint32_t)s->groups.size() : 1u;
    NB_ASSERT(group < groups, "launch group %u of %u", group, groups);
    SimBatch::Group uniform;   // a uniform ensemble is one group of all members
    if (!s->ragged) {
        uniform.path = s->path;
        uniform.k = s->k;
        uniform.w = s->w;
        uniform.lanes = s->lanes;
        uniform.workgroups = s->workgroups;
    }
    const SimBatch::Group &g = s->ragged ? s->groups[group] : uniform;
    if (path) *path = g.path;
    if (k) *k = g.k;
    if (w) *w = g.w;
    if (lanes) *lanes = g.lanes;
    if (members) *members = s->ragged ? (uint32_t)g.members.size() : s->count;
    if (workgroups) *workgroups = g.workgroups;
    return groups;
}

void nb_hip_ragged_member_shape(const SimBatch *s, uint32_t member, uint32_t *group, int *k, int *w, int *lanes) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    NB_ASSERT(member < s->count, "member %u of %u", member, s->count);
    const uint32_t n = s->n_len[member], tiles = nb::chain_tiles(n);
    int mw = 16, ml = 1;
    if (tiles)
        mw = (int)(16u / tiles);
    else
        ml = nb::batch_lane_shape(n, &mw);
    uint32_t gi = 0;
    for (uint32_t i = 0; s->ragged && i < s->groups.size(); i++)
        if (s->groups[i].path == (tiles ? 0 : 1) && (tiles || s->groups[i].lanes == ml)) gi = i;
    if (group) *group = gi;
    if (k) *k = tiles ? 2 : 1;
    if (w) *w = mw;
    if (lanes) *lanes = ml;
}

void nb_hip_batch_destroy(SimBatch *s) {
    if (s == nullptr) return;
    if (s->on_device) {
        use_device();
        ASSERT_HIP(hipStreamSynchronize(s->stream), "sync before destroying an ensemble");
        for (auto &p : s->pos) dev_free(p);
        dev_free(s->vel);
        dev_free(s->acc);
        dev_free(s->radius);
        dev_free(s->mass);
        dev_free(s->gm);
        dev_free(s->mass_len_dev);
        dev_free(s->dt_dev);
        dev_free(s->aos);
        if (s->n_len_dev) dev_free(s->n_len_dev);
        if (s->offsets_dev) dev_free(s->offsets_dev);
        for (auto &g : s->groups)
            if (g.list) dev_free(g.list);
        if (s->diag) dev_free(s->diag);
        if (s->diag_phi) dev_free(s->diag_phi);
        if (s->trace) dev_free(s->trace);
        if (s->render_views) dev_free(s->render_views);
        if (s->render_keys) dev_free(s->render_keys);
        if (s->render_counts) dev_free(s->render_counts);
        if (s->render_rgba) dev_free(s->render_rgba);
        if (s->render_discs) dev_free(s->render_discs);
        if (s->adapt) dev_free(s->adapt);
        if (s->lf_dt) dev_free(s->lf_dt);
        for (auto &e : s->ev_render)
            if (e) ASSERT_HIP(hipEventDestroy(e), "event");
        for (auto &e : s->ev_diag)
            if (e) ASSERT_HIP(hipEventDestroy(e), "event");
        for (auto &e : s->ev) ASSERT_HIP(hipEventDestroy(e), "event");
        ASSERT_HIP(hipStreamDestroy(s->stream), "stream");
    }
    delete s;
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
    if (s->ragged)
        nb::launch_ragged_split(s->stream, s->aos, s->offsets_dev, s->n_len_dev, s->mass_len_dev, s->count, s->n, s->stride, s->pos[0],
                                s->vel, s->acc, s->radius, s->mass, s->gm, NB_G);
    else
        nb::launch_batch_split(s->stream, s->aos, s->mass_len_dev, s->count, s->n, s->stride, s->pos[0], s->vel, s->acc, s->radius,
                               s->mass, s->gm, NB_G);
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

// n adaptive steps of every member: per step the criterion launch (one workgroup per member writes dt[b]), then the launches
// of a one-step update reading the same dt[count]; nothing returns to the host until the one copy at the end.
void nb_hip_ensemble_adaptive_steps(SimBatch *s, uint32_t n, const NbAdaptive *cfg, float *dt_log, NbAdaptiveResult *out) {
    const char *what = "nb_hip_ensemble_adaptive_steps";
    NB_ASSERT(s != nullptr && cfg != nullptr, "%s: NULL argument", what);
    const char *fault = nb_timestep_cfg_fault(cfg);
    NB_ASSERT(fault == nullptr, "%s: %s (eta %g, dt_min %g, dt_max %g, span %g)", what, fault, (double)cfg->eta, (double)cfg->dt_min,
              (double)cfg->dt_max, cfg->span);
    NB_ASSERT(n <= NB_ADAPT_MAX_STEPS, "%s: %u steps > 2^20 in one call", what, n);
    NB_ASSERT(!s->ragged, "%s: adaptive steps of ragged ensembles (members of different sizes) are not supported", what);
    if (n == 0) {
        if (out) memset(out, 0, (size_t)s->count * sizeof *out);
        return;
    }
    NB_ASSERT(s->has_data, "%s before nb_hip_batch_set_data", what);
    use_device();
    const size_t head = (size_t)s->count * sizeof(nb::AdaptState);
    const size_t log_bytes = dt_log ? (size_t)n * s->count * sizeof(float) : 0;
    if (s->adapt_bytes < head + log_bytes) {   // a regrow carries the records over: a continued call goes on from them
        void *old = s->adapt;
        s->adapt = dev_alloc_bytes(head + log_bytes);
        s->adapt_bytes = head + log_bytes;
        if (old) {
            ASSERT_HIP(hipMemcpyAsync(s->adapt, old, head, hipMemcpyDeviceToDevice, s->stream), "carry the adaptive-step records over");
            ASSERT_HIP(hipStreamSynchronize(s->stream), "sync before freeing the old adaptive-step buffer");
            dev_free(old);
        }
    }
    nb::TimestepParams t;
    memset(&t, 0, sizeof t);
    t.acc = s->acc;
    t.radius = s->radius;
    t.n = s->n;
    t.stride = s->stride;
    t.eta = cfg->eta;
    t.dt_min = cfg->dt_min;
    t.dt_max = cfg->dt_max;
    t.span = cfg->span;
    t.state = static_cast<nb::AdaptState *>(s->adapt);
    t.dt_out = s->dt_dev;
    t.commit = 1;
    float *log = dt_log ? reinterpret_cast<float *>(static_cast<char *>(s->adapt) + head) : nullptr;
    nb::BatchParams p = step_params(s);
    if (!(cfg->flags & NB_ADAPT_CONTINUE) || !s->adapt_armed) nb::launch_arm(s->stream, t.state, s->count);
    s->adapt_armed = true;
    if (cfg->flags & NB_ADAPT_LEAPFROG) {
        // per step: the criterion on the members' own acc writes dt_i[count] to one of two alternating rows, one pass closes
        // step i - 1 with the other row and opens step i with this one, then the force launch; a last pass closes step n - 1
        begin_leapfrog(s, p);
        ASSERT_HIP(hipEventRecord(s->ev[0], s->stream), "event record");
        for (uint32_t i = 0; i < n; i++) {
            t.log = log ? log + (size_t)i * s->count : nullptr;
            t.dt_out = s->lf_dt + (size_t)(i & 1) * s->count;
            nb::launch_ensemble_timestep(s->stream, t, s->count);
            launch_kicks(s, i > 0, true, (i & 1) ^ 1, i & 1);
            launch_force(s, p);
        }
        launch_kicks(s, true, false, (n - 1) & 1, 0);
        s->acc_current = true;
    } else {
        s->acc_current = false;   // Euler steps leave the acc of the state before them
        if (cfg->flags & NB_ADAPT_PRIME) {   // one dt = 0 step of the ordinary path: acc becomes the state's own
            const float zero = 0.0f;
            upload_dts(s, &zero, true);
            launch_steps(s, p, 1);
        }
        ASSERT_HIP(hipEventRecord(s->ev[0], s->stream), "event record");
        for (uint32_t i = 0; i < n; i++) {
            t.log = log ? log + (size_t)i * s->count : nullptr;
            nb::launch_ensemble_timestep(s->stream, t, s->count);
            launch_steps(s, p, 1);
        }
    }
    ASSERT_HIP(hipGetLastError(), "adaptive ensemble launches (%u members of %u particles, %u steps)", s->count, s->n, n);
    ASSERT_HIP(hipEventRecord(s->ev[1], s->stream), "event record");
    s->timed = true;
    s->dt_valid = false;   // the device chose the step sizes: the next fixed-step update uploads its own afresh
    s->adapt_host.resize(head + log_bytes);
    ASSERT_HIP(hipMemcpyAsync(s->adapt_host.data(), s->adapt, head + log_bytes, hipMemcpyDeviceToHost, s->stream),
               "D2H of %u x %u step sizes and the results", n, s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after an adaptive ensemble update");
    for (uint32_t b = 0; out && b < s->count; b++) {
        nb::AdaptState st;
        memcpy(&st, s->adapt_host.data() + (size_t)b * sizeof st, sizeof st);
        out[b] = NbAdaptiveResult{st.t, st.steps, st.idle_steps, st.dt_last, st.dt_smallest};
    }
    if (dt_log) memcpy(dt_log, s->adapt_host.data() + head, log_bytes);
}

double nb_hip_batch_last_ms(SimBatch *s) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (!s->timed) return 0.0;
    use_device();
    ASSERT_HIP(hipEventSynchronize(s->ev[1]), "event sync");
    float ms = 0.0f;
    ASSERT_HIP(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]), "elapsed time");
    return (double)ms;
}

uint32_t nb_hip_batch_dt_uploads(const SimBatch *s) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    return s->dt_uploads;
}

void nb_hip_ensemble_energy(SimBatch *s, WorldEnergy *out) {
    check_diag(s, out, "nb_hip_ensemble_energy");
    constexpr size_t Q = NB_DIAG_SUMS;
    begin_diag(s);
    double *res = energy_slab(s) + (size_t)s->count * nbd::ensemble_tiles(s->n) * Q;
    launch_energy_sums(s, res);
    end_diag(s);
    s->diag_host.resize((size_t)s->count * Q);
    ASSERT_HIP(hipMemcpyAsync(s->diag_host.data(), res, (size_t)s->count * Q * sizeof(double), hipMemcpyDeviceToHost, s->stream),
               "D2H of %u members' energy sums", s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_ensemble_energy");
    for (uint32_t b = 0; b < s->count; b++) nb_energy_from_sums(s->diag_host.data() + (size_t)b * Q, out + b);
}

void nb_hip_ensemble_potential(SimBatch *s, float *phi) {
    check_diag(s, phi, "nb_hip_ensemble_potential");
    nbd::EnsembleDiagParams p = begin_diag(s);
    const size_t total = (size_t)s->offsets[s->count];
    p.phi = grown(s, s->diag_phi, s->diag_phi_cap, total);
    if (s->ragged)
        nbd::launch_ragged_potential(s->stream, p, s->count, s->n_len_dev, s->offsets_dev);
    else
        nbd::launch_ensemble_potential(s->stream, p, s->count);
    ASSERT_HIP(hipGetLastError(), "ensemble_phi_kernel launch (%u members of %u)", s->count, s->n);
    end_diag(s);
    ASSERT_HIP(hipMemcpyAsync(phi, p.phi, total * sizeof(float), hipMemcpyDeviceToHost, s->stream), "D2H of %u members' potentials",
               s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_ensemble_potential");
}

// tuning hook (nbody_hip_tuning.h): device time of the kernels of the last nb_hip_ensemble_energy / _potential
double nb_hip_ensemble_last_diag_ms(SimBatch *s) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (!s->diag_timed) return 0.0;
    use_device();
    ASSERT_HIP(hipEventSynchronize(s->ev_diag[1]), "diagnostics end event");
    float ms = 0.0f;
    ASSERT_HIP(hipEventElapsedTime(&ms, s->ev_diag[0], s->ev_diag[1]), "diagnostics elapsed time");
    return (double)ms;
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

void nb_hip_ensemble_bounds(SimBatch *s, float *bounds) {
    check_not_ragged(s, "nb_hip_ensemble_bounds");
    check_diag(s, bounds, "nb_hip_ensemble_bounds");
    begin_render(s);
    if (!s->render_keys) s->render_keys = dev_alloc<uint32_t>((size_t)s->count * 4);
    nbr::launch_ensemble_bounds(s->stream, s->pos[s->cur], s->n, s->stride, s->count, s->render_keys);
    ASSERT_HIP(hipGetLastError(), "ensemble_bounds_kernel launch (%u members of %u)", s->count, s->n);
    end_render(s);   // the event pair is shared with the renders; render_tile / render_launches speak of renders only
    std::vector<uint32_t> keys((size_t)s->count * 4);
    ASSERT_HIP(hipMemcpyAsync(keys.data(), s->render_keys, keys.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream),
               "D2H of %u members' bounds", s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_ensemble_bounds");
    for (uint32_t b = 0; b < s->count; b++) nb_render_bounds_from_keys(keys.data() + (size_t)b * 4, bounds + (size_t)b * 4);
}

void nb_hip_ensemble_render_counts(SimBatch *s, const RenderView *views, uint32_t *counts) {
    check_not_ragged(s, "nb_hip_ensemble_render_counts");
    check_diag(s, counts, "nb_hip_ensemble_render_counts");
    check_views(s, views, "nb_hip_ensemble_render_counts");
    use_device();
    uint32_t launches = 0;
    enqueue_render(s, views, nullptr, &launches);
    const size_t bytes = (size_t)s->count * NB_RENDER_CLASSES * views[0].width * views[0].height * sizeof(uint32_t);
    ASSERT_HIP(hipMemcpyAsync(counts, s->render_counts, bytes, hipMemcpyDeviceToHost, s->stream), "D2H of %u count images", s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_ensemble_render_counts");
}

void nb_hip_ensemble_render_rgba(SimBatch *s, const RenderView *views, const RenderPalette *palette, uint8_t *rgba) {
    check_not_ragged(s, "nb_hip_ensemble_render_rgba");
    check_diag(s, rgba, "nb_hip_ensemble_render_rgba");
    check_views(s, views, "nb_hip_ensemble_render_rgba");
    NB_ASSERT(palette != nullptr, "nb_hip_ensemble_render_rgba: NULL RenderPalette");
    NB_ASSERT(palette->saturation >= 1u, "RenderPalette saturation must be at least 1");
    use_device();
    uint32_t launches = 0;
    enqueue_render(s, views, palette, &launches);
    const size_t bytes = (size_t)s->count * views[0].width * views[0].height * sizeof(uint32_t);
    ASSERT_HIP(hipMemcpyAsync(rgba, s->render_rgba, bytes, hipMemcpyDeviceToHost, s->stream), "D2H of %u frames", s->count);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "sync after nb_hip_ensemble_render_rgba");
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
    if (!s->render_timed) return 0.0;
    use_device();
    ASSERT_HIP(hipEventSynchronize(s->ev_render[1]), "render end event");
    float ms = 0.0f;
    ASSERT_HIP(hipEventElapsedTime(&ms, s->ev_render[0], s->ev_render[1]), "render elapsed time");
    return (double)ms;
}

void nb_hip_batch_launch_shape(const SimBatch *s, int *path, int *k, int *w, int *lanes, uint32_t *workgroups) {
    NB_ASSERT(s != nullptr, "NULL ensemble");
    if (path) *path = s->path;
    if (k) *k = s->k;
    if (w) *w = s->w;
    if (lanes) *lanes = s->lanes;
    if (workgroups) *workgroups = s->workgroups;
}

}  // extern "C"
