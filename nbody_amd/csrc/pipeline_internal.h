// pipeline_internal.h -- what the translation units behind include/nbody_hip.h share (C++, not part of the C-ABI):
//
//   this header      besides the two structs' shared declarations: DevBuf<T>, DevEvent and Interval, the owner types every
//                    device array, event and timed interval of a SimPipeline / SimBatch is a member of.  Nothing in these files
//                    frees device memory or destroys an event by hand: the member's destructor does, when the struct is deleted.
//                    And ReadScratch / read_call: the one scratch and the one host protocol of every read-only call below
//   device_ctx.hip   the process-wide device context (the reference keeps one global vulkan_ctx, vulkan_ctx.c:11); the one
//                    allocation seam (dev_alloc_bytes / dev_free) and the counters behind nb_hip_live_resources
//   rccl_bind.hip    RCCL bound lazily with dlopen, the communicator of a sharded pipeline, the watchdog
//   shard_plan.hip   nb_hip_shard_plan: who owns which receivers and sources (pure host arithmetic)
//   step_chain.hip   one step / n fixed Euler steps as launches: the launch plan, cached hipGraph chains, the one-workgroup chain
//   shard_exchange.hip  the sharded step: the four transports of its in-place all-gather, captured sharded chains
//   step_schedule.hip   device-chosen and leapfrog steps of a pipeline: the target of step_schedule.h's one launch schedule
//   pipeline.hip     SimPipeline life cycle and the C-ABI entry points (Create/Destroy/Set/Get/PerformSimUpdate, knobs);
//                    release_device ends what no owner type holds: streams, cached graphs, IPC mappings, pinned host memory
//   kernels.hip      the gfx950 force kernels and their entry points (kernels.h); each ensemble kernel once, instantiated
//                    for the two ways a launch finds its members (by block index / through a ragged ensemble's tables)
//   launch_shape.hip the host-side launch policy: shape, grid, LDS of a launch (launch_shape.h)
//   convert.hip      AoS <-> SoA converters, pads, G*m, fills (convert.h)
//   batch.hip        SimBatch (batch_internal.h): ensembles of small worlds, uniform or ragged, stepped by one launch
//                    (nb_hip_batch_*, nb_hip_ragged_*): one constructor, and the target of ensemble_walk.h's one launch walk
//                    (host only, no HIP) for every fixed step; their traced, adaptive and leapfrog updates (the ensemble's
//                    target of step_schedule.h)
//   batch_observe.hip  the read-only calls on a SimBatch: energy, potential, the field calls, bounds, count images and frames
//   diagnostics.hip  energy / momentum / potential of the state a pipeline holds (nb_hip_energy, nb_hip_potential)
//   batch_diag.hip   the same for every member of a SimBatch, uniform or ragged: the kernels behind nb_hip_ensemble_energy / _potential
//                    (batch_diag.h; the arithmetic both share: diag_common.h)
//   render.hip       bounds, count image and RGBA frame of the state a pipeline holds (nb_hip_bounds, nb_hip_render_*)
//   render_kernels.hip  the render kernels of a world and of an ensemble, what they share written once, and their launchers (render_kernels.h)
//   field.hip        the potential and the acceleration at probe points and as maps over a view (nb_hip_potential_at,
//                    nb_hip_potential_map, nb_hip_acceleration_at, nb_hip_acceleration_map): one sampler, two pair statements
//                    (the kernel templates and the host side of a call: field_sampler.h)
//   tidal.hip        the tidal tensor at the same places, for a pipeline and for an ensemble (nb_hip_tidal_at, nb_hip_tidal_map;
//                    the kernels behind nb_hip_ensemble_tidal_at / _tidal_map): the sampler's third pair statement
//   profile.hip      radial profiles of a pipeline and of every member of an ensemble (nb_hip_profile, nb_hip_ensemble_profile): the
//                    chunk, reduce and ensemble kernels and their entry points (the statement: profile_common.h)
//   paircount.hip    pair-separation counts of a pipeline and of every member of an ensemble (nb_hip_pair_counts,
//                    nb_hip_ensemble_pair_counts): one kernel and its entry points (the statement: paircount_common.h)
//   neighbour.hip    the nearest neighbour and the neighbour count of every particle of a pipeline and of every member of an
//                    ensemble (nb_hip_neighbours, nb_hip_ensemble_neighbours): one kernel template, its span policy and its
//                    entry points (the statement: neighbour_common.h)
//   group.hip        the friends-of-friends groups of a pipeline and of every member of an ensemble (nb_hip_groups,
//                    nb_hip_ensemble_groups): the init, pair and flatten kernels, the span policy and the entry points (the
//                    statement and the union-find: group_common.h)
//   timestep.hip     the adaptive step size: the criterion kernels between two step launches (timestep.h, timestep_common.h)
//   leapfrog.hip     the kick / drift passes of a kick-drift-kick step around a dt = 0 force launch (leapfrog.h, leapfrog_common.h)
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "convert.h"
#include "kernels.h"
#include "launch_shape.h"
#include "nbody_hip.h"

// ---- error convention: print where, abort (reference src/lib/util.h:17-29,47-60) -------------------------

#define NB_FAIL(...)                                                          \
    do {                                                                      \
        fprintf(stderr, "%s:%d [%s] ", __FILE__, __LINE__, __func__);         \
        fprintf(stderr, __VA_ARGS__);                                         \
        fprintf(stderr, "\n");                                                \
        abort();                                                              \
    } while (0)

#define NB_ASSERT(COND, ...)               \
    do {                                   \
        if (!(COND)) NB_FAIL(__VA_ARGS__); \
    } while (0)

#define ASSERT_HIP(X, ...)                                                                              \
    do {                                                                                                \
        hipError_t nb_e_ = (X);                                                                         \
        if (nb_e_ != hipSuccess) {                                                                      \
            fprintf(stderr, "%s:%d [%s] hipError_t = %d, str = %s\n", __FILE__, __LINE__, __func__,     \
                    (int)nb_e_, hipGetErrorString(nb_e_));                                              \
            NB_FAIL(__VA_ARGS__);                                                                       \
        }                                                                                               \
    } while (0)

#define NB_HIDDEN __attribute__((visibility("hidden")))   // not among the library's exported symbols

typedef struct ncclComm *ncclComm_t;  // opaque; rccl_bind.hip holds the rest of the binding

namespace nbi {

// ---- device_ctx.hip ------------------------------------------------------------------------------------------

struct DeviceCtx {
    bool ready = false;
    int ordinal = -1;  // -1: not chosen yet
    int compute_units = 0;
    char info[256] = {0};
};
extern DeviceCtx g_dev;
extern int g_requested_ordinal;

void ensure_device();  // first touch of the GPU by this process; aborts unless a gfx950 device answers (no CPU fallback)
void use_device();     // ensure_device + hipSetDevice on the calling thread (HIP's current device is per THREAD)
void *dev_alloc_bytes(size_t bytes);
void dev_free(void *p);   // NULL: no HIP call
// what nb_hip_live_resources reports: device allocations and events alive in the process (plain host counters)
extern NB_HIDDEN std::atomic<uint32_t> g_live_buffers, g_live_events;

// libc's rand() stream belongs to the caller: the reference harness seeds it ONCE and draws every universe of its table
// from it (src/bench.c:42,53), between GPU calls.  The HIP runtime's first stream / allocation / code-object set-up
// draws from (or reseeds) that same process-global state -- measured: tools/rand_probe.py, profiles/r04_rand_probe.txt --
// so the first device set-up of a pipeline and RCCL's bootstrap run with a private state swapped in.
// initstate / setstate swap ONE process-global pointer, so two guards that each saved "the previous state" would hand each
// other's private state back to the caller.  The guard is therefore reference-counted process-wide: the FIRST guard to
// come alive saves the caller's state and installs the private one, the LAST to go restores it; the mutex is held only
// for that bookkeeping, never across the guarded region.  That matters because a guarded region can WAIT ON OTHER RANKS
// (the direct exchange's IPC-handle hand-over and "ready" barrier run through the caller's all-gather callback inside the
// first SetSimulationData; ncclCommInitRank blocks until every rank has joined): ranks driven from threads of one process
// would deadlock on a lock held across such a wait (round 5 held one).  Guards nest freely on one thread.
// A caller's own rand() racing a live guard on another thread is the caller's race: libc's rand() stream is one
// process-global object to begin with (tests/test_abi.py pins the two-thread and the wait-inside-a-guard cases).
class RandGuard {
  public:
    RandGuard() {
        std::lock_guard<std::mutex> l(gate());
        if (alive()++ == 0) saved() = initstate(1u, private_state(), 128);
    }
    ~RandGuard() {
        std::lock_guard<std::mutex> l(gate());
        if (--alive() == 0 && saved()) {
            setstate(saved());
            saved() = nullptr;
        }
    }
    RandGuard(const RandGuard &) = delete;
    RandGuard &operator=(const RandGuard &) = delete;

  private:
    static std::mutex &gate() {
        static std::mutex m;
        return m;
    }
    static int &alive() {   // guards alive in the process, any thread; guarded by gate()
        static int n = 0;
        return n;
    }
    static char *&saved() {   // the caller's state while alive() > 0
        static char *p = nullptr;
        return p;
    }
    static char *private_state() {
        static char buf[128];
        return buf;
    }
};

template <typename T>
T *dev_alloc(size_t count) {
    return static_cast<T *>(dev_alloc_bytes((count ? count : 1) * sizeof(T)));
}

inline uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// ---- the owners: every device buffer and every event of the seam is a member of one of these three types, and is released
// by that member's destructor -- once, when its SimPipeline / SimBatch / calling function goes, after whoever deletes the
// owner has drained its streams.  One that was never made makes no HIP call when it goes.

// A device array: a pointer and an element count.  Reads as a plain T * wherever a parameter block is filled.
template <typename T>
class NB_HIDDEN DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { dev_free(p_); }

    operator T *() const { return p_; }
    size_t count() const { return n_; }   // elements asked for (0 before alloc)

    T *alloc(size_t count) {   // once
        NB_ASSERT(p_ == nullptr, "device array made twice");
        n_ = count;
        return p_ = dev_alloc<T>(count);
    }
    // Scratch grown on demand: at least `need` elements afterwards, exactly `need` when it had to be made anew.  The old
    // contents go (work queued on `st` may still read them: it is drained first).  True when the array moved.
    bool grown(hipStream_t st, size_t need) { return regrow(st, need, 0); }
    // The same for an array whose first `head` bytes are records a continued call goes on from: they are carried over.
    bool grown_carrying(hipStream_t st, size_t need, size_t head) { return regrow(st, need, head); }

  private:
    bool regrow(hipStream_t st, size_t need, size_t head) {
        if (p_ && n_ >= need) return false;
        T *old = p_;
        p_ = nullptr;
        if (old && head == 0) {
            ASSERT_HIP(hipStreamSynchronize(st), "sync before regrowing a scratch buffer");
            dev_free(old);
            old = nullptr;
        }
        alloc(need);
        if (old) {
            ASSERT_HIP(hipMemcpyAsync(p_, old, head, hipMemcpyDeviceToDevice, st), "carry the head of a regrown buffer over");
            ASSERT_HIP(hipStreamSynchronize(st), "sync before freeing the old buffer");
            dev_free(old);
        }
        return true;
    }
    T *p_ = nullptr;
    size_t n_ = 0;
};

// An event, created on first use with the flags given.
class NB_HIDDEN DevEvent {
  public:
    explicit DevEvent(unsigned flags = hipEventDefault) : flags_(flags) {}
    DevEvent(DevEvent &&o) noexcept : ev_(o.ev_), flags_(o.flags_) { o.ev_ = nullptr; }
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    ~DevEvent() {
        if (!ev_) return;
        ASSERT_HIP(hipEventDestroy(ev_), "event");
        g_live_events--;
    }
    hipEvent_t get() {
        if (!ev_) {
            ASSERT_HIP(hipEventCreateWithFlags(&ev_, flags_), "event");
            g_live_events++;
        }
        return ev_;
    }
    void record(hipStream_t st) { ASSERT_HIP(hipEventRecord(get(), st), "event record"); }

  private:
    hipEvent_t ev_ = nullptr;
    unsigned flags_;
};

// device time between two recorded events, once the later one has completed
inline double elapsed_ms(hipEvent_t ev0, hipEvent_t ev1) {
    ASSERT_HIP(hipEventSynchronize(ev1), "end event");
    float ms = 0.0f;
    ASSERT_HIP(hipEventElapsedTime(&ms, ev0, ev1), "elapsed time");
    return (double)ms;
}

// A timed interval of stream work: two events and whether the pair was recorded by the last call that could have.
class NB_HIDDEN Interval {
  public:
    void begin(hipStream_t st) { first.record(st); }
    void end(hipStream_t st) { last.record(st), valid_ = true, ms_ = -1.0; }
    void clear() { valid_ = false; }   // the last call had nothing to time
    bool valid() const { return valid_; }
    double ms() { return !valid_ ? 0.0 : ms_ >= 0.0 ? ms_ : (ms_ = elapsed_ms(first.get(), last.get())); }
    DevEvent first, last;

  private:
    bool valid_ = false;
    double ms_ = -1.0;   // of the pair as recorded, kept from the first query (below 0: none yet): hipEventElapsedTime asked again moves by a ns
};

// The scratch of every read-only call of a SimPipeline / SimBatch -- energy, potential, the six field calls, profile, pair counts,
// neighbours, groups, bounds, count image, frame: sixteen.  Each ends in a stream sync before it returns, so no two are ever in flight and
// one set serves them all.  A call finds in it whatever the last call of any kind left, so it reads only what it wrote or reset
// itself.  Energy, potential, the field calls and profile only store.  Pair counts zero the table they add into; neighbours set
// the keys they take minima into to all ones and zero the counts a radius asks for; groups set the table they hook into to the identity.  Bounds: a pipeline's two memsets set its four
// keys to the identities of min and max; an ensemble's workgroups store each member's four.  Count image and frame: the image added
// into and the disc cursor are zeroed by memset (an ensemble's global path: by one), only discs[0 .. cursor) is ever read, the shade
// stores every pixel of the frame; an ensemble's tile path builds the image in LDS and stores every word of the counts, or frame.
struct NB_HIDDEN ReadScratch {
    DevBuf<char> args;        // what a call uploads
    DevBuf<char> work;        // what its kernels write: workspace and result, in the call's own layout (several arrays: section())
    std::vector<char> host;   // where the copied-back bytes land when the caller's array has another layout
    Interval iv;              // around the last call's launches and memsets (nb_hip_last_diag_ms / nb_hip_ensemble_last_diag_ms), but
                              // for bounds and renders, which bracket render_iv / bounds_iv.  A call with nothing to launch (no probe;
                              // no neighbour receiver or source under the masks; no pair that could link) returns its defaults, clears it and stops there
};

// the next section of a call's `work`, on a 256-byte boundary: its offset; `end` moves past it and ends as the size to ask for
inline size_t section(size_t &end, size_t bytes) { return std::exchange(end, end + (bytes + 255) / 256 * 256); }

// The protocol of every read-only call on s (a SimPipeline or a SimBatch: its `read` and its `stream`), written once: grow the two
// buffers (never shrunk; the stream is drained before one moves), upload `args`, then inside the interval `iv` `enqueue(args on the
// device, work)` launches the call's kernels and returns where on the device the bytes to copy back start, one copy of `back_bytes`
// to `dst` -- null: to read.host -- and one sync.  Returns where the bytes landed.  `args` stays alive until then.  A size of 0 leaves
// that buffer alone.  tests/sequence_driver.py (the reads kinds) issues all the calls in drawn orders on one long-lived object.
template <class Owner, class Enqueue>
void *read_call(Owner *s, Interval &iv, const char *what, const void *args, size_t args_bytes, size_t work_bytes, void *dst,
                size_t back_bytes, Enqueue enqueue) {
    ReadScratch &r = s->read;
    use_device();
    if (args_bytes) r.args.grown(s->stream, args_bytes);
    if (work_bytes) r.work.grown(s->stream, work_bytes);
    if (args_bytes)
        ASSERT_HIP(hipMemcpyAsync(r.args, args, args_bytes, hipMemcpyHostToDevice, s->stream), "%s: H2D of %zu bytes", what, args_bytes);
    iv.begin(s->stream);
    const void *from = enqueue(static_cast<void *>(r.args), static_cast<void *>(r.work));
    iv.end(s->stream);
    if (!dst) {
        if (r.host.size() < back_bytes) r.host.resize(back_bytes);   // never shrunk either: a resize back up would zero-fill
        dst = r.host.data();
    }
    ASSERT_HIP(hipMemcpyAsync(dst, from, back_bytes, hipMemcpyDeviceToHost, s->stream), "%s: D2H of %zu bytes", what, back_bytes);
    ASSERT_HIP(hipStreamSynchronize(s->stream), "%s: sync", what);
    return dst;
}

// ---- rccl_bind.hip -------------------------------------------------------------------------------------------

// A collective that never completes (a rank that died, a fabric that does not come up) must not hang the job: every
// call that waits on other ranks -- ncclCommInitRank, the first all-gather, and the blocking waits of a sharded
// pipeline (PerformSimUpdate's sync, the collective GetSimulationData) -- runs under a watchdog that prints what was
// being waited for, the tail of RCCL's own log when NCCL_DEBUG_FILE names one, and _exit(3)s.  No retry and no
// re-exec: the process has initialised the GPU.  NB_HIP_COMM_TIMEOUT_S (default 180) sets the bound; 0 disables it.
// One long-lived thread per process does the watching; a Watchdog object only adds its deadline to the watcher's list and
// takes it off again (a mutex and a notify: a frame loop of short sharded calls does not pay a thread spawn + join per
// sync).  Waits nest per THREAD (an inner wait keeps the outer deadline); waits on different threads are each watched.
class Watchdog {
  public:
    Watchdog(const char *what, int rank, int nranks);
    ~Watchdog();
    Watchdog(const Watchdog &) = delete;
    Watchdog &operator=(const Watchdog &) = delete;

  private:
    uint64_t seq_ = 0;   // 0: not armed by this object (disabled, or an outer wait of the same thread is being watched)
};

// ncclCommInitRank + cross-check of the communicator's own rank count + a verified probe all-gather, all bounded
void comm_create(::SimPipeline *s, const void *unique_id128);
void comm_destroy(::SimPipeline *s);
// in-place ncclAllGather of `count` floats per rank (sendbuff = recvbuff + rank * count) on `st`
void comm_allgather_f32(::SimPipeline *s, void *base, size_t count_per_rank, hipStream_t st, const char *what);

// ---- a cached chain of step launches ---------------------------------------------------------------------------

struct StepGraph {
    uint32_t n = 0;           // steps in the chain
    uint32_t passes = 1;      // source passes per step
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    std::vector<hipGraphNode_t> nodes;  // one kernel node per launch, in order
    std::vector<nb::StepParams> params; // what each node currently holds
    int phase = -1;                     // which pos buffer the chain reads first
    nb::LaunchShape shape;
    uint32_t dealt_groups = 0;          // workgroups of its dealt step launches (items + extra); 0: classic launches
    uint64_t last_use = 0;              // for eviction: the cache holds at most GRAPH_CACHE_MAX chains
};

// Event pairs around the kernels and the gathers of a sharded chain (the plain-launch path, "timing" knob on), so that
// a multi-GPU run can say how much of a step was the all-gather.  Grown on demand, reused by every call.
struct EventPool {
    std::vector<DevEvent> ev;
    size_t used = 0;
    hipEvent_t next() {
        if (used == ev.size()) ev.emplace_back();
        return ev[used++].get();
    }
};

}  // namespace nbi

struct LocalGroup {
    std::vector<SimPipeline *> members;
    hipStream_t stream = nullptr;  // every member enqueues here, so program order is the only ordering needed
};

struct SimPipeline {
    WorldData data;
    // sharding (nranks == 1: the whole world on one device)
    int rank = 0, nranks = 1;
    bool sharded = false;  // RCCL path (nranks > 1, or forced for single-GPU testing of that path)
    NbShardPlan plan;
    ncclComm_t comm = nullptr;
    struct LocalGroup *group = nullptr;  // test transport: all ranks are pipelines of this process (no RCCL)
    // caller-supplied transport (CreateSimPipelineShardedWith): an in-place all-gather over HOST memory; the pipeline
    // stages each exchange through one page-locked buffer (D2H own slot, wait, callback, H2D the other ranks' slots)
    NbAllGatherFn host_gather = nullptr;
    void *host_gather_ctx = nullptr;
    void *stage = nullptr;        // page-locked staging, max(gathered sources, gathered particle slices) bytes
    size_t stage_bytes = 0;
    // direct transport (CreateSimPipelineShardedDirect): the per-step exchange is P - 1 device-to-device copies of this
    // rank's slice straight into every peer's gathered array (mapped with hipIpcOpenMemHandle: over xGMI each copy rides
    // its own link), then a host-side step barrier through the caller's callback.  peer_src[b][q] = rank q's src_pos[b]
    // as seen from this process (own entry = the local array).
    bool direct = false;
    std::vector<float2 *> peer_src[2];
    uint64_t direct_steps = 0;    // exchanges done: the ranks compare it at every barrier

    bool on_device = false;  // buffers exist and hold data
    uint32_t slots = 0;      // receiver slots on this device (allocation; includes a shard's pad slots)
    uint32_t n_real = 0;     // receivers actually computed (== slots when unsharded)
    uint32_t n_src = 0;      // sources every receiver sees (mass_len, or the padded gathered length)

    // SoA streams (DESIGN.md "Layout in HBM")
    nbi::DevBuf<float2> pos[2];
    nbi::DevBuf<float2> vel, acc;
    nbi::DevBuf<float> radius, mass;
    // the sources of a step (ping-pong): a view of pos[] when unsharded (the first mass_len receivers ARE the sources), of
    // the gathered source positions when sharded
    float2 *src_pos[2] = {nullptr, nullptr};
    nbi::DevBuf<float2> gathered[2];
    nbi::DevBuf<float> src_gm;
    // the step size lives in device memory, like the reference's uniform block (sim_gpu.h:8-12): kernels read it
    // through StepParams::dt, a new value is written in stream order when PerformSimUpdate's dt differs from the last
    // one enqueued (the reference's re-upload, sim_gpu.c:268-284), and no cached hipGraph ever needs re-patching
    nbi::DevBuf<float> dt_dev;
    float dt_enqueued = 0.0f;
    bool dt_valid = false;
    uint32_t dt_uploads = 0;
    nbi::DevBuf<Particle> aos;        // device AoS staging for Set/Get (whole world)
    nbi::DevBuf<Particle> aos_shard;  // sharded only: every rank's slice, uniform size
    void *host_array = nullptr;  // caller's long-lived particle array (nb_hip_note_host_array), page-locked lazily
    size_t host_bytes = 0;
    bool host_pinned = false;
    void *host_dev = nullptr;    // device-side address of the page-locked array (kernels store to it over PCIe)
    // eager read-back (knob "readback"): in a frame loop -- every blocking update followed by a Get into the noted
    // array -- the merge kernel of the NEXT Get is appended to the update's own submission and stores straight into the
    // noted array, so the Get finds its data already there: one submission + one wait per frame instead of two
    // (step + wait, then merge + D2H copy + wait).  Frozen since round 2: the GUI it serves is out of scope.
    int readback = 2;             // 0 never, 1 after every blocking update, 2 auto (after two update->Get pairs in a row)
    int zero_copy_upload = 1;     // SetSimulationData from the noted array: the split kernel reads host memory directly
    bool host_current = false;    // the noted array already holds the device's latest state
    uint32_t updates_since_get = 0, frame_streak = 0;
    // record the step interval around every chain (nb_hip_last_step_ms) and, on the sharded plain-launch path,
    // the per-step kernel / gather event pairs (nb_hip_last_step_breakdown).  Off unless asked for: the records cost an
    // interactive caller 3-7 us per call (profiles/r02_frame_loop_latency.txt).
    int timing = 0;
    nbi::DevBuf<float2> parts;      // split steps only: [split][n_real] partial sums
    nbi::DevBuf<uint32_t> tickets;  // fused finish: one arrival counter per receiver tile, zero between launches (re-zeroed at every upload
                                    // and before a chain is built: a launch that ended part-way must not leave a tile unfinished for ever)
    int fused_finish = 2;         // 0: step kernel + finish kernel; 1: the last workgroup of a tile finishes it, whenever
                                  // the shape allows; 2 (default): auto (launch_shape.hip fused_finish_rule)
    nbi::DevBuf<uint32_t> deal_counter;   // dealt launches: the ticket counter, zero between launches (zeroed with the tickets); unsharded only
    int deal = 2;                 // 0: classic launches; 1: dealt whenever the shape allows; 2 (default): auto (step_chain.hip deal_applies)
    int want_deal_extra = 0;      // workgroups a dealt launch holds on top of its items; 0 = launch_shape.hip deal_extra
    uint32_t last_deal_items = 0, last_deal_extra = 0;   // what the last resolved step launches: 0 items = not dealt
    int cur = 0;             // pos[cur] is the latest state

    hipStream_t stream = nullptr;
    hipStream_t comm_stream = nullptr;
    nbi::Interval step_iv;   // around the last chain, when the "timing" knob was on
    nbi::DevEvent ev_local{hipEventDisableTiming}, ev_gather{hipEventDisableTiming};   // sharded: what orders stream and comm stream
    uint32_t timed_launches = 0;         // step-kernel launches inside step_iv
    uint32_t timed_finish_launches = 0;  // finish-kernel launches in the same interval (split shapes only)
    // sharded plain-launch chains: [begin, end) event pairs of each step's kernels and of each gather
    nbi::EventPool pool;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> kernel_iv, comm_iv;
    uint32_t detail_steps = 0;  // steps the intervals above cover (capped)
    uint64_t use_clock = 0;     // ticks once per graph lookup (LRU)

    // knobs
    // the launch shape asked for ("variant" knob, shape hooks; launch_shape.h LaunchShape): all auto by default -- the
    // scalar-cache route is 8 % faster than LDS tiles at N = 2^20 (roofline.alt_lds)
    nb::LaunchShape want;
    int use_graph = 2, overlap = 0, sharded_graph = 0;  // use_graph: 0 never, 1 always, 2 from a chain length's second use
    int fused_chain = 2;                                // one-launch n-step chains for one-workgroup worlds: 0 never, 2 auto
    std::vector<uint32_t> seen_chains;                  // chain lengths already run once as plain launches
    int want_passes = 0;  // source passes per step (0 = auto: keep each pass's sources within one XCD's L2)
    double first_gather_ms = 0.0;  // sharded: device time of the probe all-gather at creation (includes lazy setup)
    double comm_init_ms = 0.0;     // sharded over RCCL: host time of ncclCommInitRank
    double small_gather_us = 0.0;  // sharded over RCCL: device time of one warm 8-byte-per-rank all-gather (mean of 16 in-stream)
    nb::LaunchShape last_shape = {.variant = nb::VARIANT_LDS};   // all zero until the first step
    uint32_t last_groups = 0;
    uint32_t fused_steps = 0;   // steps the last update ran inside fused (one-launch) chains

    std::vector<nbi::StepGraph> graphs;

    // every read-only call (diagnostics, field, tidal, profile, paircount, neighbour, group, render .hip): its scratch; all but render.hip's: its interval
    nbi::ReadScratch read;

    nbi::Interval render_iv, bounds_iv;    // render.hip's own: around the last render and the last nb_hip_bounds (nb_hip_last_render_ms)
    nbi::DevEvent ev_splat, ev_disc;       // inside render_iv: after the splat, after the disc pass ("render_detail")
    bool render_detailed = false;          // the last render recorded those two
    int render_merge = 1, render_detail = 0;   // tuning hooks (nbody_hip_tuning.h)

    // field.hip, tidal.hip (nb_hip_potential_at / _map, nb_hip_acceleration_at / _map, nb_hip_tidal_at / _map)
    int field_shape = 0;           // tuning hooks, Phi, g and T: 0 auto, 1 source split, 2 one wave per tile
    int gravity_shape = 0;
    int tidal_shape = 0;

    // adaptive steps (step_schedule.hip enqueue_adaptive; kernels: timestep.hip): one device buffer grown on demand --
    // ADAPT_HEAD bytes of records (the call's AdaptState, the record and result of nb_hip_timestep), then the call's log
    nbi::DevBuf<char> adapt;
    bool adapt_armed = false;        // the call record holds a call to continue (NB_ADAPT_CONTINUE)
    uint32_t adapt_logged = 0;       // steps of the last adaptive call: what nb_hip_adaptive_collect copies back
    std::vector<char> adapt_host;    // where that copy lands

    // leapfrog steps (step_schedule.hip enqueue_leapfrog; kernels: leapfrog.hip).  Their step sizes live in two words of the
    // adaptive head (LEAPFROG_WORDS): a fixed-step call uses the first, an adaptive one alternates so that one launch can
    // close step i - 1 and open step i.
    bool acc_current = false;        // acc = F(x) of the state held: true after a leapfrog call, false after anything else that moves it
    uint32_t lf_force_launches = 0;  // force evaluations of the last leapfrog call (nb_hip_last_leapfrog_info)
    bool lf_primed = false;          // ... and whether it had to run one first
};

namespace nbi {

// ---- step_chain.hip ------------------------------------------------------------------------------------------

constexpr uint32_t CANON_STEPS = 32;  // length of the prebuilt chain of small worlds (see wants_canonical)
constexpr uint32_t CHAIN_MAX_STEPS_PER_LAUNCH = 1u << 16;   // steps one launch of the one-workgroup chain runs (batch.hip too)
constexpr uint32_t DETAIL_STEPS_MAX = 256;  // steps per call whose kernels / gathers get their own event pairs

void destroy_graph(StepGraph &g);
nb::LaunchShape resolve_shape(SimPipeline *s);
bool wants_canonical(const SimPipeline *s);
StepGraph *find_graph(SimPipeline *s, uint32_t n, uint32_t passes, nb::LaunchShape sh, int phase);
StepGraph *find_or_build_graph(SimPipeline *s, uint32_t n, float dt, nb::LaunchShape sh);
void evict_for_one_more(SimPipeline *s);   // the least recently used cached chain goes once the cache is full
constexpr uint32_t GRAPH_CHAIN_MAX = 64;   // longer requests replay an even-length chain
// the single-kernel step that reads phase `in` and writes phase `in ^ 1`; its source passes; its launches
nb::StepParams whole_step(const SimPipeline *s, int in, float dt);
uint32_t passes_for(const SimPipeline *s, const nb::StepParams &p);
void launch_step(SimPipeline *s, nb::LaunchShape sh, const nb::StepParams &p, hipStream_t st);
void upload_dt(SimPipeline *s, float dt);
void zero_tickets(SimPipeline *s);   // fused finish: all tile tickets back to 0, in stream order; and the deal counter
bool deal_applies(const SimPipeline *s, nb::LaunchShape sh);   // "deal" knob: this shape's step launches are dealt
// what every step call starts and ends with: the per-call records cleared; the end of step_iv and the launch counts of the timed interval
void begin_call(SimPipeline *s);
void end_call(SimPipeline *s, uint32_t launches);
void enqueue_steps(SimPipeline *s, uint32_t n, float dt);  // what PerformSimUpdate / nb_hip_step_async enqueue

// ---- shard_exchange.hip --------------------------------------------------------------------------------------

// one sharded step of one rank; `cs` carries the gather (the comm stream with RCCL; the group stream locally)
void sharded_step(SimPipeline *s, nb::LaunchShape sh, float dt, hipStream_t cs, bool detail = false);
// in-place all-gather of a device array of nranks slots through the caller's host transport
void host_allgather(SimPipeline *s, void *dev_base, size_t bytes_per_rank, hipStream_t st);
void enqueue_sharded(SimPipeline *s, uint32_t n, float dt);

// ---- step_schedule.hip ---------------------------------------------------------------------------------------

// the part of an adaptive call's checks a pipeline and an ensemble share: NULL arguments, the NbAdaptive's fault, the step count
void check_adaptive_cfg(const void *s, uint32_t n, const NbAdaptive *cfg, const char *what);

// ---- diagnostics.hip -----------------------------------------------------------------------------------------

void check_diag(SimPipeline *s, const char *what);   // every read-only call: aborts on NULL, on a sharded pipeline and before SetSimulationData

// ---- render.hip ----------------------------------------------------------------------------------------------

void check_view(const RenderView *view);   // a render's or a map's one view: aborts on NULL and on nb_render_view_fault

}  // namespace nbi
