// shard_exchange.hip -- the sharded step: every rank steps its own receivers against all sources, then the ranks exchange
// the source positions they produced with an in-place all-gather -- RCCL, a local group, a caller-supplied host transport or
// direct stores into the peers' arrays -- in-stream or overlapped with the own-shard launch; captured sharded chains; the
// local group (all ranks in this process, one stream: the test transport) and its step call.
#include "pipeline_internal.h"

namespace nbi {

// In-place all-gather of a device array of nranks slots through the caller's host transport: own slot down, wait,
// callback (blocks until every rank's slot is in the staging buffer), everything up.  The stream stays ordered: what
// was enqueued before has completed when the callback runs, what is enqueued after sees the gathered array.
void host_allgather(SimPipeline *s, void *dev_base, size_t bytes_per_rank, hipStream_t st) {
    NB_ASSERT(bytes_per_rank * (size_t)s->nranks <= s->stage_bytes, "staging too small: %zu x %d > %zu", bytes_per_rank, s->nranks,
              s->stage_bytes);
    char *host = static_cast<char *>(s->stage);
    char *dev = static_cast<char *>(dev_base);
    const size_t mine = (size_t)s->rank * bytes_per_rank;
    ASSERT_HIP(hipMemcpyAsync(host + mine, dev + mine, bytes_per_rank, hipMemcpyDeviceToHost, st), "D2H of the own slot");
    ASSERT_HIP(hipStreamSynchronize(st), "sync before the host all-gather");
    s->host_gather(s->host_gather_ctx, host, (uint64_t)bytes_per_rank, s->rank, s->nranks);
    // the own slot never left the device: upload the slots before and after it only (in overlap mode the next step's
    // own-shard launch may already be reading it on the compute stream)
    if (s->rank > 0)
        ASSERT_HIP(hipMemcpyAsync(dev, host, mine, hipMemcpyHostToDevice, st), "H2D of the slots before rank %d's", s->rank);
    if (s->rank + 1 < s->nranks)
        ASSERT_HIP(hipMemcpyAsync(dev + mine + bytes_per_rank, host + mine + bytes_per_rank,
                                  bytes_per_rank * (size_t)(s->nranks - 1 - s->rank), hipMemcpyHostToDevice, st),
                   "H2D of the slots after rank %d's", s->rank);
}

// The direct exchange's data movement: ONE launch reads this rank's slice once and stores it into every peer's gathered
// array (IPC-mapped; over xGMI each peer's stores ride that peer's own link), instead of P - 1 separately submitted
// copies.  16-byte accesses; the slice length is a multiple of 64 float2.
constexpr int DIRECT_PUSH_MAX_PEERS = 15;
struct PushTargets {
    float4 *dst[DIRECT_PUSH_MAX_PEERS];
    int n;
};

__global__ __launch_bounds__(256) void direct_push_kernel(const float4 *__restrict__ src, PushTargets to, uint32_t count4) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count4) return;
    const float4 v = src[i];
    for (int q = 0; q < to.n; q++) to.dst[q][i] = v;
}

void allgather_sources(SimPipeline *s, int buf, hipStream_t st) {
    // in place: this rank's slice already sits at rank * Mc (written by the step kernel's mirror store)
    const size_t per_rank = (size_t)s->plan.mass_chunk * 2;  // floats
    if (per_rank == 0) return;
    float *base = reinterpret_cast<float *>(s->src_pos[buf]);
    if (s->group) {
        // local transport: push the slice into every peer's gathered array (same device, same stream)
        for (SimPipeline *peer : s->group->members) {
            if (peer == s) continue;
            float *dst = reinterpret_cast<float *>(peer->src_pos[buf]);
            ASSERT_HIP(hipMemcpyAsync(dst + (size_t)s->rank * per_rank, base + (size_t)s->rank * per_rank,
                                      per_rank * sizeof(float), hipMemcpyDeviceToDevice, st),
                       "local push of rank %d's sources", s->rank);
        }
        return;
    }
    if (s->direct) {
        // the direct all-gather: this rank's slice goes straight into every peer's gathered array, device to device --
        // over xGMI one copy per peer, each on its own link (no ring, no staging) -- then one host-side barrier: when it
        // opens, every slice of this array has landed everywhere (each rank synchronised its stream before entering it).
        // The ping-pong makes the writes safe: peers write into src_pos[buf] while every rank still reads src_pos[buf ^ 1].
        const size_t off = (size_t)s->rank * per_rank, bytes = per_rank * sizeof(float);
        if (s->nranks - 1 <= DIRECT_PUSH_MAX_PEERS && s->nranks > 1) {
            PushTargets to;
            to.n = 0;
            for (int q = 0; q < s->nranks; q++)
                if (q != s->rank) to.dst[to.n++] = reinterpret_cast<float4 *>(reinterpret_cast<float *>(s->peer_src[buf][(size_t)q]) + off);
            const uint32_t count4 = (uint32_t)(per_rank / 4);   // per_rank floats = Mc float2, Mc a multiple of 64
            hipLaunchKernelGGL(direct_push_kernel, dim3((count4 + 255) / 256), dim3(256), 0, st, reinterpret_cast<const float4 *>(base + off), to, count4);
            ASSERT_HIP(hipGetLastError(), "direct push launch (rank %d, %d peers)", s->rank, to.n);
        } else {
            for (int q = 0; q < s->nranks; q++) {
                if (q == s->rank) continue;
                float *dst = reinterpret_cast<float *>(s->peer_src[buf][(size_t)q]);
                ASSERT_HIP(hipMemcpyAsync(dst + off, base + off, bytes, hipMemcpyDeviceToDevice, st), "direct push of rank %d's sources to rank %d", s->rank, q);
            }
        }
        ASSERT_HIP(hipStreamSynchronize(st), "sync before the step barrier of the direct exchange");
        uint64_t seen[64];
        seen[s->rank] = ++s->direct_steps;
        s->host_gather(s->host_gather_ctx, seen, sizeof(uint64_t), s->rank, s->nranks);
        for (int q = 0; q < s->nranks; q++)
            NB_ASSERT(seen[q] == s->direct_steps, "direct exchange: rank %d is at step %llu, rank %d at %llu", q, (unsigned long long)seen[q], s->rank,
                      (unsigned long long)s->direct_steps);
        return;
    }
    if (s->host_gather) {
        host_allgather(s, base, per_rank * sizeof(float), st);
        return;
    }
    comm_allgather_f32(s, base, per_rank, st, "source positions");
}

// One sharded step of one rank.  `cs` carries the gather (the comm stream with RCCL; the group stream locally).
// `detail`: bracket the step's kernels and its gather with event pairs (plain launches only, not under capture).
void sharded_step(SimPipeline *s, nb::LaunchShape sh, float dt, hipStream_t cs, bool detail) {
    const uint32_t Mc = s->plan.mass_chunk;
    const uint32_t own_lo = (uint32_t)s->rank * Mc, own_hi = own_lo + Mc;
    const int in = s->cur;
    auto mark = [&](hipStream_t st) -> hipEvent_t {
        if (!detail) return nullptr;
        hipEvent_t e = s->pool.next();
        ASSERT_HIP(hipEventRecord(e, st), "record interval event");
        return e;
    };
    if (!s->overlap) {
        // one kernel over all gathered sources, then gather the positions it produced
        const hipEvent_t k0 = mark(s->stream);
        launch_step(s, sh, whole_step(s, in, dt), s->stream);
        const hipEvent_t k1 = mark(s->stream);  // end of the kernels == begin of the gather (same stream)
        allgather_sources(s, in ^ 1, s->stream);
        const hipEvent_t g1 = mark(s->stream);
        if (detail) {
            s->kernel_iv.emplace_back(k0, k1);
            s->comm_iv.emplace_back(k1, g1);
        }
    } else {
        // own-shard sources are already here: start on them while the other P-1 slices of
        // src_pos[in] are still arriving on the comm stream, then finish with the remote ones
        nb::StepParams a = whole_step(s, in, dt);
        a.src_begin[0] = own_lo;
        a.src_end[0] = own_hi;
        a.flags = nb::STEP_NO_FINALIZE;
        a.n_mirror = 0;
        const hipEvent_t a0 = mark(s->stream);
        launch_step(s, sh, a, s->stream);
        const hipEvent_t a1 = mark(s->stream);
        ASSERT_HIP(hipStreamWaitEvent(s->stream, s->ev_gather.get(), 0), "wait gather");
        const hipEvent_t b0 = mark(s->stream);  // stamped once the previous step's gather has landed
        nb::StepParams b = whole_step(s, in, dt);
        b.src_begin[0] = 0;
        b.src_end[0] = own_lo;
        b.src_begin[1] = own_hi;
        b.src_end[1] = s->n_src;
        b.flags = nb::STEP_ACC_IN;
        launch_step(s, sh, b, s->stream);
        const hipEvent_t b1 = mark(s->stream);
        s->ev_local.record(s->stream);
        ASSERT_HIP(hipStreamWaitEvent(cs, s->ev_local.get(), 0), "comm waits for the new slice");
        const hipEvent_t g0 = mark(cs);
        allgather_sources(s, in ^ 1, cs);
        const hipEvent_t g1 = mark(cs);
        s->ev_gather.record(cs);
        if (detail) {
            s->kernel_iv.emplace_back(a0, a1);
            s->kernel_iv.emplace_back(b0, b1);
            s->comm_iv.emplace_back(g0, g1);
        }
    }
    s->cur ^= 1;
}

// Opt-in ("sharded_graph"): the chain of {step kernel(s), in-place all-gather} x n captured from the stream into a
// hipGraph and replayed, like the single-GPU chains.  Only the in-stream (non-overlapped) step is captured; an even
// chain length keeps the ping-pong phase so a cached graph can be replayed as is.  Off by default: RCCL inside
// stream capture is the least-travelled path of this library (exercised with one rank only, tests).
StepGraph *capture_sharded_chain(SimPipeline *s, uint32_t n, float dt, nb::LaunchShape sh) {
    const uint32_t passes = passes_for(s, whole_step(s, s->cur, dt));
    if (StepGraph *c = find_graph(s, n, passes, sh, s->cur)) {
        c->last_use = ++s->use_clock;
        return c;
    }
    evict_for_one_more(s);  // captured RCCL nodes pin communicator resources: the cache stays small
    s->graphs.emplace_back();
    StepGraph *g = &s->graphs.back();
    g->last_use = ++s->use_clock;
    g->n = n;
    g->passes = passes;
    g->phase = s->cur;
    g->shape = sh;
    const int cur0 = s->cur;
    ASSERT_HIP(hipStreamBeginCapture(s->stream, hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
    for (uint32_t i = 0; i < n; i++) sharded_step(s, sh, dt, s->stream);
    ASSERT_HIP(hipStreamEndCapture(s->stream, &g->graph), "hipStreamEndCapture");
    ASSERT_HIP(hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0), "hipGraphInstantiate (sharded, %u steps)", n);
    s->cur = cur0;  // capture only recorded the work; the replay below advances the phase
    return g;
}

void enqueue_sharded(SimPipeline *s, uint32_t n, float dt) {
    NB_ASSERT(s->group == nullptr, "members of a local group step through nb_hip_local_group_step");
    const nb::LaunchShape sh = resolve_shape(s);
    if (s->sharded_graph && !s->overlap && n > 1 && !s->host_gather) {  // a host callback cannot run inside a captured graph
        uint32_t left = n;
        while (left > 0) {
            const uint32_t chunk = left > GRAPH_CHAIN_MAX ? GRAPH_CHAIN_MAX : left;
            StepGraph *g = capture_sharded_chain(s, chunk, dt, sh);
            ASSERT_HIP(hipGraphLaunch(g->exec, s->stream), "hipGraphLaunch (sharded, %u steps)", chunk);
            if (chunk & 1) s->cur ^= 1;
            left -= chunk;
        }
        return;
    }
    // per-step event pairs only when the caller asked for timing: up to ~1000 hipEventRecord per call otherwise for nothing
    for (uint32_t i = 0; i < n; i++) sharded_step(s, sh, dt, s->comm_stream, s->timing != 0 && i < DETAIL_STEPS_MAX);
    s->detail_steps = s->timing ? (n < DETAIL_STEPS_MAX ? n : DETAIL_STEPS_MAX) : 0;
    if (s->overlap) ASSERT_HIP(hipStreamWaitEvent(s->stream, s->ev_gather.get(), 0), "join comm stream");
}

}  // namespace nbi

using namespace nbi;

extern "C" {

int nb_hip_local_group_create(WorldData data, int nranks, SimPipeline **out) {
    NB_ASSERT(nranks >= 1 && out != nullptr, "bad local group request");
    use_device();
    LocalGroup *g = new LocalGroup();
    ASSERT_HIP(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking), "group stream");
    for (int r = 0; r < nranks; r++) {
        SimPipeline *s = CreateSimPipeline(data);
        s->rank = r;
        s->nranks = nranks;
        s->sharded = true;
        s->group = g;
        s->plan = nb_hip_shard_plan(data.total_len, data.mass_len, r, nranks);
        g->members.push_back(s);
        out[r] = s;
    }
    return nranks;
}

void nb_hip_local_group_step(SimPipeline **sims, int nranks, uint32_t n, float dt) {
    NB_ASSERT(sims != nullptr && nranks >= 1 && sims[0]->group != nullptr, "not a local group");
    LocalGroup *g = sims[0]->group;
    NB_ASSERT((int)g->members.size() == nranks, "group has %zu members, %d passed", g->members.size(), nranks);
    for (int r = 0; r < nranks; r++) NB_ASSERT(sims[r]->on_device, "member %d has no data", r);
    use_device();
    for (int r = 0; r < nranks; r++) {
        SimPipeline *s = sims[r];
        s->pool.used = 0;
        s->kernel_iv.clear();
        s->comm_iv.clear();
        s->detail_steps = 0;
        upload_dt(s, dt);
    }
    // with the "timing" knob every member's kernels and pushes get their own event pairs, so that
    // nb_hip_last_step_breakdown(member) says what ONE rank's shard step costs (bench.py S2 / S4 / S8)
    for (uint32_t i = 0; i < n; i++)
        for (int r = 0; r < nranks; r++) {
            SimPipeline *s = sims[r];
            sharded_step(s, resolve_shape(s), dt, g->stream, s->timing != 0 && i < DETAIL_STEPS_MAX);
        }
    for (int r = 0; r < nranks; r++) {
        SimPipeline *s = sims[r];
        s->detail_steps = s->timing ? (n < DETAIL_STEPS_MAX ? n : DETAIL_STEPS_MAX) : 0;
        s->step_iv.clear();   // no whole-chain event pair for group members; the breakdown has its own
    }
    ASSERT_HIP(hipStreamSynchronize(g->stream), "group sync");
}

}  // extern "C"
