// timestep.hip -- the adaptive step size of include/nbody_adaptive.h on the device: a small reduction between two step
// launches that writes the next step's dt where that launch reads it (StepParams::dt, BatchParams::dt[count]), so n adaptive
// steps need no host round trip.
//
//   timestep_kernel            one world.  A bounded grid (at most four workgroups per XCD) walks acc and radius grid-stride
//                              with coalesced loads, takes the minimum q within the wave by cross-lane moves, within the
//                              workgroup through four LDS words, and across workgroups by an agent-scope atomic min on the bits
//                              of q (non-negative floats order as their bits).  The workgroup that draws the last ticket
//                              commits: it takes the word (and re-arms it) with an atomic exchange, evaluates the scalar tail
//                              of timestep_common.h once, writes dt for the next launch, advances the float64 t, counts, logs,
//                              and puts the ticket back to zero.  The word and the ticket are only ever touched by returning
//                              agent-scope atomics, each issued after the previous one has returned, so nothing has to be
//                              published through a cache write-back; everything else the commit touches is read and written
//                              by one thread per launch and crosses launches at the kernel boundary.
//   ensemble_timestep_kernel   one workgroup per member, the same statement, no cross-workgroup stage.
//
// Rows at or beyond n (the pad rows of an ensemble's stride) are never read.  The minimum of floats is exact in any order and
// the tail runs once, so the result does not depend on the grid: tests/test_gpu_adaptive.py and test_gpu_adaptive_edges.py hold
// it to the host path bit for bit.
#include "timestep.h"
#include "timestep_common.h"

namespace nb {

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = TIMESTEP_THREADS / WAVE;

__device__ __forceinline__ float min_lt(float a, float b) { return b < a ? b : a; }

// min over rows [first, n) in steps of `stride_threads`, then over the workgroup; valid in thread 0
__device__ __forceinline__ float block_min_q(const float2 *__restrict__ acc, const float *__restrict__ radius, uint32_t n, uint32_t first,
                                             uint32_t stride_threads, float *lds) {
    float q = NB_TS_INF;
    for (uint32_t i = first; i < n; i += stride_threads) {
        const float2 a = acc[i];
        q = min_lt(q, nb_timestep_q(a.x, a.y, radius[i]));
    }
    for (int d = WAVE / 2; d > 0; d >>= 1) q = min_lt(q, __shfl_xor(q, d, WAVE));
    if ((threadIdx.x & (WAVE - 1)) == 0) lds[threadIdx.x / WAVE] = q;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < WAVES; w++) q = min_lt(q, lds[w]);
    return q;
}

// the scalar tail, once per step and world (one thread)
__device__ __forceinline__ void commit(const TimestepParams &p, float q, AdaptState *st, float *dt_out, float *log) {
    float dt = nb_timestep_dt(q, p.eta, p.dt_min, p.dt_max);
    if (p.commit) {
        double t = st->t;
        dt = nb_timestep_clip(dt, p.span, &t);
        uint32_t steps = st->steps, idle = st->idle_steps;
        float last = st->dt_last, smallest = st->dt_smallest;
        nb_timestep_count(dt, &steps, &idle, &last, &smallest);
        st->t = t;
        st->steps = steps;
        st->idle_steps = idle;
        st->dt_last = last;
        st->dt_smallest = smallest;
        if (log) *log = dt;
    }
    *dt_out = dt;
}

}  // namespace

__global__ __launch_bounds__(TIMESTEP_THREADS) void timestep_kernel(TimestepParams p) {
    __shared__ float lds[WAVES];
    const float q = block_min_q(p.acc, p.radius, p.n, blockIdx.x * TIMESTEP_THREADS + threadIdx.x, gridDim.x * TIMESTEP_THREADS, lds);
    if (threadIdx.x != 0) return;
    AdaptState *st = p.state;
    const uint32_t before = __hip_atomic_fetch_min(&st->qbits, __float_as_uint(q), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" : : "v"(before) : "memory");   // the min has been applied before the ticket is drawn
    const uint32_t arrived = __hip_atomic_fetch_add(&st->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arrived + 1 != gridDim.x) return;
    const uint32_t bits = __hip_atomic_exchange(&st->qbits, Q_ARMED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // take and re-arm
    __hip_atomic_store(&st->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    commit(p, __uint_as_float(bits), st, p.dt_out, p.log);
}

__global__ __launch_bounds__(TIMESTEP_THREADS) void ensemble_timestep_kernel(TimestepParams p) {
    __shared__ float lds[WAVES];
    const uint32_t b = blockIdx.x;
    const size_t row0 = (size_t)b * p.stride;
    const float q = block_min_q(p.acc + row0, p.radius + row0, p.n, threadIdx.x, TIMESTEP_THREADS, lds);
    if (threadIdx.x != 0) return;
    commit(p, q, p.state + b, p.dt_out + b, p.log ? p.log + b : nullptr);
}

__global__ __launch_bounds__(TIMESTEP_THREADS) void timestep_arm_kernel(AdaptState *state, uint32_t count) {
    const uint32_t i = blockIdx.x * TIMESTEP_THREADS + threadIdx.x;
    if (i >= count) return;
    AdaptState s;
    s.t = 0.0;
    s.steps = 0;
    s.idle_steps = 0;
    s.dt_last = 0.0f;
    s.dt_smallest = 0.0f;
    s.qbits = Q_ARMED;
    s.ticket = 0;
    state[i] = s;
}

void launch_arm(hipStream_t st, AdaptState *state, uint32_t count) {
    hipLaunchKernelGGL(timestep_arm_kernel, dim3((count + TIMESTEP_THREADS - 1) / TIMESTEP_THREADS), dim3(TIMESTEP_THREADS), 0, st, state, count);
}

void launch_timestep(hipStream_t st, const TimestepParams &p) {
    hipLaunchKernelGGL(timestep_kernel, dim3(timestep_groups(p.n)), dim3(TIMESTEP_THREADS), 0, st, p);
}

void launch_ensemble_timestep(hipStream_t st, const TimestepParams &p, uint32_t count) {
    hipLaunchKernelGGL(ensemble_timestep_kernel, dim3(count), dim3(TIMESTEP_THREADS), 0, st, p);
}

}  // namespace nb
