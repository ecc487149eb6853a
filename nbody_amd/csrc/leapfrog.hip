// leapfrog.hip -- the O(N) passes of a kick-drift-kick step (include/nbody_leapfrog.h; the statement: leapfrog_common.h).
// A leapfrog step is open(dt), a dt = 0 force launch of the ordinary stepper, close(dt); the step kernels stay as they are.
//
//   leapfrog_kernel<CLOSE, OPEN>   one grid-stride pass over the particles.  CLOSE adds the closing half kick of the step
//                                  that just had its force evaluated, OPEN the opening half kick and the drift of the next
//                                  one, so one launch between two force launches serves both: 24 bytes in (vel, acc, pos)
//                                  and 16 out (vel, pos) per particle, 16 in and 8 out for a close alone.  The two kicks stay
//                                  two roundings of v -- nothing is merged -- so the bits do not depend on where a call ends.
//
// The step sizes are read from device memory (one word per world, dt[b] per ensemble member); the half step h is formed here.
// Consecutive lanes touch consecutive float2 rows: every access is one coalesced 512-byte request per wave.  Positions are
// updated in place in the array the next force launch reads as receivers and as sources (an unsharded pipeline's sources
// are its position array itself).  Ensembles use batch.hip's [count][stride] layout, one grid row per member; rows at or
// beyond n (the pad rows of a stride) are never touched.  No LDS, no scratch, no atomics.
#include "leapfrog.h"
#include "leapfrog_common.h"

namespace nb {

namespace {

template <bool CLOSE, bool OPEN>
__device__ __forceinline__ void leapfrog_rows(float2 *__restrict__ pos, float2 *__restrict__ vel, const float2 *__restrict__ acc, uint32_t n,
                                              float dt_close, float dt_open) {
    const float h_close = nb_leapfrog_half(dt_close), h_open = nb_leapfrog_half(dt_open);
    for (uint32_t i = blockIdx.x * LEAPFROG_THREADS + threadIdx.x; i < n; i += gridDim.x * LEAPFROG_THREADS) {
        const float2 a = acc[i];
        float2 v = vel[i];
        if constexpr (CLOSE) {
            v.x = nb_leapfrog_kick(v.x, a.x, h_close);
            v.y = nb_leapfrog_kick(v.y, a.y, h_close);
        }
        if constexpr (OPEN) {
            v.x = nb_leapfrog_kick(v.x, a.x, h_open);
            v.y = nb_leapfrog_kick(v.y, a.y, h_open);
            float2 q = pos[i];
            q.x = nb_leapfrog_drift(q.x, v.x, dt_open);
            q.y = nb_leapfrog_drift(q.y, v.y, dt_open);
            pos[i] = q;
        }
        vel[i] = v;
    }
}

}  // namespace

template <bool CLOSE, bool OPEN>
__global__ __launch_bounds__(LEAPFROG_THREADS) void leapfrog_kernel(LeapfrogParams p) {
    leapfrog_rows<CLOSE, OPEN>(p.pos, p.vel, p.acc, p.n, CLOSE ? *p.dt_close : 0.0f, OPEN ? *p.dt_open : 0.0f);
}

template <bool CLOSE, bool OPEN>
__global__ __launch_bounds__(LEAPFROG_THREADS) void ensemble_leapfrog_kernel(LeapfrogParams p) {
    const uint32_t b = blockIdx.y;
    const size_t row0 = (size_t)b * p.stride;
    leapfrog_rows<CLOSE, OPEN>(p.pos + row0, p.vel + row0, p.acc + row0, p.n, CLOSE ? p.dt_close[b] : 0.0f, OPEN ? p.dt_open[b] : 0.0f);
}

namespace {

template <bool CLOSE, bool OPEN>
void launch_as(hipStream_t st, const LeapfrogParams &p, uint32_t count) {
    if (count == 0)
        hipLaunchKernelGGL((leapfrog_kernel<CLOSE, OPEN>), dim3(leapfrog_groups(p.n)), dim3(LEAPFROG_THREADS), 0, st, p);
    else
        hipLaunchKernelGGL((ensemble_leapfrog_kernel<CLOSE, OPEN>), dim3((p.stride + LEAPFROG_THREADS - 1) / LEAPFROG_THREADS, count),
                           dim3(LEAPFROG_THREADS), 0, st, p);
}

}  // namespace

void launch_leapfrog(hipStream_t st, const LeapfrogParams &p, bool close, bool open, uint32_t count) {
    if (p.n == 0 || (!close && !open)) return;
    if (close && open)
        launch_as<true, true>(st, p, count);
    else if (close)
        launch_as<true, false>(st, p, count);
    else
        launch_as<false, true>(st, p, count);
}

}  // namespace nb
