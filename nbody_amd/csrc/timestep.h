// timestep.h -- internal (C++) interface between the pipelines and the adaptive step-size kernels (timestep.hip).
// The arithmetic is timestep_common.h; this is only who launches what.  Not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "nbody_adaptive.h"

namespace nb {

// What one world's adaptive call keeps on the device between its steps: the NbAdaptiveResult in the making and, for the
// one-world kernel, the word the workgroups reduce into and their arrival ticket.  32 bytes; an ensemble holds one per member.
struct AdaptState {
    double t;            // time covered by this call, float64
    uint32_t steps;      // steps with dt > 0
    uint32_t idle_steps;
    float dt_last;
    float dt_smallest;   // 0 until the first dt > 0
    uint32_t qbits;      // min over the workgroups of the bits of q (non-negative floats order as their bits); armed at +inf
    uint32_t ticket;     // workgroups that have arrived; the last one commits and puts it back to 0
};
static_assert(sizeof(AdaptState) == 32, "AdaptState is copied to the host as 32-byte records");

constexpr uint32_t Q_ARMED = 0x7f800000u;   // the bits of +inf

struct TimestepParams {
    const float2 *acc;     // [n] (ensemble: [count][stride])
    const float *radius;
    uint32_t n;            // particles (per member); rows at or beyond n are never read
    uint32_t stride;       // ensemble only: rows per member
    float eta, dt_min, dt_max;
    double span;
    AdaptState *state;     // one record (ensemble: [count])
    float *dt_out;         // where the next step launch reads its step size (ensemble: [count])
    float *log;            // this step's slot (ensemble: this step's row of [count]); may be null
    uint32_t commit;       // 1: advance t, count, log; 0: the criterion alone (dt_out only, no clip)
};

// what a call reports of a record copied back from the device
inline NbAdaptiveResult adaptive_result(const void *record) {
    AdaptState st;
    memcpy(&st, record, sizeof st);
    return NbAdaptiveResult{st.t, st.steps, st.idle_steps, st.dt_last, st.dt_smallest};
}

// the fields a world and an ensemble fill alike; state, dt_out, log and commit are the caller's
inline TimestepParams timestep_params(const float2 *acc, const float *radius, uint32_t n, uint32_t stride, const NbAdaptive &cfg) {
    TimestepParams p;
    memset(&p, 0, sizeof p);
    p.acc = acc;
    p.radius = radius;
    p.n = n;
    p.stride = stride;
    p.eta = cfg.eta;
    p.dt_min = cfg.dt_min;
    p.dt_max = cfg.dt_max;
    p.span = cfg.span;
    return p;
}

constexpr uint32_t TIMESTEP_THREADS = 256;
constexpr uint32_t TIMESTEP_MAX_GROUPS = 32;   // four per XCD: a grid-stride read of 12 bytes per particle needs no more

inline uint32_t timestep_groups(uint32_t n) {
    const uint32_t g = (n + TIMESTEP_THREADS - 1) / TIMESTEP_THREADS;
    return g == 0 ? 1 : g > TIMESTEP_MAX_GROUPS ? TIMESTEP_MAX_GROUPS : g;
}

// state[0 .. count) = a call's starting record (t = 0, nothing counted, word armed, ticket 0), in stream order
void launch_arm(hipStream_t st, AdaptState *state, uint32_t count);
// one world: timestep_groups(p.n) workgroups; the last to arrive commits
void launch_timestep(hipStream_t st, const TimestepParams &p);
// an ensemble: one workgroup per member
void launch_ensemble_timestep(hipStream_t st, const TimestepParams &p, uint32_t count);

}  // namespace nb
