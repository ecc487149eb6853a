// leapfrog.h -- internal (C++) interface between the pipelines and the kick / drift passes of leapfrog.hip.
// The arithmetic is leapfrog_common.h; this is only who launches what.  Not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nb {

struct LeapfrogParams {
    float2 *pos;            // [n] (ensemble: [count][stride]); the opening pass drifts it in place
    float2 *vel;
    const float2 *acc;
    const float *dt_close;  // the step size of the closing kick: one word (ensemble: [count]); unused without a close
    const float *dt_open;   // the step size of the opening kick and the drift; unused without an open
    uint32_t n;             // particles (per member); rows at or beyond n are neither read nor written
    uint32_t stride;        // ensemble only: rows per member
};

constexpr uint32_t LEAPFROG_THREADS = 256;
constexpr uint32_t LEAPFROG_MAX_GROUPS = 2048;   // eight workgroups per compute unit: a grid-stride loop covers the rest

inline uint32_t leapfrog_groups(uint32_t n) {
    const uint32_t g = (n + LEAPFROG_THREADS - 1) / LEAPFROG_THREADS;
    return g == 0 ? 1 : g > LEAPFROG_MAX_GROUPS ? LEAPFROG_MAX_GROUPS : g;
}

// One launch: the previous step's close (if `close`), then the next step's open (if `open`), per particle.
// count = 0: one world; otherwise an ensemble of `count` members, grid (ceil(stride / 256), count).
void launch_leapfrog(hipStream_t st, const LeapfrogParams &p, bool close, bool open, uint32_t count);

}  // namespace nb
