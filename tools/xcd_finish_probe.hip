// xcd_finish_probe: does each XCD work through its own share of a large grid at its own pace, or does the dispatcher
// place workgroups in grid order across the XCDs so that all eight finish together?
//
// The odd XCDs hold about 2 % less clock than the even ones under the step kernel (DESIGN.md §3 "Held clock").  A scheme
// that hands work out by speed can only pay if a fast XCD runs AHEAD of a slow one inside a launch.  This probe measures
// that: a 1-D grid of 16 384 workgroups of 1 024 threads (the headline launch's 32 resident rounds), every workgroup
// running the paired interaction statement of interaction_asm.h over the same fixed source count (as the loop of
// clock_probe.hip does), thread 0 stamping the XCD id, s_memrealtime and s_memtime at entry and at the workgroup's exit.
// Per XCD it reports how many workgroups it ran, when its first entered and its last left (relative to the launch's
// first entry), the clock its workgroups saw, and how far it had got at the quarter points of the launch.
//
//   hipcc -O3 --offload-arch=gfx950 -I nbody_amd/csrc tools/xcd_finish_probe.hip -o tools/xcd_finish_probe
//   tools/xcd_finish_probe [workgroup_ms=1.5] [launches=2]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "interaction_asm.h"

#define CHECK(x)                                                              \
    do {                                                                      \
        hipError_t e = (x);                                                   \
        if (e != hipSuccess) {                                                \
            printf("%s failed: %s\n", #x, hipGetErrorString(e));              \
            return 1;                                                         \
        }                                                                     \
    } while (0)

constexpr int WAVES = 16;             // 1 024 threads, two workgroups per CU, 8 waves per SIMD: the N = 2^20 shape
constexpr uint32_t GROUPS = 16384;    // 32 rounds of the 512 resident workgroups

struct Stamp {
    uint64_t ref_in, ref_out;         // s_memrealtime (constant 100 MHz) at entry and at exit
    uint64_t cyc_in, cyc_out;         // s_memtime (shader cycles of this XCD) at the same two points
    uint32_t xcc, pad;
};

__global__ __launch_bounds__(64 * WAVES, 8) void finish_probe_kernel(const float *__restrict__ src, uint32_t iters, Stamp *__restrict__ stamps,
                                                                     float *__restrict__ sink) {
    const uint32_t tid = threadIdx.x;
    uint32_t id = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    const uint64_t c0 = __builtin_amdgcn_s_memtime();
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    float sx[8], sy[8], sg[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        sx[u] = src[2 * u];
        sy[u] = src[2 * u + 1];
        sg[u] = src[16 + u];
    }
    float px0 = 1000.0f + (float)tid, py0 = -500.0f + (float)(blockIdx.x & 1023u), r0 = 2.0f;
    float px1 = -3000.0f - (float)tid, py1 = 700.0f + (float)(blockIdx.x & 1023u), r1 = 3.0f;
    float ax0 = 0.f, ay0 = 0.f, ax1 = 0.f, ay1 = 0.f;
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    for (uint32_t i = 0; i < iters; i++) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            asm(NB_INTERACTION2_ASM
                : [ax0] "+v"(ax0), [ay0] "+v"(ay0), [ax1] "+v"(ax1), [ay1] "+v"(ay1)
                : [sx] "s"(sx[u]), [sy] "s"(sy[u]), [g] "s"(sg[u]), [px0] "v"(px0), [py0] "v"(py0), [r0] "v"(r0), [px1] "v"(px1),
                  [py1] "v"(py1), [r1] "v"(r1)
                : NB_CLOBBERS2);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::"v"(ax0), "v"(ay0), "v"(ax1), "v"(ay1));
    // the exit stamp is the WORKGROUP's: its slot on the CU is free for the next workgroup once all sixteen waves are through
    __syncthreads();
    const uint64_t c1 = __builtin_amdgcn_s_memtime();
    const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_sched_barrier(0);
    if (tid == 0) {
        Stamp s;
        s.ref_in = t0;
        s.ref_out = t1;
        s.cyc_in = c0;
        s.cyc_out = c1;
        s.xcc = id & 0xfu;
        s.pad = 0;
        stamps[blockIdx.x] = s;
    }
    if (ax0 + ay0 + ax1 + ay1 == 12345.678f) sink[tid] = ax0;
}

static double median(std::vector<double> v) {
    if (v.empty()) return 0.0;
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char **argv) {
    const double wg_ms = argc > 1 ? atof(argv[1]) : 1.5;
    const int launches = argc > 2 ? atoi(argv[2]) : 2;
    if (!(wg_ms > 0.0 && wg_ms <= 5.0) || launches < 1 || launches > 8) {
        printf("usage: xcd_finish_probe [workgroup_ms in (0, 5]] [launches 1..8]\n");
        return 2;
    }
    int dev = 0, wall_khz = 0, cus = 0;
    CHECK(hipGetDevice(&dev));
    if (hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || wall_khz <= 0) {
        (void)hipGetLastError();
        wall_khz = 100000;
    }
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const double khz = (double)wall_khz;   // s_memrealtime ticks per millisecond
    // one loop trip = 8 sources x 2 receivers = 16 wave-interactions per wave, 8 waves per SIMD, ~27 cycles each at ~2.3 GHz
    const double trip_us = 16.0 * 8.0 * 27.0 / 2300.0;
    const uint32_t iters = (uint32_t)std::max(16.0, wg_ms * 1000.0 / trip_us);

    float host_src[24];
    for (int u = 0; u < 8; u++) {
        host_src[2 * u] = 11.0f * (float)u;
        host_src[2 * u + 1] = -7.0f * (float)u;
        host_src[16 + u] = 1.0e4f + (float)u;
    }
    float *src, *sink;
    Stamp *stamps;
    CHECK(hipMalloc(&src, sizeof host_src));
    CHECK(hipMalloc(&sink, 64 * WAVES * sizeof(float)));
    CHECK(hipMalloc(&stamps, GROUPS * sizeof(Stamp)));
    CHECK(hipMemcpy(src, host_src, sizeof host_src, hipMemcpyHostToDevice));
    hipStream_t st;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    std::vector<Stamp> h(GROUPS);

    printf("xcd_finish_probe: %u workgroups x %d threads, %u loop trips each (aimed at %.2f ms per workgroup), %d CUs, reference clock %.0f MHz\n",
           GROUPS, 64 * WAVES, iters, wg_ms, cus, khz * 1.0e-3);
    // launch 0 warms the clock up (and is reported: it shows the ramp); the later ones are the measurement
    for (int l = 0; l <= launches; l++) {
        CHECK(hipMemsetAsync(stamps, 0, GROUPS * sizeof(Stamp), st));
        hipLaunchKernelGGL(finish_probe_kernel, dim3(GROUPS), dim3(64 * WAVES), 0, st, src, iters, stamps, sink);
        CHECK(hipGetLastError());
        CHECK(hipMemcpyAsync(h.data(), stamps, GROUPS * sizeof(Stamp), hipMemcpyDeviceToHost, st));
        CHECK(hipStreamSynchronize(st));

        uint64_t first_in = ~0ull, last_out = 0;
        for (const Stamp &s : h) {
            if (s.ref_out == 0) continue;
            first_in = std::min(first_in, s.ref_in);
            last_out = std::max(last_out, s.ref_out);
        }
        if (last_out == 0) {
            printf("launch %d: no workgroup reported a stamp\n", l);
            return 1;
        }
        const double launch_ms = (double)(last_out - first_in) / khz;
        struct PerXcd {
            uint32_t n = 0, in_order = 0;
            double first_in = 1e30, last_out = 0.0;
            std::vector<double> ghz, life, outs;
        } x[8];
        // which residue of blockIdx % 8 does each XCD mostly run?  (static round-robin dealing: all of one residue)
        uint32_t residue[8][8] = {};
        for (uint32_t b = 0; b < GROUPS; b++) {
            const Stamp &s = h[b];
            if (s.ref_out == 0) continue;
            PerXcd &p = x[s.xcc & 7u];
            p.n++;
            residue[s.xcc & 7u][b & 7u]++;
            const double tin = (double)(s.ref_in - first_in) / khz, tout = (double)(s.ref_out - first_in) / khz;
            p.first_in = std::min(p.first_in, tin);
            p.last_out = std::max(p.last_out, tout);
            p.outs.push_back(tout);
            p.life.push_back(tout - tin);
            if (s.ref_out > s.ref_in) p.ghz.push_back((double)(s.cyc_out - s.cyc_in) / (double)(s.ref_out - s.ref_in) * khz * 1.0e-6);
        }
        printf("\nlaunch %d%s: %.3f ms from the first entry to the last exit\n", l, l == 0 ? " (warm-up)" : "", launch_ms);
        printf("xcd  workgroups  of one blockIdx%%8  first_in_ms  last_out_ms  last_out/launch  clock_ghz  wg_life_ms  done@25%%  done@50%%  done@75%%\n");
        double lo = 1e30, hi = 0.0, even_last = 0.0, odd_last = 0.0, even_sum = 0.0, odd_sum = 0.0, f_sum = 0.0, f_min = 1e30;
        int n_even = 0, n_odd = 0;
        int n_xcd = 0;
        for (int k = 0; k < 8; k++) {
            PerXcd &p = x[k];
            if (p.n == 0) continue;
            n_xcd++;
            const uint32_t top = *std::max_element(residue[k], residue[k] + 8);
            uint32_t done[3] = {0, 0, 0};
            for (double t : p.outs)
                for (int q = 0; q < 3; q++)
                    if (t <= launch_ms * 0.25 * (q + 1)) done[q]++;
            const double f = median(p.ghz);
            printf("%3d  %10u  %15.4f  %11.3f  %11.3f  %15.5f  %9.4f  %10.4f  %8u  %8u  %8u\n", k, p.n, (double)top / p.n, p.first_in, p.last_out,
                   p.last_out / launch_ms, f, median(p.life), done[0], done[1], done[2]);
            lo = std::min(lo, p.last_out);
            hi = std::max(hi, p.last_out);
            (k & 1 ? odd_last : even_last) = std::max(k & 1 ? odd_last : even_last, p.last_out);
            (k & 1 ? odd_sum : even_sum) += p.last_out;
            (k & 1 ? n_odd : n_even)++;
            f_sum += f;
            f_min = std::min(f_min, f);
        }
        const double f_mean = f_sum / std::max(1, n_xcd);
        printf("spread of last exits: %.3f ms = %.5f of the launch;  even XCDs' last exit %.3f ms, odd XCDs' %.3f ms: odd - even = %.5f of the launch\n",
               hi - lo, (hi - lo) / launch_ms, even_last, odd_last, (odd_last - even_last) / launch_ms);
        if (n_even && n_odd)
            printf("mean last exit of the even XCDs %.3f ms, of the odd XCDs %.3f ms: odd - even = %.5f of the launch\n", even_sum / n_even, odd_sum / n_odd,
                   (odd_sum / n_odd - even_sum / n_even) / launch_ms);
        printf("clock under this launch: mean of the XCD medians %.4f GHz, slowest XCD %.4f GHz: 1 - f_slowest / f_mean = %.5f\n", f_mean, f_min,
               1.0 - f_min / f_mean);
    }
    CHECK(hipStreamDestroy(st));
    CHECK(hipFree(src));
    CHECK(hipFree(sink));
    CHECK(hipFree(stamps));
    return 0;
}
